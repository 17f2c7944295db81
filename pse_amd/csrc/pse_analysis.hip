// Kernels of the analyses (pse_analysis.h): the pair-distance histogram and the cluster analysis on the engine's cell list, the static
// structure factor and the displacement moments on the caller-order arrays.  They stand beside the path and read what the step leaves;
// nothing here writes a force.  The bond-orientational order has a unit of its own (pse_order.hip).  gfx950, wave64, fp64.
#include "pse_analysis.h"
#include "pse_excl.h"

namespace pse {

// Pair-distance histogram (pse_pair_hist_accumulate): the distances of all unordered pairs, one row of nbins uniform bins on
// [rmin, rmax) per pair type p(a, b) -- the raw counts of the radial distribution functions g_ab(r).  A kernel of its own, as
// k_pair_table_typed is (see the note on shared code above k_pair_repulsion); the walk, the type mirror (k_type_mirror) and the
// exclusion lookup are those of k_pair_table_typed.  One thread per sorted row i; a pair j > i -- every unordered pair once, the
// rule of the OBS sums -- with r^2 < rmax^2, r^2 > 0, r = sqrt(r^2) >= rmin that is not excluded adds 1 to counter p nbins + b,
// b = min((int)((r - rmin) scale), nbins - 1): r within an ulp of rmax may give t = nbins, the clamp keeps it in the last bin.
// Counters: `ncount` = npt nbins <= PAIR_HIST_MAX_COUNTERS unsigned words of dynamic LDS (at most 32 KB), zeroed by the workgroup
// before one barrier and added to by ds_add_u32 without a returned value.  Behind the walk and ONE more barrier the workgroup adds
// its non-zero counters to the caller's 64-bit counters with global integer atomics without a returned value.  An LDS counter holds
// the pairs of 256 rows: no overflow.  No floating point is summed: every count is exact and independent of the order, equal inputs
// give equal bits.  No lane leaves before either barrier.
// Measured and dropped (docs/HISTORY.md): a copy of the counters per wave (no difference, at one bin as at 128), and several row
// blocks per workgroup before the flush (slower at 10^6 and 10^7 rows: fewer workgroups hide the gathers worse than the flush costs).
template <bool EXCL>
__global__ void __launch_bounds__(TPB)
k_pair_hist(const double4 *__restrict__ pos_s, const unsigned *__restrict__ tag_s, const unsigned char *__restrict__ type_s, int N,
            const int *__restrict__ cell_off, DBox box, DCells nc, int ntypes, int nbins, int ncount, double rmin, double rmax2, double scale,
            unsigned long long *__restrict__ counts /* [ncount], added to */, ExclRows ex) {
    extern __shared__ unsigned ph_cnt[];   // [ncount]
    for (int c = threadIdx.x; c < ncount; c += TPB) ph_cnt[c] = 0u;
    __syncthreads();
    const int blast = nbins - 1;
    const int i = xcd_block(blockIdx.x, gridDim.x) * TPB + threadIdx.x;
    if (i < N) {
        const double4 pi = pos_s[i];
        double fx, fy, fz;
        frac_coords(box, pi.x, pi.y, pi.z, fx, fy, fz);
        const int cx = cell_coord(fx, nc.nx), cy = cell_coord(fy, nc.ny), cz = cell_coord(fz, nc.nz);
        const int ti = type_s[i];
        unsigned eb = 0u, ee = 0u;
        if (EXCL) excl_row(ex, tag_s[i], eb, ee);
        for_each_run(nc, cell_off, cx, cy, cz, [&](int jb, int je, unsigned) {
            for (int j = max(jb, i + 1); j < je; ++j) {
                const double4 pj = pos_s[j];
                double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                min_image(box, dx, dy, dz);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (r2 < rmax2 && r2 > 0.0) {
                    const double r = sqrt(r2);
                    if (r >= rmin && !(EXCL && eb < ee && excl_has(ex.ent, eb, ee, tag_s[j]))) {
                        const int tj = type_s[j];
                        const int lo = min(ti, tj), hi = max(ti, tj);
                        const int p = lo * ntypes - ((lo * (lo - 1)) >> 1) + (hi - lo);
                        const int bin = min((int)((r - rmin) * scale), blast);
                        atomicAdd(ph_cnt + p * nbins + bin, 1u);
                    }
                }
            }
        });
    }
    __syncthreads();
    for (int c = threadIdx.x; c < ncount; c += TPB) {
        const unsigned v = ph_cnt[c];
        if (v) atomicAdd(counts + c, (unsigned long long)v);
    }
}
void launch_pair_hist(const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc, const PairHist &ph,
                      unsigned long long *counts, hipStream_t s, const PairExclusions *ex) {
    static_assert((size_t)PAIR_HIST_MAX_COUNTERS * sizeof(unsigned) <= 32768, "the counters take at most 32 KB of LDS");
    const int nb = nblocks(N, TPB);
    const int ncount = ph.ntypes * (ph.ntypes + 1) / 2 * ph.nbins;
    const size_t lds = (size_t)ncount * sizeof(unsigned);
    const double scale = (double)ph.nbins / (ph.rmax - ph.rmin);
    launch_type_mirror(tag_s, N, ph.types, ph.n, ph.type_s, s);
    launch_with_excl(ex, [&](auto excl, ExclRows er) {
        hipLaunchKernelGGL((k_pair_hist<decltype(excl)::value>), dim3(nb), dim3(TPB), lds, s, pos_s, tag_s, ph.type_s, N, cell_off, box,
                           nc, ph.ntypes, ph.nbins, ncount, ph.rmin, ph.rmax * ph.rmax, scale, counts, er);
    });
}

// Cluster analysis (pse_clusters_label): the connected components of the graph whose edges are the pairs with 0 < r^2 < rlink[p]^2,
// p the pair type, that are not excluded.  A lock-free union-find over the SORTED ROWS -- neighbours in space are neighbours in memory
// there -- in five launches behind the sort: k_type_mirror, k_cluster_init, k_cluster_link, k_cluster_flatten, k_cluster_write.
// parent[x] <= x always: a row is its own root until ONE compare-and-swap hooks it under a smaller row, and nothing else ever writes
// parent[x] while x is a root (path halving points a row that is NOT a root at a smaller row of its own tree: the inequality stays,
// trees only ever merge, and every walk still ends at the one root of the tree).  Hence
//   find(x) follows strictly decreasing rows: at most N loads;
//   unite(i, j) finds both roots, hooks the LARGER under the smaller with atomicCAS(parent + hi, hi, lo), and where the CAS fails --
//     another lane hooked hi first -- continues from the value it returned, which is below hi: the rows it tries to hook decrease
//     strictly, so it fails fewer than N times (and over all lanes at most N - 1 hooks ever succeed).
// No lane ever waits for another.  Every loop nevertheless carries a trip cap of N; a lane that reaches it ORs a bit into the object's
// status word and leaves, and k_cluster_write then writes ~0u labels and zero sizes.
// parent is read with relaxed agent-scope atomic loads (global_load_dword sc1): a plain load may be kept in a register or served from
// this CU's L1.  Nothing depends on how FRESH a load is: an old value of parent[x] is x itself, which the lane takes for a root; the
// CAS, which is decided where the word lives, then fails and returns the truth.  A successful CAS needs hi to be a root, not lo: a root
// hooked under ANY smaller row of the other tree is a valid union.
// The partition and the smallest caller index of a component do not depend on the order in which the hooks happen, and everything
// summed is an integer: equal inputs give equal outputs, and a permuted particle order gives the same labels.
// Path halving in k_cluster_link (cluster_find<true>) was measured against the plain walk at N = 10^6 (docs/HISTORY.md): one cluster of
// 10^6 rows 1.70 ms against 2.44, below the threshold 0.59 against 0.57 and 0.86 against 0.80; kept.  k_cluster_flatten walks without it
// and shortens every path to one hop.
constexpr unsigned CLUSTER_CAP_FIND = 1u, CLUSTER_CAP_UNITE = 2u;   // bits of the status word
__device__ __forceinline__ unsigned cluster_parent(const unsigned *parent, unsigned x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The root of x's tree, or ~0u behind the trip cap (never reached: x, parent[x], ... decrease strictly and x < cap = N).
// HALVE: path halving -- a row that is not a root is pointed at its grandparent on the way (a relaxed store: parent[x] stays a row
// of x's own tree below x, whichever of two racing stores lands last and however old the values they were made from; the CAS of
// cluster_unite only ever succeeds on a root, and a row that has stopped being a root never becomes one again).
template <bool HALVE>
__device__ __forceinline__ unsigned cluster_find(unsigned *parent, unsigned x, unsigned cap, unsigned *status) {
    for (unsigned trip = 0; trip < cap; ++trip) {
        const unsigned p = cluster_parent(parent, x);
        if (p == x) return x;
        if (HALVE) {
            const unsigned gp = cluster_parent(parent, p);
            if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            x = gp;
        } else {
            x = p;
        }
    }
    atomicOr(status, CLUSTER_CAP_FIND);
    return ~0u;
}
__device__ __forceinline__ void cluster_unite(unsigned *parent, unsigned a, unsigned b, unsigned cap, unsigned *status) {
    for (unsigned trip = 0; trip < cap; ++trip) {
        a = cluster_find<true>(parent, a, cap, status);
        b = cluster_find<true>(parent, b, cap, status);
        if (a == b || a == ~0u || b == ~0u) return;
        const unsigned hi = max(a, b), lo = min(a, b);
        const unsigned seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return;
        a = seen; b = lo;   // hi was hooked by another lane, under seen < hi
    }
    atomicOr(status, CLUSTER_CAP_UNITE);
}
__global__ void __launch_bounds__(TPB)
k_cluster_init(int N, unsigned *__restrict__ parent, unsigned *__restrict__ mintag, unsigned *__restrict__ csize,
               unsigned long long *__restrict__ stats /* may be null */) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < N) { parent[i] = (unsigned)i; mintag[i] = ~0u; csize[i] = 0u; }
    if (stats && i < 4) stats[i] = 0ull;
}
// One thread per sorted row i, the rows j > i of its 27 cells -- every unordered pair once, the walk of k_pair_hist written out the
// same way.  rl2[p] = rlink[p]^2 (0: off) of at most 36 pair types staged in LDS; per pair the wave-uniform prefilter
// r^2 < max_p rl2 and r^2 > 0 first, behind it the partner's type byte, the pair type's own rl2 and, with EXCL, the lookup of
// k_pair_table_typed.  A linked pair calls cluster_unite(i, j).  No lane leaves before the barrier.
template <bool EXCL>
__global__ void __launch_bounds__(TPB)
k_cluster_link(const double4 *__restrict__ pos_s, const unsigned *__restrict__ tag_s, const unsigned char *__restrict__ type_s, int N,
               const int *__restrict__ cell_off, DBox box, DCells nc, int ntypes, const double *__restrict__ rlink2 /* npt */, double rl2_all,
               unsigned *parent, unsigned *status, ExclRows ex) {
    __shared__ double rl2[PAIR_TYPED_MAX_PAIR_TYPES];
    if ((int)threadIdx.x < ntypes * (ntypes + 1) / 2) rl2[threadIdx.x] = rlink2[threadIdx.x];
    __syncthreads();
    const int i = xcd_block(blockIdx.x, gridDim.x) * TPB + threadIdx.x;
    if (i < N) {
        const double4 pi = pos_s[i];
        double fx, fy, fz;
        frac_coords(box, pi.x, pi.y, pi.z, fx, fy, fz);
        const int cx = cell_coord(fx, nc.nx), cy = cell_coord(fy, nc.ny), cz = cell_coord(fz, nc.nz);
        const int ti = type_s[i];
        unsigned eb = 0u, ee = 0u;
        if (EXCL) excl_row(ex, tag_s[i], eb, ee);
        for_each_run(nc, cell_off, cx, cy, cz, [&](int jb, int je, unsigned) {
            for (int j = max(jb, i + 1); j < je; ++j) {
                const double4 pj = pos_s[j];
                double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                min_image(box, dx, dy, dz);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (r2 < rl2_all && r2 > 0.0) {
                    const int tj = type_s[j];
                    const int lo = min(ti, tj), hi = max(ti, tj);
                    const int p = lo * ntypes - ((lo * (lo - 1)) >> 1) + (hi - lo);
                    if (r2 < rl2[p] && !(EXCL && eb < ee && excl_has(ex.ent, eb, ee, tag_s[j])))
                        cluster_unite(parent, (unsigned)i, (unsigned)j, (unsigned)N, status);
                }
            }
        });
    }
}
// Every row learns its root and stores it back (one hop from now on); the root collects the smallest caller index and the number of
// members with integer atomics.  A store of a root into parent[i] while another lane walks through i hands that lane an ancestor of i,
// as the old value was.  The rows of a wave are neighbours in space and, in a large cluster, share their root: the lanes whose root
// is that of the wave's first lane reduce among themselves (a butterfly minimum, a ballot count) and ONE of them adds for all; the
// others add for themselves.  (One atomic per row put 2 x 10^6 atomics on two words when the system is one cluster: 11.5 ms of a
// 13.7 ms call at N = 10^6, docs/HISTORY.md.)  No lane leaves before the butterfly.
__global__ void __launch_bounds__(TPB)
k_cluster_flatten(const unsigned *__restrict__ tag_s, int N, unsigned *parent, unsigned *__restrict__ mintag, unsigned *__restrict__ csize,
                  unsigned *status) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    unsigned root = ~0u, tag = ~0u;   // (~0u: a lane past the last row, or one that gave up)
    if (i < N) {
        root = cluster_find<false>(parent, (unsigned)i, (unsigned)N, status);   // (no halving here: k_cluster_write needs parent[i] = root)
        if (root != ~0u) {
            __hip_atomic_store(parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tag = tag_s[i];
        }
    }
    const unsigned lead = __shfl(root, 0, 64);
    const bool with_lead = root != ~0u && root == lead;
    const unsigned long long group = __ballot(with_lead);
    unsigned least = with_lead ? tag : ~0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) least = min(least, (unsigned)__shfl_xor((int)least, o, 64));
    if (with_lead) {
        if ((threadIdx.x & 63) == (unsigned)(__ffsll((long long)group) - 1)) {
            atomicMin(mintag + root, least);
            atomicAdd(csize + root, (unsigned)__popcll(group));
        }
    } else if (root != ~0u) {
        atomicMin(mintag + root, tag);
        atomicAdd(csize + root, 1u);
    }
}
// label and size by caller index; a row that is its own root adds its cluster to stats (clusters, largest, sum s^2, N) and to
// hist[min(s, nhist) - 1].  The workgroup first sums in LDS -- four 64-bit words and the first CLUSTER_LDS_BINS bins, where the small
// clusters of a dilute system all land -- and adds what is not zero to the caller's words behind ONE barrier; a cluster beyond those
// bins adds to its word directly.  A non-zero status word: ~0u labels, zero sizes, stats left at the zeros of k_cluster_init, hist untouched.
constexpr int CLUSTER_LDS_BINS = 64;
__global__ void __launch_bounds__(TPB)
k_cluster_write(const unsigned *__restrict__ tag_s, int N, const unsigned *__restrict__ parent, const unsigned *__restrict__ mintag,
                const unsigned *__restrict__ csize, const unsigned *__restrict__ status, unsigned *__restrict__ label,
                unsigned *__restrict__ size, unsigned long long *__restrict__ stats, unsigned long long *__restrict__ hist, unsigned nhist) {
    __shared__ unsigned long long st[4];
    __shared__ unsigned hb[CLUSTER_LDS_BINS];
    if (threadIdx.x < 4) st[threadIdx.x] = 0ull;
    if (threadIdx.x < CLUSTER_LDS_BINS) hb[threadIdx.x] = 0u;
    __syncthreads();
    const bool gave_up = *status != 0u;
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < N) {
        const unsigned root = parent[i], t = tag_s[i];
        if (label) label[t] = gave_up ? ~0u : mintag[root];
        if (size) size[t] = gave_up ? 0u : csize[root];
        if (!gave_up && root == (unsigned)i) {
            const unsigned long long sz = csize[i];
            if (stats) {
                atomicAdd(st + 0, 1ull);
                atomicMax(st + 1, sz);
                atomicAdd(st + 2, sz * sz);
                atomicAdd(st + 3, sz);
            }
            if (hist) {
                const unsigned long long b = min(sz, (unsigned long long)nhist) - 1ull;
                if (b < (unsigned long long)CLUSTER_LDS_BINS) atomicAdd(hb + (unsigned)b, 1u);
                else atomicAdd(hist + b, 1ull);
            }
        }
    }
    __syncthreads();
    if (stats && threadIdx.x < 4 && st[threadIdx.x]) {
        if (threadIdx.x == 1) atomicMax(stats + 1, st[1]);
        else atomicAdd(stats + threadIdx.x, st[threadIdx.x]);
    }
    if (hist && threadIdx.x < CLUSTER_LDS_BINS && threadIdx.x < nhist && hb[threadIdx.x]) atomicAdd(hist + threadIdx.x, (unsigned long long)hb[threadIdx.x]);
}
void launch_clusters(const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc, const ClusterLinks &cl,
                     unsigned *label, unsigned *size, unsigned long long *stats, unsigned long long *hist, unsigned nhist, hipStream_t s,
                     const PairExclusions *ex) {
    static_assert(PAIR_TYPED_MAX_PAIR_TYPES <= TPB, "one lane stages one link distance");
    const int nb = nblocks(N, TPB);
    launch_type_mirror(tag_s, N, cl.types, cl.n, cl.type_s, s);
    hipLaunchKernelGGL(k_cluster_init, dim3(nb), dim3(TPB), 0, s, N, cl.parent, cl.mintag, cl.csize, stats);
    launch_with_excl(ex, [&](auto excl, ExclRows er) {
        hipLaunchKernelGGL((k_cluster_link<decltype(excl)::value>), dim3(nb), dim3(TPB), 0, s, pos_s, tag_s, cl.type_s, N, cell_off, box, nc,
                           cl.ntypes, cl.rlink2, cl.rl2_all, cl.parent, cl.status, er);
    });
    hipLaunchKernelGGL(k_cluster_flatten, dim3(nb), dim3(TPB), 0, s, tag_s, N, cl.parent, cl.mintag, cl.csize, cl.status);
    hipLaunchKernelGGL(k_cluster_write, dim3(nb), dim3(TPB), 0, s, tag_s, N, cl.parent, cl.mintag, cl.csize, cl.status, label, size, stats,
                       hist, nhist);
}

// Static structure factor (pse_structure_factor_accumulate): rho_a(m) = sum_{j of type a} exp(-2 pi i m.s_j) over a list of integer
// modes m, s the fractional coordinates (x - xy y)/Lx, y/Ly, z/Lz without the 1/2 and without wrapping, and the products
// Re(rho_a conj rho_b).  N x nk complex exponentials, no cell list, nothing sorted: the pass reads pos through `group`.
// Pass 1, k_sf_partial.  The modes come as SEGMENTS (structure_factor_plan): arithmetic progressions m0 + t d of len <= SF_RUN modes of
// the canonically sorted list.  A LANE owns a segment and keeps its SF_RUN complex sums in registers; a workgroup is ONE wave, 64
// segments (a tile), and walks a span of particles -- row `row` of the workspace -- in chunks of SF_CHUNK staged in LDS: each lane
// computes s for four particles (two divisions and a fused multiply-add, so that s_x has two roundings and s_y, s_z one) and
// stores s and the type; then all lanes walk the chunk together.  The particle index is wave-uniform, the LDS reads broadcast, and
// there is NO reduction across lanes: the sum of a mode is formed by one lane in particle order.  Per particle and segment:
// f_c = fma(m_c, s_c, -rint(m_c s_c)) takes the integer part off every product EXACTLY (the fused operation rounds once, a value
// below 1/2), t = f_x + f_y + f_z, t -= rint(t), and sincospi(2 t) is the seed; the same for the step d; then SF_RUN - 1 complex
// multiplications.  Sums past len continue the progression and are not written.  The segments of at most SF_SHORT = 2 modes -- all
// of a scattered list, the ends of runs -- are walked by a second launch of the same kernel with two sums per lane (R = SF_SHORT): one
// step of the recurrence instead of seven.  Nothing takes sin or cos of a large argument.
// Types: the pass runs once per type over the span and skips the particles of the other types -- a wave-uniform branch on a byte
// from LDS, two instructions against the ~150 of a particle that counts -- and restages the chunks per type (1.3 % of the walk per
// type).  Row (row, a) of the workspace, one complex number per distinct mode at its canonical position, is written whole, zeros for a type that is
// absent: the finish reads no stale word.  Two barriers per chunk; no lane leaves before a barrier: a lane past the last segment
// walks a segment of len 0 and writes nothing.
// Pass 2, k_sf_finish: one thread column per distinct mode of the canonical order, SF_FIN_WAVES waves per workgroup that share the rows r = w, w + W, ...;
// each adds its rows in ascending order (four at a time in flight), the waves' sums are added in wave order through LDS: a fixed
// order, no floating-point atomics, equal inputs give equal bits.  Wave 0 then holds rho_a of its mode for all types, writes rho
// and adds the products to sums, at every caller position of the mode (perm[uoff[q] .. uoff[q + 1]): a mode listed twice is computed
// once and has the same bits in both places).
// Measured (docs/HISTORY.md, N = 10^6): 768 modes on the three axes 0.77 ms, 4096 scattered modes 7.6 ms, one type or two.  Measured
// and dropped: one launch with eight sums per lane for every segment -- 9.8 ms on the scattered list, whose segments are pairs.  Not
// built, so not measured: lanes over particles with a tile of mode sums per lane and a wave + LDS reduction per tile, and a
// deterministic partition of the chunk by type.
constexpr int SF_CHUNK = 256;       // particles staged per barrier pair: 6.25 KB of LDS
constexpr int SF_TILE = 64;         // segments per workgroup of k_sf_partial: one wave
constexpr int SF_FIN_WAVES = 16;    // waves of a workgroup of k_sf_finish
__device__ __forceinline__ void sf_phase(double mx, double my, double mz, double sx, double sy, double sz, double &c, double &s) {
    const double fx = fma(mx, sx, -rint(mx * sx)), fy = fma(my, sy, -rint(my * sy)), fz = fma(mz, sz, -rint(mz * sz));
    double t = fx + fy + fz;
    t -= rint(t);
    sincospi(-2.0 * t, &s, &c);   // exp(-2 pi i t)
}
template <int R>
__global__ void __launch_bounds__(SF_TILE)
k_sf_partial(const double4 *__restrict__ pos, const unsigned *__restrict__ group, int N, const unsigned char *__restrict__ types, unsigned ntyped,
             int ntypes, DBox box, const int4 *__restrict__ segs, int nseg, int ntiles, int span, int nu,
             double2 *__restrict__ rows /* [nrows][ntypes][nu] */) {
    __shared__ double sx[SF_CHUNK], sy[SF_CHUNK], sz[SF_CHUNK];
    __shared__ unsigned char st[SF_CHUNK];
    const int lane = threadIdx.x, tile = blockIdx.x % ntiles, row = blockIdx.x / ntiles;
    const int seg = tile * SF_TILE + lane;
    int4 a0 = make_int4(0, 0, 0, 0), a1 = make_int4(0, 0, 0, 0);
    if (seg < nseg) { a0 = segs[2 * seg]; a1 = segs[2 * seg + 1]; }
    const double mx = a0.x, my = a0.y, mz = a0.z, dx = a1.x, dy = a1.y, dz = a1.z;
    const int len = a0.w, first = a1.w;
    const long jb = (long)row * span, je = min((long)N, jb + span);
    for (int a = 0; a < ntypes; ++a) {
        double re[R], im[R];
#pragma unroll
        for (int t = 0; t < R; ++t) re[t] = im[t] = 0.0;
        for (long base = jb; base < je; base += SF_CHUNK) {
            const int cnt = (int)min((long)SF_CHUNK, je - base);
            __syncthreads();   // the walk of the chunk before is over
            for (int q = lane; q < cnt; q += SF_TILE) {
                const unsigned idx = group ? group[base + q] : (unsigned)(base + q);
                const double4 p = pos[idx];
                sx[q] = fma(-box.xy, p.y, p.x) / box.Lx;
                sy[q] = p.y / box.Ly;
                sz[q] = p.z / box.Lz;
                st[q] = idx < ntyped ? types[idx] : (unsigned char)0;
            }
            __syncthreads();
            for (int q = 0; q < cnt; ++q) {
                if (__builtin_amdgcn_readfirstlane((int)st[q]) != a) continue;   // (wave-uniform: a scalar branch)
                const double x = sx[q], y = sy[q], z = sz[q];
                double cr, ci, wr, wi;
                sf_phase(mx, my, mz, x, y, z, cr, ci);
                sf_phase(dx, dy, dz, x, y, z, wr, wi);
#pragma unroll
                for (int t = 0; t < R; ++t) {
                    re[t] += cr; im[t] += ci;
                    const double nr = cr * wr - ci * wi;
                    ci = cr * wi + ci * wr;
                    cr = nr;
                }
            }
        }
        double2 *__restrict__ out = rows + ((size_t)row * ntypes + a) * nu + first;
#pragma unroll
        for (int t = 0; t < R; ++t)
            if (t < len) out[t] = make_double2(re[t], im[t]);
    }
}
__global__ void __launch_bounds__(SF_TILE * SF_FIN_WAVES)
k_sf_finish(const double2 *__restrict__ rows, int nrows, int ntypes, int nu, int nk, const unsigned *__restrict__ perm,
            const unsigned *__restrict__ uoff, double *__restrict__ rho, double *__restrict__ sums) {
    __shared__ double2 sh[SF_FIN_WAVES][SF_TILE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = blockIdx.x * SF_TILE + lane;
    const bool live = q < nu;
    double rr[PAIR_TYPED_MAX_TYPES], ri[PAIR_TYPED_MAX_TYPES];
#pragma unroll
    for (int a = 0; a < PAIR_TYPED_MAX_TYPES; ++a) {
        rr[a] = ri[a] = 0.0;
        if (a < ntypes) {   // (uniform: no lane leaves before a barrier)
            double2 s0 = make_double2(0.0, 0.0), s1 = s0, s2 = s0, s3 = s0;
            if (live) {
                const double2 *__restrict__ col = rows + (size_t)a * nu + q;
                const size_t stride = (size_t)ntypes * nu;
                int r = w;
                for (; r + 3 * SF_FIN_WAVES < nrows; r += 4 * SF_FIN_WAVES) {
                    const double2 v0 = col[(size_t)r * stride], v1 = col[(size_t)(r + SF_FIN_WAVES) * stride],
                                  v2 = col[(size_t)(r + 2 * SF_FIN_WAVES) * stride], v3 = col[(size_t)(r + 3 * SF_FIN_WAVES) * stride];
                    s0.x += v0.x; s0.y += v0.y; s1.x += v1.x; s1.y += v1.y; s2.x += v2.x; s2.y += v2.y; s3.x += v3.x; s3.y += v3.y;
                }
                for (; r < nrows; r += SF_FIN_WAVES) { const double2 v = col[(size_t)r * stride]; s0.x += v.x; s0.y += v.y; }
            }
            sh[w][lane] = make_double2((s0.x + s1.x) + (s2.x + s3.x), (s0.y + s1.y) + (s2.y + s3.y));
            __syncthreads();
            if (w == 0) {
                double x = 0.0, y = 0.0;
#pragma unroll
                for (int v = 0; v < SF_FIN_WAVES; ++v) { x += sh[v][lane].x; y += sh[v][lane].y; }
                rr[a] = x; ri[a] = y;
            }
            __syncthreads();
        }
    }
    if (w != 0 || !live) return;   // (behind the last barrier)
    for (unsigned e = uoff[q]; e < uoff[q + 1]; ++e) {   // (one place, or every place of a mode that is listed more than once)
        const unsigned o = perm[e];
        int p = 0;
#pragma unroll
        for (int a = 0; a < PAIR_TYPED_MAX_TYPES; ++a) {
            if (a >= ntypes) break;
            if (rho) { rho[2 * ((size_t)a * nk + o)] = rr[a]; rho[2 * ((size_t)a * nk + o) + 1] = ri[a]; }
#pragma unroll
            for (int b = a; b < PAIR_TYPED_MAX_TYPES; ++b) {
                if (b >= ntypes) break;
                if (sums) sums[(size_t)p * nk + o] += rr[a] * rr[b] + ri[a] * ri[b];
                ++p;
            }
        }
    }
}
int sf_span(unsigned n_max, int ntypes, int nk) {
    const long chunks = nblocks((long)n_max, SF_CHUNK);
    const long per = ((long)1 << 24) / ((long)ntypes * nk);   // rows that fit 2^24 complex numbers = 256 MB (>= 64: ntypes nk <= 2^18)
    return (int)(SF_CHUNK * ((chunks + per - 1) / per));
}
size_t sf_workspace(unsigned n_max, int ntypes, int nk) {
    return (size_t)nblocks((long)n_max, sf_span(n_max, ntypes, nk)) * ntypes * nk;
}
void launch_structure_factor(const double4 *pos, const unsigned *group, int N, DBox box, const StructureFactor &sf, double *rho, double *sums,
                             hipStream_t s) {
    static_assert(SF_TILE == 64, "a workgroup of k_sf_partial is one wave");
    const int nrows = nblocks(N, sf.span), nshort = sf.nseg - sf.nlong;
    if (sf.nlong) {
        const int ntiles = nblocks(sf.nlong, SF_TILE);
        hipLaunchKernelGGL(k_sf_partial<SF_RUN>, dim3((unsigned)(nrows * ntiles)), dim3(SF_TILE), 0, s, pos, group, N, sf.types, sf.n, sf.ntypes,
                           box, sf.segs, sf.nlong, ntiles, sf.span, sf.nu, sf.rows);
    }
    if (nshort) {
        const int ntiles = nblocks(nshort, SF_TILE);
        hipLaunchKernelGGL(k_sf_partial<SF_SHORT>, dim3((unsigned)(nrows * ntiles)), dim3(SF_TILE), 0, s, pos, group, N, sf.types, sf.n,
                           sf.ntypes, box, sf.segs + 2 * sf.nlong, nshort, ntiles, sf.span, sf.nu, sf.rows);
    }
    hipLaunchKernelGGL(k_sf_finish, dim3(nblocks(sf.nu, SF_TILE)), dim3(SF_TILE * SF_FIN_WAVES), 0, s, sf.rows, nrows, sf.ntypes, sf.nu,
                       sf.nk, sf.perm, sf.uoff, rho, sums);
}

// Displacement moments (pse_msd_store, pse_msd_accumulate, pse_msd_displacement): the unwrapped position of a particle is
// r_u = (fma(iy, sLy, fma(ix, Lx, x)), fma(iy, Ly, y), fma(iz, Lz, z)), sLy = strain Ly from the host: two roundings in x_u, one in y_u
// and z_u.  An object keeps slots of r_u as three planes of n_max doubles, indexed by the caller-order particle index.
// k_msd_store: one lane per group member; OUT = false writes r_u into the planes of a slot, OUT = true reads them and writes
// (d, |d|^2) to the caller's row.
// k_msd_partial: a WAVE owns MSD_SPAN = 256 consecutive group members, four per lane (member = base + 64 p + lane: every load of a
// plane is 8 bytes per lane and, with an identity group, 512 contiguous bytes per wave); the waves of a workgroup share nothing: no
// LDS, no barrier.  A lane reads pos, image and type of its four particles ONCE, forms r_u once and walks the listed slots: twelve
// 8-byte loads, the four displacements, and per type PRESENT in the wave (one ballot per type, before the loop) the ten moments of
// the lane's particles of that type, added in the order p = 0..3 -- ten doubles, never a table of types x moments.  The wave then
// adds them up with msd_wave_rows: a halving tree instead of ten butterflies -- at the level of lane bit b a lane keeps half of
// its values, sends the other half to the lane across that bit and adds what it receives, 10 -> 5 -> 3 -> 2 -> 1 values over bits
// 0..3 (11 exchanges), then two butterfly levels over bits 4 and 5: 13 exchanges of a double where ten butterflies take 60 (the
// exchanges go through the LDS crossbar, which the first form of this kernel -- one particle per lane, ten butterflies, the four waves
// added through LDS behind a barrier per slot -- was bound by: 1.48 ms for 64 origins at N = 10^6, docs/HISTORY.md).  Lane l < 16 ends
// with the wave's sum of moment 5 b0 + 3 b1 + 2 b2 + b3 (b_i the bits of l; the ten lanes for which that is a moment) and writes it to
// row (wave, pair, type) of the workspace; a type that is absent from the wave gets zeros.  Every row is written whole: the finish
// reads no stale word.  A member past N carries the type 255, which no ballot matches, and reads nothing.
// k_msd_finish: one workgroup of MSD_FIN threads per listed pair; a thread owns one of the ntypes x 10 columns and one of the
// MSD_FIN / columns strips; a strip adds the rows b = strip, strip + nstrip, ... in ascending order, four in flight, the strips
// are added in strip order through LDS, and the first strip adds the total to the caller's sums.  No floating-point atomics: every sum
// has a fixed order, equal inputs give equal bits.  Two pairs never name the same row of sums (the validator refuses that), so the
// workgroups of the finish write disjoint rows.
// The pass is a stream over N (45 + 24 npairs) bytes.  Measured: docs/HISTORY.md.
constexpr int MSD_PER_LANE = 4;                 // particles of one lane of k_msd_partial
constexpr int MSD_SPAN = 64 * MSD_PER_LANE;     // particles of one wave: one row of the workspace per (wave, pair, type)
constexpr int MSD_FIN = 1024;   // threads of a workgroup of k_msd_finish
__device__ __forceinline__ void msd_unwrap(const double4 p, const int3 im, double Lx, double Ly, double Lz, double sLy, double &xu, double &yu,
                                           double &zu) {
    xu = fma((double)im.y, sLy, fma((double)im.x, Lx, p.x));
    yu = fma((double)im.y, Ly, p.y);
    zu = fma((double)im.z, Lz, p.z);
}
template <bool OUT>
__global__ void __launch_bounds__(TPB)
k_msd_store(const double4 *__restrict__ pos, const int3 *__restrict__ image, const unsigned *__restrict__ group, int N, double Lx, double Ly,
            double Lz, double sLy, double *__restrict__ px, double *__restrict__ py, double *__restrict__ pz, size_t n_max,
            double4 *__restrict__ out) {
    const long i = (long)blockIdx.x * TPB + threadIdx.x;
    if (i >= N) return;
    const unsigned idx = group ? group[i] : (unsigned)i;
    if (idx >= n_max) return;
    double xu, yu, zu;
    msd_unwrap(pos[idx], image[idx], Lx, Ly, Lz, sLy, xu, yu, zu);
    if (OUT) {
        const double dx = xu - px[idx], dy = yu - py[idx], dz = zu - pz[idx];
        out[idx] = make_double4(dx, dy, dz, (dx * dx + dy * dy) + dz * dz);
    } else {
        px[idx] = xu; py[idx] = yu; pz[idx] = zu;
    }
}
// One level of the halving tree: of v[0 .. N) the lane keeps the lower half if `up` is false, the upper half (padded with +0.0) if it
// is true, sends the other half across `mask` and adds what the lane there sends: v[0 .. (N + 1)/2) on return.
template <int N>
__device__ __forceinline__ void msd_halve(double (&v)[MSD_MOMENTS], bool up, int mask) {
    constexpr int H = (N + 1) / 2;
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const double lo = v[j], hi = j + H < N ? v[j + H] : 0.0;
        v[j] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, mask, 64);
    }
}
// The sums over the wave of the ten values of every lane: on return lane l < 16 holds in v[0] the sum of value msd_lane_moment(l), if
// that is below MSD_MOMENTS (ten of the sixteen lanes).  Fixed order: equal inputs give equal bits.
__device__ __forceinline__ void msd_wave_rows(double (&v)[MSD_MOMENTS], int lane) {
    static_assert(MSD_MOMENTS == 10, "the tree halves 10 -> 5 -> 3 -> 2 -> 1");
    msd_halve<10>(v, lane & 1, 1);
    msd_halve<5>(v, lane & 2, 2);
    msd_halve<3>(v, lane & 4, 4);
    msd_halve<2>(v, lane & 8, 8);
    v[0] += __shfl_xor(v[0], 16, 64);
    v[0] += __shfl_xor(v[0], 32, 64);
}
__device__ __forceinline__ int msd_lane_moment(int lane) {   // (>= MSD_MOMENTS: the lane holds a sum of padding)
    const int b0 = lane & 1, b1 = (lane >> 1) & 1, b2 = (lane >> 2) & 1, b3 = (lane >> 3) & 1;
    const int low = 2 * b2 + b3;   // position among the (at most) three values kept at bit 1
    return low < (b1 ? 2 : 3) ? 5 * b0 + 3 * b1 + low : MSD_MOMENTS;
}
__global__ void __launch_bounds__(TPB)
k_msd_partial(const double4 *__restrict__ pos, const int3 *__restrict__ image, const unsigned *__restrict__ group, int N,
              const unsigned char *__restrict__ types, unsigned ntyped, int ntypes, double Lx, double Ly, double Lz, double sLy,
              const double *__restrict__ planes, size_t n_max, MsdPairs pairs, double *__restrict__ part /* [waves][npairs][ntypes][10] */) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (wave * MSD_SPAN >= N) return;   // (wave-uniform; the waves share nothing)
    unsigned idx[MSD_PER_LANE];
    int ty[MSD_PER_LANE];
    double xu[MSD_PER_LANE], yu[MSD_PER_LANE], zu[MSD_PER_LANE];
#pragma unroll
    for (int p = 0; p < MSD_PER_LANE; ++p) {
        const long i = wave * MSD_SPAN + p * 64 + lane;
        idx[p] = 0u; ty[p] = 255; xu[p] = yu[p] = zu[p] = 0.0;
        if (i < N) {
            idx[p] = group ? group[i] : (unsigned)i;
            if (idx[p] < n_max) {
                ty[p] = idx[p] < ntyped ? (int)types[idx[p]] : 0;
                msd_unwrap(pos[idx[p]], image[idx[p]], Lx, Ly, Lz, sLy, xu[p], yu[p], zu[p]);
            }
        }
    }
    unsigned present = 0u;   // (wave-uniform)
    for (int a = 0; a < ntypes; ++a) {
        bool mine = false;
#pragma unroll
        for (int p = 0; p < MSD_PER_LANE; ++p) mine |= ty[p] == a;
        if (__ballot(mine) != 0ull) present |= 1u << a;
    }
    const int c = msd_lane_moment(lane);
    const bool writer = lane < 16 && c < MSD_MOMENTS;
    for (int q = 0; q < pairs.npairs; ++q) {
        const double *__restrict__ px = planes + (size_t)pairs.slot[q] * 3 * n_max;
        double dx[MSD_PER_LANE], dy[MSD_PER_LANE], dz[MSD_PER_LANE];
#pragma unroll
        for (int p = 0; p < MSD_PER_LANE; ++p) {
            dx[p] = dy[p] = dz[p] = 0.0;
            if (ty[p] != 255) { dx[p] = xu[p] - px[idx[p]]; dy[p] = yu[p] - px[n_max + idx[p]]; dz[p] = zu[p] - px[2 * n_max + idx[p]]; }
        }
        double *__restrict__ row = part + ((size_t)wave * pairs.npairs + q) * ntypes * MSD_MOMENTS;
        for (int a = 0; a < ntypes; ++a, row += MSD_MOMENTS) {
            if (!(present & (1u << a))) {   // (wave-uniform: a scalar branch)
                if (lane < MSD_MOMENTS) row[lane] = 0.0;
                continue;
            }
            double v[MSD_MOMENTS];
#pragma unroll
            for (int k = 0; k < MSD_MOMENTS; ++k) v[k] = 0.0;
#pragma unroll
            for (int p = 0; p < MSD_PER_LANE; ++p) {
                if (ty[p] != a) continue;
                const double xx = dx[p] * dx[p], yy = dy[p] * dy[p], zz = dz[p] * dz[p];
                const double r2 = (xx + yy) + zz;
                v[0] += dx[p]; v[1] += dy[p]; v[2] += dz[p];
                v[3] += xx; v[4] += yy; v[5] += zz;
                v[6] += dx[p] * dy[p]; v[7] += dx[p] * dz[p]; v[8] += dy[p] * dz[p];
                v[9] += r2 * r2;
            }
            msd_wave_rows(v, lane);
            if (writer) row[c] = v[0];
        }
    }
}
__global__ void __launch_bounds__(MSD_FIN)
k_msd_finish(const double *__restrict__ part, int nblk, int ntypes, MsdPairs pairs, double *__restrict__ sums) {
    __shared__ double sh[MSD_FIN];
    const int ncol = ntypes * MSD_MOMENTS, nstrip = MSD_FIN / ncol;
    const int q = blockIdx.x, strip = threadIdx.x / ncol, col = threadIdx.x - strip * ncol;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (strip < nstrip) {
        const size_t stride = (size_t)pairs.npairs * ncol;
        const double *__restrict__ p = part + (size_t)q * ncol + col;
        int b = strip;
        for (; b + 3 * nstrip < nblk; b += 4 * nstrip) {
            const double v0 = p[(size_t)b * stride], v1 = p[(size_t)(b + nstrip) * stride], v2 = p[(size_t)(b + 2 * nstrip) * stride],
                         v3 = p[(size_t)(b + 3 * nstrip) * stride];
            s0 += v0; s1 += v1; s2 += v2; s3 += v3;
        }
        for (; b < nblk; b += nstrip) s0 += p[(size_t)b * stride];
    }
    sh[threadIdx.x] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (strip != 0) return;   // (behind the only barrier)
    double t = 0.0;
    for (int r = 0; r < nstrip; ++r) t += sh[r * ncol + col];
    sums[(size_t)pairs.row[q] * ncol + col] += t;
}
// (a call lists up to MSD_MAX_ORIGINS pairs whatever the number of slots -- a slot may be named for several rows -- and the rows of
// the workspace are per listed pair: sized for the most pairs, never for norigins)
size_t msd_workspace(unsigned n_max, int ntypes) {
    return (size_t)nblocks((long)n_max, MSD_SPAN) * MSD_MAX_ORIGINS * ntypes * MSD_MOMENTS;
}
void launch_msd_store(const double4 *pos, const int3 *image, const unsigned *group, int N, double Lx, double Ly, double Lz, double sLy,
                      const MsdOrigins &mo, int slot, double4 *out, hipStream_t s) {
    double *px = mo.planes + (size_t)slot * 3 * mo.n_max, *py = px + mo.n_max, *pz = py + mo.n_max;
    if (out)
        hipLaunchKernelGGL(k_msd_store<true>, dim3(nblocks(N, TPB)), dim3(TPB), 0, s, pos, image, group, N, Lx, Ly, Lz, sLy, px, py, pz, mo.n_max, out);
    else
        hipLaunchKernelGGL(k_msd_store<false>, dim3(nblocks(N, TPB)), dim3(TPB), 0, s, pos, image, group, N, Lx, Ly, Lz, sLy, px, py, pz, mo.n_max, out);
}
void launch_msd_accumulate(const double4 *pos, const int3 *image, const unsigned *group, int N, double Lx, double Ly, double Lz, double sLy,
                           const MsdOrigins &mo, const MsdPairs &pairs, double *sums, hipStream_t s) {
    static_assert(MSD_FIN >= PAIR_TYPED_MAX_TYPES * MSD_MOMENTS, "a workgroup of k_msd_finish holds at least one strip");
    const int nblk = nblocks(N, MSD_SPAN);   // rows of the workspace per (pair, type): one per wave; npairs <= MSD_MAX_ORIGINS, N <= n_max (validated)
    hipLaunchKernelGGL(k_msd_partial, dim3(nblocks(nblk, TPB / 64)), dim3(TPB), 0, s, pos, image, group, N, mo.types, mo.n, mo.ntypes, Lx, Ly, Lz, sLy, mo.planes,
                       mo.n_max, pairs, mo.part);
    hipLaunchKernelGGL(k_msd_finish, dim3(pairs.npairs), dim3(MSD_FIN), 0, s, mo.part, nblk, mo.ntypes, pairs, sums);
}

}  // namespace pse
