// Kernels of the cluster analysis with percolation (pse_percolation.h; pse_clusters_span): the lock-free union-find of
// pse_analysis.hip with an integer image offset beside every parent pointer -- which clusters are connected to their own periodic
// image and along which lattice axes, every other cluster made whole across the boundaries, and its radius of gyration.  A family of
// its own beside the five launches of pse_clusters_label, which it leaves as they are.  gfx950, wave64, fp64 and integers.
//
// The word of row x (pse_cluster_word.h) holds parent[x] <= x and o_x = c_x - c_parent, c an unfolding of x's tree: an integer vector
// per row with c_j = c_i + n_ij on every link (i, j) that hooked, n_ij the shift that min_image takes from r_i - r_j.  Every load,
// store and compare-and-swap of a word is ONE 8-byte relaxed agent-scope atomic: parent and offset are never seen torn.
// Everything the comment above cluster_find (pse_analysis.hip) says about the parents holds word for word.  For the offsets:
//   * a hook joins two DIFFERENT trees (the CAS succeeds only on a root), so it fixes the one free constant between their
//     unfoldings and changes no difference c_x - c_y inside either: the relative offsets inside a tree are fixed once and for all;
//   * every word ever written states such a difference between two rows of one tree: the hook writes (lo, c_hi - c_lo) from the two
//     sums it carried, path halving writes (grandparent, o_x + o_parent) from two words it loaded.  A stale word is still a true one,
//     whichever of two racing stores lands last;
//   * find(x) therefore returns the root r it reached and c_x - c_r, however the tree changed meanwhile.
// unite(i, j, n): roots A, B with a = c_i - c_A, b = c_j - c_B.  A != B: the larger root goes under the smaller with one CAS on
// (hi, 0, 0, 0); for hi = A the word is (B, b - n - a), for hi = B it is (A, a + n - b).  Where the CAS fails, the lane continues
// from the word it returned -- hi's parent and hi's offset to it, folded into the sum of that side.  A == B: the link closes a cycle
// of winding m = b - a - n; every axis k with m_k != 0 is ORed into flag[A].  Each link ends as a hook or a check; the checked links
// are the fundamental cycles of the final spanning forest, whose windings generate those of every closed walk: the OR of their
// non-zero components is the set of spanned axes, whatever the order of the hooks.
// Caps (status bits of pse_cluster_word.h, sticky, the call then writes ~0u labels): an offset component beyond +-2047 where a word
// is packed, a |q| >= 2^31 in the geometry, N > 2^28.  None is reachable at any size that is tested or run.
#include "pse_percolation.h"
#include "pse_excl.h"

namespace pse {

struct SpanAt {
    unsigned row;      // ~0u: gave up
    int cx, cy, cz;    // c_start - c_row
};
__device__ __forceinline__ unsigned long long span_word(const unsigned long long *word, unsigned x) {
    return __hip_atomic_load(word + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The root of x's tree and c_x - c_root.  HALVE: a row that is not a root is pointed at its grandparent with the sum of the two offsets.
template <bool HALVE>
__device__ __forceinline__ SpanAt span_find(unsigned long long *word, unsigned x, unsigned cap, unsigned *status) {
    int sx = 0, sy = 0, sz = 0;
    for (unsigned trip = 0; trip < cap; ++trip) {
        unsigned p;
        int ox, oy, oz;
        cluster_word_unpack(span_word(word, x), p, ox, oy, oz);
        if (p == x) return SpanAt{x, sx, sy, sz};
        if (HALVE) {
            unsigned gp;
            int px, py, pz;
            cluster_word_unpack(span_word(word, p), gp, px, py, pz);   // (a root p: gp = p and zeros)
            ox += px; oy += py; oz += pz;
            if (gp != p) {
                if (cluster_offset_fits(ox, oy, oz))
                    __hip_atomic_store(word + x, cluster_word_pack(gp, ox, oy, oz), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else
                    atomicOr(status, CLUSTER_CAP_OFFSET);
            }
            x = gp;
        } else {
            x = p;
        }
        sx += ox; sy += oy; sz += oz;
    }
    atomicOr(status, CLUSTER_CAP_FIND_BIT);
    return SpanAt{~0u, 0, 0, 0};
}
__device__ __forceinline__ void span_unite(unsigned long long *word, unsigned *flag, unsigned i, unsigned j, int n1, int n2, int n3, unsigned cap,
                                           unsigned *status) {
    unsigned x = i, y = j;
    int ax = 0, ay = 0, az = 0, bx = 0, by = 0, bz = 0;   // c_i - c_x, c_j - c_y
    for (unsigned trip = 0; trip < cap; ++trip) {
        const SpanAt A = span_find<true>(word, x, cap, status);
        if (A.row == ~0u) return;
        x = A.row; ax += A.cx; ay += A.cy; az += A.cz;
        const SpanAt B = span_find<true>(word, y, cap, status);
        if (B.row == ~0u) return;
        y = B.row; bx += B.cx; by += B.cy; bz += B.cz;
        if (x == y) {
            const unsigned bits = (bx - ax - n1 != 0 ? 1u : 0u) | (by - ay - n2 != 0 ? 2u : 0u) | (bz - az - n3 != 0 ? 4u : 0u);
            // (bits are only ever set: a lane that sees them set already has nothing to add.  In one spanning cluster of 10^6 rows most
            // of the 6 x 10^6 checked links wind, and without the load every one of them puts an atomic on the same word.)
            if (bits && (__hip_atomic_load(flag + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bits) != bits) atomicOr(flag + x, bits);
            return;
        }
        const bool x_hi = x > y;
        const unsigned hi = x_hi ? x : y, lo = x_hi ? y : x;
        const int hx = x_hi ? bx - n1 - ax : ax + n1 - bx, hy = x_hi ? by - n2 - ay : ay + n2 - by, hz = x_hi ? bz - n3 - az : az + n3 - bz;
        if (!cluster_offset_fits(hx, hy, hz)) { atomicOr(status, CLUSTER_CAP_OFFSET); return; }
        const unsigned long long seen = atomicCAS(word + hi, (unsigned long long)hi, cluster_word_pack(lo, hx, hy, hz));
        if (seen == (unsigned long long)hi) return;
        unsigned p;   // hi was hooked by another lane, under p < hi at the offset the word states
        int ox, oy, oz;
        cluster_word_unpack(seen, p, ox, oy, oz);
        if (x_hi) { x = p; ax += ox; ay += oy; az += oz; }
        else { y = p; bx += ox; by += oy; bz += oz; }
    }
    atomicOr(status, CLUSTER_CAP_UNITE_BIT);
}
// min_image (pse_device.h) with the integers it takes: d -= n1 a1 + n2 a2 + n3 a3, the same arithmetic in the same order.
__device__ __forceinline__ void min_image_shift(const DBox &b, double &dx, double &dy, double &dz, int &n1, int &n2, int &n3) {
    const double ny = rint(dy * b.iLy);
    dy -= ny * b.Ly;
    dx -= ny * b.xy * b.Ly;
    const double nx = rint(dx * b.iLx);
    dx -= nx * b.Lx;
    const double nz = rint(dz * b.iLz);
    dz -= nz * b.Lz;
    n1 = (int)nx; n2 = (int)ny; n3 = (int)nz;
}
__global__ void __launch_bounds__(TPB)
k_span_init(int N, unsigned long long *__restrict__ word, unsigned long long *__restrict__ minkey, unsigned long long *__restrict__ sums,
            unsigned *__restrict__ flag, unsigned *__restrict__ csize, unsigned *status, unsigned long long *__restrict__ stats,
            unsigned long long *__restrict__ pstats) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < N) {
        word[i] = (unsigned long long)i; minkey[i] = ~0ull; flag[i] = 0u; csize[i] = 0u;
#pragma unroll
        for (int k = 0; k < 5; ++k) sums[5 * (size_t)i + k] = 0ull;
    }
    if (stats && i < 4) stats[i] = 0ull;
    if (pstats && i < 8) pstats[i] = 0ull;
    if (i == 0 && (unsigned)N > CLUSTER_WORD_MAX_ROWS) atomicOr(status, CLUSTER_CAP_ROWS);
}
// The walk of k_cluster_link with the shift of every linked pair.  No lane leaves before the barrier.
template <bool EXCL>
__global__ void __launch_bounds__(TPB)
k_span_link(const double4 *__restrict__ pos_s, const unsigned *__restrict__ tag_s, const unsigned char *__restrict__ type_s, int N,
            const int *__restrict__ cell_off, DBox box, DCells nc, int ntypes, const double *__restrict__ rlink2 /* npt */, double rl2_all,
            unsigned long long *word, unsigned *flag, unsigned *status, ExclRows ex) {
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
                int n1, n2, n3;
                min_image_shift(box, dx, dy, dz, n1, n2, n3);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (r2 < rl2_all && r2 > 0.0) {
                    const int tj = type_s[j];
                    const int lo = min(ti, tj), hi = max(ti, tj);
                    const int p = lo * ntypes - ((lo * (lo - 1)) >> 1) + (hi - lo);
                    if (r2 < rl2[p] && !(EXCL && eb < ee && excl_has(ex.ent, eb, ee, tag_s[j])))
                        span_unite(word, flag, (unsigned)i, (unsigned)j, n1, n2, n3, (unsigned)N, status);
                }
            }
        });
    }
}
// Every row stores (root, c_row - c_root); the root collects the number of members, the smallest (caller index, row) key and the
// flags found at rows that have since been hooked.  The wave-aggregated atomics of k_cluster_flatten: the lanes whose root is that of
// the wave's first lane reduce among themselves and ONE adds for all.  No lane leaves before the butterfly.
__global__ void __launch_bounds__(TPB)
k_span_flatten(const unsigned *__restrict__ tag_s, int N, unsigned long long *word, unsigned long long *__restrict__ minkey,
               unsigned *__restrict__ csize, unsigned *flag, unsigned *status) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    unsigned root = ~0u, mine = 0u;
    unsigned long long key = ~0ull;
    if (i < N) {
        const SpanAt at = span_find<false>(word, (unsigned)i, (unsigned)N, status);
        if (at.row != ~0u) {
            if (cluster_offset_fits(at.cx, at.cy, at.cz)) {
                root = at.row;
                __hip_atomic_store(word + i, cluster_word_pack(root, at.cx, at.cy, at.cz), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                key = ((unsigned long long)tag_s[i] << 32) | (unsigned)i;
                mine = root != (unsigned)i ? __hip_atomic_load(flag + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            } else {
                atomicOr(status, CLUSTER_CAP_OFFSET);
            }
        }
    }
    const unsigned lead = __shfl(root, 0, 64);
    const bool with_lead = root != ~0u && root == lead;
    const unsigned long long group = __ballot(with_lead);
    unsigned long long least = with_lead ? key : ~0ull;
    unsigned bits = with_lead ? mine : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(least, o, 64);
        least = other < least ? other : least;
        bits |= (unsigned)__shfl_xor((int)bits, o, 64);
    }
    if (with_lead) {
        if ((threadIdx.x & 63) == (unsigned)(__ffsll((long long)group) - 1)) {
            atomicMin(minkey + root, least);
            atomicAdd(csize + root, (unsigned)__popcll(group));
            if (bits) atomicOr(flag + root, bits);
        }
    } else if (root != ~0u) {
        atomicMin(minkey + root, key);
        atomicAdd(csize + root, 1u);
        if (mine) atomicOr(flag + root, mine);
    }
}
// What a row of a cluster that spans nothing needs of its label member (row0, the sorted row of the smallest caller index): the
// image dc = c_i - c_0 stated for the CALLER's positions -- the sorted rows are wrapped copies, r_s = r - w (a1, a2, a3), and an
// unfolding of the sorted rows c_s gives c = c_s - w for the caller's -- and, for the geometry,
//   D = (r_i - r_0) + dc (a1, a2, a3):  Dx = ((x_i - x_0) + dc1 Lx) + dc2 (xy Ly),  Dy = (y_i - y_0) + dc2 Ly,  Dz = (z_i - z_0) + dc3 Lz.
__device__ __forceinline__ void span_wrap(const DBox &box, const double4 &p, const double4 &ps, int &w1, int &w2, int &w3) {
    double dx = p.x - ps.x, dy = p.y - ps.y, dz = p.z - ps.z;
    min_image_shift(box, dx, dy, dz, w1, w2, w3);
}
__device__ __forceinline__ void span_image(const double4 *__restrict__ pos, const double4 *__restrict__ pos_s, const unsigned *__restrict__ tag_s,
                                           const DBox &box, const unsigned long long *__restrict__ word, unsigned i, unsigned row0, const double4 &pi,
                                           double4 &p0, int &d1, int &d2, int &d3) {
    unsigned r;
    int ix, iy, iz, zx, zy, zz, w1, w2, w3, v1, v2, v3;
    cluster_word_unpack(word[i], r, ix, iy, iz);
    cluster_word_unpack(word[row0], r, zx, zy, zz);
    p0 = pos[tag_s[row0]];
    span_wrap(box, pi, pos_s[i], w1, w2, w3);
    span_wrap(box, p0, pos_s[row0], v1, v2, v3);
    d1 = (ix - w1) - (zx - v1); d2 = (iy - w2) - (zy - v2); d3 = (iz - w3) - (zz - v3);
}
// Geometry of the clusters that span nothing: every member adds q = llrint(D 2^20) and q^2, split at bit 32, to the five integer
// words of its root.  The lanes that share the root of the wave's first contributing lane reduce among themselves and add once; a
// cluster of 10^5 rows puts a few thousand atomics on its words, not 10^5.  Integers: the order does not matter.  No lane leaves
// before the butterfly.
__global__ void __launch_bounds__(TPB)
k_span_geometry(const double4 *__restrict__ pos, const double4 *__restrict__ pos_s, const unsigned *__restrict__ tag_s, int N, DBox box,
                const unsigned long long *__restrict__ word, const unsigned long long *__restrict__ minkey, const unsigned *__restrict__ flag,
                unsigned long long *__restrict__ sums, unsigned *status) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    unsigned root = ~0u;
    bool on = false;
    unsigned long long v[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    if (i < N) {
        root = cluster_word_parent(word[i]);
        const unsigned row0 = (unsigned)minkey[root];   // (~0: the flatten gave up on this tree)
        if (flag[root] == 0u && row0 < (unsigned)N && row0 != (unsigned)i) {
            const double4 pi = pos[tag_s[i]];
            double4 p0;
            int d1, d2, d3;
            span_image(pos, pos_s, tag_s, box, word, (unsigned)i, row0, pi, p0, d1, d2, d3);
            const double Dx = ((pi.x - p0.x) + (double)d1 * box.Lx) + (double)d2 * (box.xy * box.Ly);
            const double Dy = (pi.y - p0.y) + (double)d2 * box.Ly;
            const double Dz = (pi.z - p0.z) + (double)d3 * box.Lz;
            const long long q[3] = {llrint(Dx * CLUSTER_Q_SCALE), llrint(Dy * CLUSTER_Q_SCALE), llrint(Dz * CLUSTER_Q_SCALE)};
            bool fits = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) fits = fits && q[k] > -CLUSTER_Q_LIMIT && q[k] < CLUSTER_Q_LIMIT;   // (a NaN converts to a value outside)
            if (fits) {
                on = true;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const unsigned long long sq = (unsigned long long)(q[k] * q[k]);
                    v[k] = (unsigned long long)q[k];
                    v[3] += sq & 0xffffffffull;
                    v[4] += sq >> 32;
                }
            } else {
                atomicOr(status, CLUSTER_CAP_Q);
            }
        }
    }
    const unsigned long long contributing = __ballot(on);
    const int first = contributing ? __ffsll((long long)contributing) - 1 : 0;
    const unsigned lead = __shfl(root, first, 64);
    const bool with_lead = on && root == lead;
    const unsigned long long group = __ballot(with_lead);
    unsigned long long t[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) t[k] = with_lead ? v[k] : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 5; ++k) t[k] += __shfl_xor(t[k], o, 64);
    }
    if (with_lead) {
        if ((threadIdx.x & 63) == (unsigned)(__ffsll((long long)group) - 1)) {
#pragma unroll
            for (int k = 0; k < 5; ++k) if (t[k]) atomicAdd(sums + 5 * (size_t)root + k, t[k]);
        }
    } else if (on) {
#pragma unroll
        for (int k = 0; k < 5; ++k) if (v[k]) atomicAdd(sums + 5 * (size_t)root + k, v[k]);
    }
}
// Everything by caller index.  label, size, stats and hist: k_cluster_write, line for line.  span: the root's flags; image: dc of
// span_image, zeros in a spanning cluster; rg2: cluster_rg2 of the root's sums, -1 in a spanning cluster; pstats: eight words summed in
// LDS behind the same barrier.  A non-zero status word: ~0u labels, zero sizes, flags and images, rg2 = -1, stats and pstats at zero.
constexpr int SPAN_LDS_BINS = 64;
__global__ void __launch_bounds__(TPB)
k_span_write(const double4 *__restrict__ pos, const double4 *__restrict__ pos_s, const unsigned *__restrict__ tag_s, int N, DBox box,
             const unsigned long long *__restrict__ word, const unsigned long long *__restrict__ minkey, const unsigned *__restrict__ csize,
             const unsigned *__restrict__ flag, const unsigned long long *__restrict__ sums, const unsigned *__restrict__ status,
             unsigned *__restrict__ label, unsigned *__restrict__ size, unsigned long long *__restrict__ stats, unsigned long long *__restrict__ hist,
             unsigned nhist, unsigned *__restrict__ span, int *__restrict__ image, double *__restrict__ rg2, unsigned long long *__restrict__ pstats) {
    __shared__ unsigned long long st[4], ps[8];
    __shared__ unsigned hb[SPAN_LDS_BINS];
    if (threadIdx.x < 4) st[threadIdx.x] = 0ull;
    if (threadIdx.x < 8) ps[threadIdx.x] = 0ull;
    if (threadIdx.x < SPAN_LDS_BINS) hb[threadIdx.x] = 0u;
    __syncthreads();
    const bool gave_up = *status != 0u;
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < N) {
        const unsigned t = tag_s[i];
        if (gave_up) {
            if (label) label[t] = ~0u;
            if (size) size[t] = 0u;
            if (span) span[t] = 0u;
            if (image) { image[3 * (size_t)t] = 0; image[3 * (size_t)t + 1] = 0; image[3 * (size_t)t + 2] = 0; }
            if (rg2) rg2[t] = -1.0;
        } else {
            const unsigned root = cluster_word_parent(word[i]);
            const unsigned long long key = minkey[root];
            const unsigned row0 = (unsigned)key, f = flag[root], sz = csize[root];
            if (label) label[t] = (unsigned)(key >> 32);
            if (size) size[t] = sz;
            if (span) span[t] = f;
            if (image) {
                int d1 = 0, d2 = 0, d3 = 0;
                if (!f && row0 != (unsigned)i) {
                    double4 p0;
                    span_image(pos, pos_s, tag_s, box, word, (unsigned)i, row0, pos[t], p0, d1, d2, d3);
                }
                image[3 * (size_t)t] = d1; image[3 * (size_t)t + 1] = d2; image[3 * (size_t)t + 2] = d3;
            }
            if (rg2) {
                const unsigned long long *q = sums + 5 * (size_t)root;
                rg2[t] = f ? -1.0 : cluster_rg2((long long)q[0], (long long)q[1], (long long)q[2], q[3], q[4], sz);
            }
            if (root == (unsigned)i) {
                const unsigned long long s64 = sz;
                if (stats) {
                    atomicAdd(st + 0, 1ull);
                    atomicMax(st + 1, s64);
                    atomicAdd(st + 2, s64 * s64);
                    atomicAdd(st + 3, s64);
                }
                if (hist) {
                    const unsigned long long b = min(s64, (unsigned long long)nhist) - 1ull;
                    if (b < (unsigned long long)SPAN_LDS_BINS) atomicAdd(hb + (unsigned)b, 1u);
                    else atomicAdd(hist + b, 1ull);
                }
                if (pstats) {
                    if (f) {
                        atomicAdd(ps + 0, 1ull);
                        atomicAdd(ps + 1, s64);
                        if (f & 1u) atomicAdd(ps + 2, 1ull);
                        if (f & 2u) atomicAdd(ps + 3, 1ull);
                        if (f & 4u) atomicAdd(ps + 4, 1ull);
                        if (f == 7u) atomicAdd(ps + 5, 1ull);
                    } else {
                        atomicMax(ps + 6, s64);
                        atomicAdd(ps + 7, s64 * s64);
                    }
                }
            }
        }
    }
    __syncthreads();
    if (stats && threadIdx.x < 4 && st[threadIdx.x]) {
        if (threadIdx.x == 1) atomicMax(stats + 1, st[1]);
        else atomicAdd(stats + threadIdx.x, st[threadIdx.x]);
    }
    if (pstats && threadIdx.x < 8 && ps[threadIdx.x]) {
        if (threadIdx.x == 6) atomicMax(pstats + 6, ps[6]);
        else atomicAdd(pstats + threadIdx.x, ps[threadIdx.x]);
    }
    if (hist && threadIdx.x < SPAN_LDS_BINS && threadIdx.x < nhist && hb[threadIdx.x]) atomicAdd(hist + threadIdx.x, (unsigned long long)hb[threadIdx.x]);
}
void launch_clusters_span(const double4 *pos, const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc,
                          const ClusterLinks &cl, const ClusterSpan &sp, unsigned *label, unsigned *size, unsigned long long *stats,
                          unsigned long long *hist, unsigned nhist, unsigned *span, int *image, double *rg2, unsigned long long *pstats,
                          hipStream_t s, const PairExclusions *ex) {
    static_assert(PAIR_TYPED_MAX_PAIR_TYPES <= TPB, "one lane stages one link distance");
    const int nb = nblocks(N, TPB);
    const bool rows_fit = (unsigned)N <= CLUSTER_WORD_MAX_ROWS;   // beyond: k_span_init sets the bit, nothing walks, k_span_write writes ~0u
    launch_type_mirror(tag_s, N, cl.types, cl.n, cl.type_s, s);
    hipLaunchKernelGGL(k_span_init, dim3(nb), dim3(TPB), 0, s, N, sp.word, sp.minkey, sp.sums, sp.flag, cl.csize, cl.status, stats, pstats);
    if (rows_fit) {
        launch_with_excl(ex, [&](auto excl, ExclRows er) {
            hipLaunchKernelGGL((k_span_link<decltype(excl)::value>), dim3(nb), dim3(TPB), 0, s, pos_s, tag_s, cl.type_s, N, cell_off, box, nc,
                               cl.ntypes, cl.rlink2, cl.rl2_all, sp.word, sp.flag, cl.status, er);
        });
        hipLaunchKernelGGL(k_span_flatten, dim3(nb), dim3(TPB), 0, s, tag_s, N, sp.word, sp.minkey, cl.csize, sp.flag, cl.status);
        if (rg2)
            hipLaunchKernelGGL(k_span_geometry, dim3(nb), dim3(TPB), 0, s, pos, pos_s, tag_s, N, box, sp.word, sp.minkey, sp.flag, sp.sums,
                               cl.status);
    }
    hipLaunchKernelGGL(k_span_write, dim3(nb), dim3(TPB), 0, s, pos, pos_s, tag_s, N, box, sp.word, sp.minkey, cl.csize, sp.flag, sp.sums,
                       cl.status, label, size, stats, hist, nhist, span, image, rg2, pstats);
}

}  // namespace pse
