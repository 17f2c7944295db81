// HIP kernels of the PSE engine for gfx950 (CDNA4, wave64): the cell sort, the gates, the gather into cell order (k_permute*), the
// near field (K9) and k_eval_fg.  The far field is pse_farfield.hip, the transforms are pse_fft.hip and pse_zfft.hip, the Lanczos and
// the other vector kernels pse_vectors.hip.  Each kernel names the reference kernel it replaces.  All
// arithmetic is fp64.
#include "pse_kernels.h"
#include "pse_vectors.h"
#include "pse_farbin.h"

#include <hipcub/hipcub.hpp>

namespace pse {

// ------------------------------------------------------------------------------------------------ binning
// (replaces HOOMD CellListGPU used through NeighborListGPUBinned, PSEv1/integrate.py:58-83)
// Counting sort by cell (rocprim's sort_pairs runs ten merge passes at N = 1e6: 0.15 ms).  Arrival ranks from atomics are
// not reproducible, and every slab rank must end up with the SAME order (rows are exchanged by position), so a last
// pass orders each cell by original index: the result equals a stable sort by key.  cell_off[c] = first slot of cell c
// (c = 0..ncell): cell c owns [cell_off[c], cell_off[c+1]) and any run of consecutive cells is one contiguous slot range.
constexpr unsigned KEY_FOREIGN = 0xFFFFFFFFu;   // a particle a slab rank counts but does not order
// (Counting the foreign particles per x layer in an LDS histogram instead -- one global add per layer and workgroup, booked on
// the layer's first cell -- was slower: 58 us against 45 us; the kernel is not bound by its global atomics.)
__global__ void k_cell_keys(const double4 *__restrict__ pos, const unsigned *__restrict__ group, int N, DBox box,
                            DCells nc, unsigned *__restrict__ keys, unsigned *__restrict__ rank, int *__restrict__ cnt, CellRanges need,
                            SlabBook sb, Gate gate) {
    if (gate.closed()) return;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = g < N;
    unsigned key = 0;
    bool mine = false;
    if (live) {
        const unsigned idx = group ? group[g] : (unsigned)g;
        const double4 p = pos[idx];
        double fx, fy, fz;
        frac_coords(box, p.x, p.y, p.z, fx, fy, fz);
        const int cx = cell_coord(fx, nc.nx), cy = cell_coord(fy, nc.ny), cz = cell_coord(fz, nc.nz);
        const int zb = cz / nc.bz;
        key = (unsigned)cell_slot(nc, cx, cy, zb, cz - zb * nc.bz);
        mine = need.cell((int)key);
        if (mine) {
            keys[g] = key;
            rank[g] = (unsigned)atomicAdd(&cnt[key], 1);
        } else {
            keys[g] = KEY_FOREIGN;
            if (sb.n == 0) atomicAdd(&cnt[key], 1);   // counted (the row offsets are global), not ranked
        }
    }
    if (sb.n > 0) {
        // A slab rank needs the row offsets of its own and its ghost cells and of every slab boundary -- not of the cells in
        // between.  The particles of another rank's cells are therefore counted per SLAB, on the first cell of that slab the rank
        // does not keep (all of them lie before or after the kept layers of that slab, so every offset that is used comes out
        // right), one atomic per distinct slab of a wavefront: device-scope atomics run at ~20 G/s however they are addressed
        // (MI355X_MICROARCH.md), and 80 % of the particles are foreign to a rank of eight.
        const int slab = live && !mine ? (int)(key / (unsigned)sb.cells_per_slab) : -1;
        unsigned long long todo = __ballot(slab >= 0);
        const int lane = threadIdx.x & 63;
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            const int s0 = __shfl(slab, src, 64);
            const unsigned long long m = __ballot(slab == s0) & todo;
            // spread over `spread` cells of that layer by workgroup: one word takes ~88 atomics per microsecond, and a step has
            // 15 000 wavefronts x 7 foreign slabs (all on ONE cell per slab the kernel took 195 us instead of 45)
            if (lane == src) atomicAdd(&cnt[sb.book[s0] + (int)((blockIdx.x * 4u + (threadIdx.x >> 6)) % (unsigned)sb.spread)], __popcll(m));
            todo &= ~m;
        }
    }
}
__global__ void k_cell_scatter(const unsigned *__restrict__ keys, const unsigned *__restrict__ rank,
                               const int *__restrict__ cell_off, int N, unsigned *__restrict__ slots, Gate gate) {
    if (gate.closed()) return;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < N && keys[g] != KEY_FOREIGN) slots[cell_off[keys[g]] + rank[g]] = (unsigned)g;
}
// one thread per slot: rank its particle among the members of its cell (a handful: the loads of a cell's threads are the same
// few words), write it in order.  (One wave per cell kept five of 64 lanes busy: 33 us at N = 1e6; this way 10.)
__global__ void __launch_bounds__(TPB)
k_cell_order(const int *__restrict__ cell_off, const unsigned *__restrict__ keys, int N, const unsigned *__restrict__ slots,
             unsigned *__restrict__ perm, CellRanges need, Gate gate) {
    if (gate.closed()) return;
    const int s = blockIdx.x * TPB + threadIdx.x;
    if (s >= N || !need.row(s, cell_off)) return;
    const unsigned v = slots[s];
    const int c = (int)keys[v], a = cell_off[c], n = cell_off[c + 1] - a;
    int smaller = 0;
    for (int t = 0; t < n; ++t) smaller += slots[a + t] < v ? 1 : 0;
    perm[a + smaller] = v;
}
size_t cell_sort_temp_bytes(size_t ncell) {
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const int *)nullptr, (int *)nullptr, (int)(ncell + 1));
    return bytes;
}
hipError_t launch_cell_scan(const int *cnt, int *out, int n, void *tmp, size_t tmp_bytes, hipStream_t s) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cnt, out, n, s);
}
hipError_t cell_sort(const double4 *pos, const unsigned *group, int N, DBox box, DCells nc, unsigned *keys, unsigned *rank,
                     unsigned *slots, int *cnt, int ncell, void *tmp, size_t tmp_bytes, int *cell_off, unsigned *perm, hipStream_t s,
                     CellRanges need, SlabBook sb, bool cnt_is_zero, Gate gate) {
    hipError_t e = cnt_is_zero ? hipSuccess : hipMemsetAsync(cnt, 0, (size_t)(ncell + 1) * sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cell_keys, dim3(nblocks(N, TPB)), dim3(TPB), 0, s, pos, group, N, box, nc, keys, rank, cnt, need, sb, gate);
    // cnt[ncell] = 0: cell_off[ncell] = N.  A failed scan (scratch too small for ncell) would leave garbage offsets: reported
    e = hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cnt, cell_off, ncell + 1, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cell_scatter, dim3(nblocks(N, TPB)), dim3(TPB), 0, s, keys, rank, cell_off, N, slots, gate);
    hipLaunchKernelGGL(k_cell_order, dim3(nblocks(N, TPB)), dim3(TPB), 0, s, cell_off, keys, N, slots, perm, need, gate);
    return hipGetLastError();
}

// Gather into cell order: wrapped sorted positions (+ the float copy and the packed records of the near field), the vector, the tags
// -- and, since round 4, what used to be two more launches over the same rows: the rank of every particle inside its far-field bin
// (far.on; was k_support) and the particle noise of the step (psi_s; K14 gpu_stokes_BrownianGenerate_kernel, PSEv1/Brownian.cu:99-130).
__global__ void __launch_bounds__(TPB)
k_permute(const double4 *__restrict__ pos, const double4 *__restrict__ vec,
                          const unsigned *__restrict__ group, const unsigned *__restrict__ perm, int N, DBox box,
                          double4 *__restrict__ pos_s, float4 *__restrict__ posf_s, double2 *__restrict__ pv,
                          double4 *__restrict__ vec_s, unsigned *__restrict__ tag_s, const double4 *__restrict__ pos_build,
                          double half_skin2, int *__restrict__ flags, CellRanges need, const int *__restrict__ cell_off,
                          FarBinArgs far, double4 *__restrict__ psi_s, uint32_t seed, uint32_t timestep, Gate gate,
                          const uint32_t *__restrict__ ts_off) {
    if (gate.closed()) return;
    if (ts_off) timestep += *ts_off;
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s - (int)(threadIdx.x & 63) >= N) return;            // whole wave past the end
    const bool live = s < N && need.row(s, cell_off);        // a slab rank holds particle data for its own and its ghost rows only
    bool bin_need = false;
    int bin = -1;
    if (live) {
        const unsigned g = perm[s];
        const unsigned idx = group ? group[g] : g;
        const double4 p = pos[idx];
        // wrap into the primary cell (keeps sheared images consistent: y images shift x by xy*Ly)
        double fx, fy, fz;
        frac_coords(box, p.x, p.y, p.z, fx, fy, fz);
        const double y = (fy - 0.5) * box.Ly;
        double4 q;
        q.x = (fx - 0.5) * box.Lx + box.xy * y;
        q.y = y;
        q.z = (fz - 0.5) * box.Lz;
        q.w = 0.0;
        pos_s[s] = q;
        posf_s[s] = make_float4((float)q.x, (float)q.y, (float)q.z, 0.0f);   // single-precision copy for the cutoff pre-filter
        if (pv) {   // packed 48-byte (position, vector) records of the near-field passes' drain: the position half
            pv[3 * (size_t)s] = make_double2(q.x, q.y);
            ((double *)&pv[3 * (size_t)s + 1])[0] = q.z;
        }
        tag_s[s] = idx;
        if (vec) {
            double4 v = vec[idx];
            v.w = 0.0;
            vec_s[s] = v;
            if (pv) {   // the vector half: the neighbour-list pass gathers (position, force) as one record
                ((double *)&pv[3 * (size_t)s + 1])[1] = v.x;
                pv[3 * (size_t)s + 2] = make_double2(v.y, v.z);
            }
        }
        if (pos_build) {   // distance check of the kept neighbour list
            const double4 b = pos_build[s];
            double dx = q.x - b.x, dy = q.y - b.y, dz = q.z - b.z;
            min_image(box, dx, dy, dz);
            if (dx * dx + dy * dy + dz * dz > half_skin2) flags[0] = 1;
        }
        if (psi_s) {       // K14, keyed by the particle's global index
            uint32_t r[4];
            philox4x32(idx, 0u, timestep, DOMAIN_PARTICLE, seed, PHILOX_KEY1, r);
            const double c = 1.7320508075688772;  // sqrt(3): variance 1
            psi_s[s] = make_double4(uniform_pm(r[0], c), uniform_pm(r[1], c), uniform_pm(r[2], c), 0.0);
        }
        if (far.on) {      // the far-field bin of the particle, from the fractional coordinates of the STORED position (as k_far_records
                           // recomputes them: both must name the same bin)
            double gx, gy, gz;
            frac_coords(box, q.x, q.y, q.z, gx, gy, gz);
            int4 o;
            double4 d;
            far_support(gx, gy, gz, far.G, o, d);
            bin_need = true;
            if (far.G.nxl < far.G.Nx) bin_need = wrapi(o.w - (far.G.x0 - far.G.P), far.G.Nx) < far.G.nxl + 2 * far.G.P;   // within a support of the slab's planes
            bin = bin_index(o.x, o.y, o.z, far.fb);
        }
    }
    if (far.on) {
        const int rk = far_bin_rank(bin_need, bin, far.fb.cnt);
        if (s < N) far.fb.rank_s[s] = rk;
    }
}

__global__ void k_permute_vec(const double4 *__restrict__ vec, const unsigned *__restrict__ tag_s, int N,
                              double4 *__restrict__ vec_s) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= N) return;
    double4 v = vec[tag_s[s]];
    v.w = 0.0;
    vec_s[s] = v;
}

void launch_permute(const double4 *pos, const double4 *vec, const unsigned *group, const unsigned *perm, int N, DBox box,
                    double4 *pos_s, float4 *posf_s, double2 *pv, double4 *vec_s, unsigned *tag_s, hipStream_t s,
                    const double4 *pos_build, double half_skin2, int *flags, CellRanges need, const int *cell_off,
                    const FarBinArgs *far, double4 *psi_s, uint32_t seed, uint32_t timestep, Gate gate, const uint32_t *ts_off) {
    hipLaunchKernelGGL(k_permute, dim3(nblocks(N, TPB)), dim3(TPB), 0, s, pos, vec, group, perm, N, box, pos_s, posf_s, pv, vec_s, tag_s,
                       pos_build, half_skin2, flags, need, cell_off, far ? *far : FarBinArgs{}, psi_s, seed, timestep, gate, ts_off);
}
__global__ void k_gate_decide(int *__restrict__ flags, int *__restrict__ word) {
    const int f = flags[0] | flags[1];
    *word = f;
    if (f) flags[1] = 0;   // the build that follows sets it again if a row overflows
}
void launch_gate_decide(int *flags, int *word, hipStream_t s) { hipLaunchKernelGGL(k_gate_decide, dim3(1), dim3(1), 0, s, flags, word); }
__global__ void k_gate_zero(Gate g, int *__restrict__ a, size_t na, int *__restrict__ b, size_t nb) {
    if (g.closed()) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += (size_t)gridDim.x * blockDim.x) {
        if (i < na) a[i] = 0; else b[i - na] = 0;
    }
}
void launch_gate_zero(Gate g, int *a, size_t na, int *b, size_t nb, hipStream_t s) {
    hipLaunchKernelGGL(k_gate_zero, dim3(std::max(1, std::min(1024, nblocks((long)(na + nb), TPB)))), dim3(TPB), 0, s, g, a, na, b, nb);
}
__global__ void k_gate_copy(Gate g, double4 *__restrict__ dst, const double4 *__restrict__ src, size_t n) {
    if (g.closed()) return;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
void launch_gate_copy(Gate g, double4 *dst, const double4 *src, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_gate_copy, dim3(std::max(1, std::min(4096, nblocks((long)n, TPB)))), dim3(TPB), 0, s, g, dst, src, n);
}
void launch_permute_vec(const double4 *vec, const unsigned *tag_s, int N, double4 *vec_s, hipStream_t s) {
    hipLaunchKernelGGL(k_permute_vec, dim3(nblocks(N, TPB)), dim3(TPB), 0, s, vec, tag_s, N, vec_s);
}

// ------------------------------------------------------------------------------------------------ near field
// K9 gpu_stokes_Mreal_kernel (PSEv1/Mobility.cu:594-687): u_i = self F_i + sum_j [f (I - rr) + g rr] F_j over
// minimum-image neighbours with r < rcut.  The neighbours come from the build's own cell list (HOOMD's
// NeighborListGPUBinned is not available, PSEv1/integrate.py:58-83).
//
// Two phases per thread so the wave does not diverge on the ~15 % of candidates that pass the cutoff: (1) scan the
// 27 neighbour cells (z-runs merged) and push the slots that pass r < rcut into a per-thread LDS queue -- cheap, no
// transcendental work; (2) drain the queue densely: every lane evaluates f, g for a real neighbour.  With LIST the
// drained pairs (j, f, (g-f)/r^2, r) are also written to a per-step ELL pair list that the Lanczos mat-vecs reuse
// (positions do not change inside a step, PSEv1/Brownian.cu:473-521 recomputes them every iteration).
// 44 entries per thread: 44 KB of queue + the 8 KB table of the metric point let THREE workgroups share a CU (48: two)
constexpr int QCAP = 44;
constexpr unsigned JMASK = (1u << 27) - 1;

// Four slots of the 64 rows of a wave form one 4096-byte group of [slot][lane] 16-byte records: a mat-vec reads a group with four
// 16-byte loads per lane (a coalesced dword or dwordx2 load occupies the texture addresser as long as a dwordx4 load,
// tools/microbench/stream_widths: 8 / 16 / 16 clk -- the twelve narrow loads of the round-2 (entry | f | h) planes cost three times that).
//
// What a record holds (round 6): the neighbour's row and the pair's term of the mat-vec, f v + h (d.v) d with d = x_i - x_j (minimum
// image) and h = (g - f) / r^2, as FOUR ROUNDED NUMBERS: fr = f and s = d sqrt|h| (the sign of h in a bit: f v + sgn (s.v) s) -- fr a
// signed 26-bit integer in units of 2^-24 (|f| < 2), s three signed 22-bit mantissas under the exponent es of its largest component
// (value = m 2^(es - 21)): absolute errors <= 3e-8 (fr) and 2^-22 |s|_max, what single precision gives for numbers of order one, in 100
// bits instead of 128 (rounds 6a: four floats + the entry = 20 bytes per pair; the mat-vec is bound by this stream).  The mat-vecs then
// gather ONE thing per pair -- the neighbour's vector row -- instead of the 48-byte (position, vector) record, and neither subtract
// positions nor look up image shifts; the list is only ever read by the Lanczos iteration of M_real^{1/2} psi (tolerance `error`,
// 1e-3 by default; the deterministic M.F of the pass that builds the list stays fp64 -- the reference's whole path is fp32,
// SURVEY.md 2.4-1).  EVERY application of the operator inside a Lanczos iteration uses these rounded numbers -- the vector that
// rides along with the build pass, the list mat-vecs, the rows that did not fit the list -- so the iteration sees ONE symmetric
// matrix: d_ji = -d_ij exactly and rounding to nearest is odd, so both directions of a pair round alike.  (The tests' CPU restatement
// of the algorithm repeats this rounding operation by operation: include/pse_amd.h, the precision note.)
struct PairCoef { int f, mx, my, mz, es; unsigned neg; };
__device__ __forceinline__ PairCoef pair_coef(double f, double h, double dx, double dy, double dz) {
    const double hs = (double)sqrtf((float)fabs(h));
    const double sx = dx * hs, sy = dy * hs, sz = dz * hs;
    const double m = fmax(fabs(sx), fmax(fabs(sy), fabs(sz)));
    int e = 0;
    (void)frexp(m, &e);
    e = e < -100 ? -100 : (e > 100 ? 100 : e);
    const double sc = __hiloint2double((21 - e + 1023) << 20, 0);   // 2^(21 - e): |component| sc < 2^21
    const double lim = 2097151.0;                                   // 2^21 - 1
    PairCoef p;
    p.mx = (int)fmax(-lim, fmin(lim, rint(sx * sc))); p.my = (int)fmax(-lim, fmin(lim, rint(sy * sc))); p.mz = (int)fmax(-lim, fmin(lim, rint(sz * sc)));
    p.es = e;
    p.f = (int)fmax(-33554431.0, fmin(33554431.0, rint(f * 16777216.0)));
    p.neg = h < 0.0 ? 1u : 0u;
    return p;
}
__device__ __forceinline__ void pair_apply(const PairCoef &p, double vx, double vy, double vz, double &ux, double &uy, double &uz) {
    const double sc = __hiloint2double((p.es - 21 + 1023) << 20, 0);
    const double fr = (double)p.f * 5.9604644775390625e-08, sx = (double)p.mx * sc, sy = (double)p.my * sc, sz = (double)p.mz * sc;   // (2^-24)
    double sd = sx * vx + sy * vy + sz * vz;
    if (p.neg) sd = -sd;
    ux += fr * vx + sd * sx; uy += fr * vy + sd * sy; uz += fr * vz + sd * sz;
}
// the 16-byte record: x = row (27) | neg (1) | fr[3:0] (4); y = fr[25:4] (22) | mx[9:0] (10); z = mx[21:10] (12) | my[19:0] (20);
// w = my[21:20] (2) | mz (22) | es + 128 (8)
typedef unsigned nb4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ nb4 nb_pack(unsigned j, const PairCoef &p) {
    const unsigned f = (unsigned)p.f & 0x3FFFFFFu, mx = (unsigned)p.mx & 0x3FFFFFu, my = (unsigned)p.my & 0x3FFFFFu, mz = (unsigned)p.mz & 0x3FFFFFu;
    nb4 w;
    w.x = j | (p.neg ? (1u << 27) : 0u) | (f << 28);
    w.y = (f >> 4) | (mx << 22);
    w.z = (mx >> 10) | (my << 12);
    w.w = (my >> 20) | (mz << 2) | ((unsigned)(p.es + 128) << 24);
    return w;
}
__device__ __forceinline__ PairCoef nb_unpack(nb4 w, bool ok) {
    PairCoef p;
    p.neg = w.x & (1u << 27);
    p.f = ok ? (int)((((w.y & 0x3FFFFFu) << 4) | (w.x >> 28)) << 6) >> 6 : 0;
    p.mx = ok ? (int)((((w.z & 0xFFFu) << 10) | (w.y >> 22)) << 10) >> 10 : 0;
    p.my = ok ? (int)((((w.w & 0x3u) << 20) | (w.z >> 12)) << 10) >> 10 : 0;
    p.mz = ok ? (int)(((w.w >> 2) & 0x3FFFFFu) << 10) >> 10 : 0;
    p.es = ok ? (int)(w.w >> 24) - 128 : 0;
    return p;
}
template <bool STREAM = false>
__device__ __forceinline__ void nb_store(char *rec, int slot, int lane, unsigned j, const PairCoef &p) {
    char *r = rec + (size_t)(slot >> 2) * (4 * NB_REC);
    const nb4 w = nb_pack(j, p);
    if (STREAM) __builtin_nontemporal_store(w, (nb4 *)r + (slot & 3) * 64 + lane);
    else ((nb4 *)r)[(slot & 3) * 64 + lane] = w;
}
constexpr unsigned NB_NEG = 1u << 27;   // entry = neighbour row | NB_NEG if h < 0

// The fp64 operator (F64 instantiations, NbList::c64): the same term f v + sgn (s.v) s with f and s = d sqrt|h| in double -- no rounding
// beyond that of the arithmetic, the root in double.  Every place the Lanczos iteration applies the operator (ride-along vector of the
// build, list mat-vecs, rows that did not fit) goes through pair_coef64 + pair_apply64, and the list carries exactly the four doubles
// pair_coef64 returns: ONE operator, exactly symmetric (d_ji = -d_ij, f and h depend on r^2 alone).
struct PairCoef64 { double f, sx, sy, sz; bool neg; };
__device__ __forceinline__ PairCoef64 pair_coef64(double f, double h, double dx, double dy, double dz) {
    const double hs = sqrt(fabs(h));
    return PairCoef64{f, dx * hs, dy * hs, dz * hs, h < 0.0};
}
__device__ __forceinline__ void pair_apply64(const PairCoef64 &p, double vx, double vy, double vz, double &ux, double &uy, double &uz) {
    double sd = p.sx * vx + p.sy * vy + p.sz * vz;
    if (p.neg) sd = -sd;
    ux += p.f * vx + sd * p.sx; uy += p.f * vy + sd * p.sy; uz += p.f * vz + sd * p.sz;
}
typedef double d4v __attribute__((ext_vector_type(4)));
// record `slot` of a row: the 16-byte record (row | sign; the rounded fields stay zero) and its 32-byte fp64 twin at the same index
template <bool STREAM = false>
__device__ __forceinline__ void nb_store64(char *rec, double4 *rec64, int slot, int lane, unsigned j, const PairCoef64 &p) {
    const size_t k = (size_t)(slot >> 2) * 256 + (slot & 3) * 64 + lane;
    nb4 w;
    w.x = j | (p.neg ? NB_NEG : 0u); w.y = 0u; w.z = 0u; w.w = 128u << 24;
    const d4v c = {p.f, p.sx, p.sy, p.sz};
    if (STREAM) { __builtin_nontemporal_store(w, (nb4 *)rec + k); __builtin_nontemporal_store(c, (d4v *)rec64 + k); }
    else { ((nb4 *)rec)[k] = w; ((d4v *)rec64)[k] = c; }
}

__device__ __forceinline__ void vl_store(char *vrec, int slot, int lane, unsigned j) {
    ((unsigned *)(vrec + (size_t)(slot >> 2) * 1024))[lane * 4 + (slot & 3)] = j;
}

// CL: the f, g coefficient table is copied to LDS first (ncoef doubles of dynamic shared memory).  Every neighbour reads
// 20 coefficients of its own interval: from global memory that was 20 of the 24 L1 accesses per pair and kept the
// texture addresser busy for the whole kernel (rocprofv3: TA_BUSY = duration, 425 M cache accesses = 20 x 21.3 M pairs).
// TWO: a second vector rides along (out2 = M_real vec2): the pass that builds the pair list for M.F also delivers
// M.psi, the first Lanczos mat-vec, for one more gather per neighbour.
// VL: the pass also writes the neighbour list kept across steps -- every pair closer than vl.rskin = rcut + skin (the
// pre-filter and the queue work with that radius; f, g and the pair list still stop at rcut).
// DEV: an owned-particle rank -- the rows come from device memory (DevRowArgs); a separate instantiation, so that the single-GPU
// pass keeps its 166 registers (with the few extra scalars it spilled)
// PK: the drain reads a neighbour's position AND vector from the packed 48-byte record pv[j] (three 16-byte gathers from one or two
// lines instead of four from two arrays): the pass is bound by the drain's round trips through the texture addresser, not by its scan.
// F64 (with LIST): the fp64 Lanczos operator -- the list gets the fp64 plane nb.c64 beside its records, the ride-along vector the
// same un-rounded coefficients (pair_coef64)
template <bool LIST, bool CL, bool TWO, bool VL, bool DEV = false, bool PK = false, bool F64 = false>
__global__ void __launch_bounds__(TPB, ((LIST && CL && !VL) ? 3 : 1))   // the list-building pass of every step: <= 168 VGPRs (it takes 166)
k_mreal_cells(const double4 *__restrict__ pos_s, const float4 *__restrict__ posf_s, const double4 *__restrict__ vec_s,
              double4 *__restrict__ out_s, RowMap rm_arg, const int *__restrict__ cell_off, DBox box, DCells nc, double rcut2,
              float rcut2_pre, double self, const double *__restrict__ coef_g, int ncoef, NbList nb,
              const double4 *__restrict__ vec2_s, double4 *__restrict__ out2_s, VerletList vl,
              double *__restrict__ sums0, int sums0_cap, Gate gate, DevRowArgs dr, const double2 *__restrict__ pvin) {
    if (gate.closed()) return;
    const RowMapRegs rm(rm_arg, DEV ? dr.rm : nullptr);
    if (!DEV) nc.xpad = 0;   // (only owned-particle ranks pad their x layers: a constant here, the term folds away)
    int nb_live = gridDim.x;
    if (DEV) {   // an owned-particle rank: the rows of this pass are known on the device only; the launch covers the capacity
        nb_live = (rm.list_rows() + TPB - 1) / TPB;
        if ((int)blockIdx.x >= nb_live) return;
    }
    // the pass that also writes the kept neighbour list queues every pair within rcut + r_buff (28 per row instead of 21): a deeper
    // queue, or half of the waves would stop for an extra, poorly filled drain in the middle of the walk
    constexpr int QC = VL ? 64 : QCAP;
    __shared__ unsigned queue[QC * TPB];
    extern __shared__ double scoef[];
    const int tid = threadIdx.x;
    if (CL) {
        // intervals padded from 20 to 21 doubles: lanes in different intervals then read different banks (unpadded, interval k
        // and k + 8 collide: two thirds of this kernel's LDS cycles were bank conflicts)
        for (int q = tid; q < ncoef; q += TPB) scoef[(q / (2 * RS_NCOEF)) * (2 * RS_NCOEF + 1) + q % (2 * RS_NCOEF)] = coef_g[q];
        __syncthreads();
    }
    const double *coef = CL ? scoef : coef_g;
    const int lr = xcd_block(blockIdx.x, nb_live) * TPB + tid;       // list row -> sorted row (own rows, then ghost layers)
    const int i_own = rm.row(lr);
    // a padding lane repeats the first row (identical stores, into the same places or into padding list rows) instead of leaving:
    // the wave-level sums at the end then see every lane
    const bool padding = i_own < 0;
    if (padding && !(TWO && sums0)) return;
    const int i = padding ? rm.first_row() : i_own;
    const double4 pi = pos_s[i];
    const double4 vi = vec_s[i];
    double ux = self * vi.x, uy = self * vi.y, uz = self * vi.z;
    double wx = 0.0, wy = 0.0, wz = 0.0;
    if (TWO) { const double4 v2 = vec2_s[i]; wx = self * v2.x; wy = self * v2.y; wz = self * v2.z; }
    double fx, fy, fz;
    frac_coords(box, pi.x, pi.y, pi.z, fx, fy, fz);
    const int cx = cell_coord(fx, nc.nx), cy = cell_coord(fy, nc.ny), cz = cell_coord(fz, nc.nz);
    const bool shift_only = nc.nx > 1 && nc.ny > 1 && nc.nz > 1;   // otherwise finish with the rint minimum image
    int qn = 0, total = 0, vtotal = 0;
    const int lane = lr & 63;
    char *rec = LIST ? nb.data + (size_t)(lr >> 6) * nb.cap * NB_REC : nullptr;
    double4 *rec64 = (LIST && F64) ? nb.c64 + (size_t)(lr >> 6) * nb.cap * 64 : nullptr;
    char *vrec = VL ? (char *)vl.idx + (size_t)(lr >> 6) * (vl.cap / 4) * 1024 : nullptr;
    const double rq2 = VL ? vl.rskin * vl.rskin : rcut2;   // what enters the queue

    // DU queue entries per iteration: their load -> distance -> table -> force chains are independent (one entry at a time the phase
    // was latency-bound: 57 % of its wave-cycles were s_waitcnt; three or four buy nothing more).  Written as loops over small arrays:
    // the compiler then keeps the pass at 166 VGPRs (the hand-interleaved form it replaces took 200), which together with the
    // 44-entry queue is what lets a third workgroup onto the CU: 0.64 -> 0.56 ms.
    auto drain = [&]() {
        constexpr int DU = 2;
        for (int q = 0; q < qn; q += DU) {
            unsigned e[DU]; int j[DU]; bool live[DU];
            double4 p[DU], F[DU], G[DU];
#pragma unroll
            for (int u = 0; u < DU; ++u) {
                live[u] = q + u < qn;
                e[u] = queue[(live[u] ? q + u : q) * TPB + tid];
                j[u] = (int)(e[u] & JMASK);
            }
#pragma unroll
            for (int u = 0; u < DU; ++u) {
                if (PK) {
                    const double2 *r = pvin + 3 * (size_t)j[u];
                    const double2 a = r[0], b = r[1], c = r[2];
                    p[u] = make_double4(a.x, a.y, b.x, 0.0); F[u] = make_double4(b.y, c.x, c.y, 0.0);
                } else { p[u] = pos_s[j[u]]; F[u] = vec_s[j[u]]; }
                if (TWO) G[u] = vec2_s[j[u]];
            }
#pragma unroll
            for (int u = 0; u < DU; ++u) {
                double sx, sy, sz;
                image_shift(e[u] >> 27, box, sx, sy, sz);
                double dx = pi.x - p[u].x - sx, dy = pi.y - p[u].y - sy, dz = pi.z - p[u].z - sz;
                if (!shift_only) min_image(box, dx, dy, dz);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (VL) {
                    if (live[u] && r2 < rq2 && r2 > 0.0) { if (vtotal < vl.cap) vl_store(vrec, vtotal, lane, (unsigned)j[u]); ++vtotal; }
                }
                const double t = VL ? fmin(r2, rcut2) : r2;   // the table ends at rcut
                double f, h;
                if (CL) eval_fg<2 * RS_NCOEF + 1>(t, coef, f, h);
                else eval_fg(t, coef, f, h);
                const bool in = live[u] && r2 < rcut2 && r2 > 0.0;   // the fp64 cutoff decides
                if (!in) { f = 0.0; h = 0.0; }
                // A pass that writes the pair list serves a Lanczos iteration: the vector of that iteration (vec2 when F rides in
                // front, else vec itself) sees the rounded pair coefficients the list carries (pair_coef, nb_store); F never does.
                if (!LIST || TWO) {
                    const double rd = (dx * F[u].x + dy * F[u].y + dz * F[u].z) * h;
                    ux += f * F[u].x + rd * dx; uy += f * F[u].y + rd * dy; uz += f * F[u].z + rd * dz;
                }
                if (LIST && F64) {
                    const PairCoef64 pc = pair_coef64(f, h, dx, dy, dz);
                    if (TWO) pair_apply64(pc, G[u].x, G[u].y, G[u].z, wx, wy, wz);
                    else pair_apply64(pc, F[u].x, F[u].y, F[u].z, ux, uy, uz);
                    if (in) {   // row | sign in 16 B, (f, s) in 32 B of doubles
                        if (total < nb.cap) nb_store64<true>(rec, rec64, total, lane, (unsigned)j[u], pc);
                        ++total;
                    }
                } else if (LIST) {
                    const PairCoef pc = pair_coef(f, h, dx, dy, dz);
                    if (TWO) pair_apply(pc, G[u].x, G[u].y, G[u].z, wx, wy, wz);
                    else pair_apply(pc, F[u].x, F[u].y, F[u].z, ux, uy, uz);
                    if (in) {   // 16 B per pair: row | sign | fr | s
                        if (total < nb.cap) nb_store<true>(rec, total, lane, (unsigned)j[u], pc);
                        ++total;
                    }
                } else if (TWO) {
                    const double sd = (dx * G[u].x + dy * G[u].y + dz * G[u].z) * h;
                    wx += f * G[u].x + sd * dx; wy += f * G[u].y + sd * dy; wz += f * G[u].z + sd * dz;
                }
            }
        }
        qn = 0;
    };

    // Scan in single precision on a float copy of the positions against a cutoff enlarged by the rounding bound, eight
    // candidates per round trip (a float4 is half the registers of a double4: the scan is bound by dependent round
    // trips at three waves per SIMD); the drain repeats the test in double precision, so the neighbour set is exactly
    // the fp64 one.
    constexpr int SU = 8;
    if (!shift_only) {   // fewer than three cells along some axis: minimum-image search in double precision
        for_each_run(nc, cell_off, cx, cy, cz, [&](int jb, int je, unsigned code) {
            for (int j = jb; j < je; ++j) {
                const double4 pj = pos_s[j];
                double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                min_image(box, dx, dy, dz);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (r2 < rq2 && j != i && r2 > 0.0) {
                    queue[qn * TPB + tid] = (unsigned)j | (code << 27);
                    ++qn;
                }
                if (__any(qn > QC - SU)) drain();
            }
        });
    } else {
        // Every lane walks ITS runs at its own pace, SU candidates of one run per round (the bounds of the run after the current
        // one are already loaded when the current one ends).  Stepping through "run k of all 64 lanes" together cost the longest
        // run k of the wave nine times over: 288 load instructions per wave for 137 candidates per lane; this way ~200.
        // the runs of this lane, one at a time (the order of for_each_run): up to three per (x, y) column.  Written out in place --
        // one site, no closure: as a lambda called from two places the iterator state went to scratch memory.
        const int zb0 = cz / nc.bz, zi0 = cz - zb0 * nc.bz;
        int ox = -1, oy = -2, rk = 0, nparts = 0;
        int f0 = 0, l0 = 0, f1 = 0, l1 = 0, f2 = 0, l2 = 0;
        unsigned c0 = 13u, c1 = 13u, c2 = 13u;
        int j = 0, je = 0, jn = 0, jen = 0;
        unsigned code = 13u, code_n = 13u;
        float qx = 0.f, qy = 0.f, qz = 0.f;
        bool have_n = true;
        int pend = 2;   // first round: prime the prefetch, then make the first run current
        while (true) {
            do {
                if (j >= je && have_n) {   // the current run is used up: the prefetched one becomes current (an empty one is skipped next round)
                    j = jn; je = jen; code = code_n;
                    double sx, sy, sz;
                    image_shift(code, box, sx, sy, sz);
                    qx = (float)(pi.x - sx); qy = (float)(pi.y - sy); qz = (float)(pi.z - sz);
                    if (rk >= nparts) {    // next (x, y) column
                        if (++oy > 1) { oy = -1; ++ox; }
                        if (ox > 1) have_n = false;
                        else {
                            int ax = cx + ox, wx = 0, ay = cy + oy, wy = 0;
                            if (ax < 0) { ax += nc.nx; wx = -1; } else if (ax >= nc.nx) { ax -= nc.nx; wx = 1; }
                            if (ay < 0) { ay += nc.ny; wy = -1; } else if (ay >= nc.ny) { ay -= nc.ny; wy = 1; }
                            const unsigned cxy = (unsigned)((wx + 1) * 9 + (wy + 1) * 3);
                            int s0, s1, s2; unsigned d0, d1, d2;
                            z_neighbour_slot(nc, ax, ay, cz, zb0, zi0, -1, cxy, s0, d0);
                            z_neighbour_slot(nc, ax, ay, cz, zb0, zi0, 0, cxy, s1, d1);
                            z_neighbour_slot(nc, ax, ay, cz, zb0, zi0, 1, cxy, s2, d2);
                            const bool m01 = s1 == s0 + 1 && d1 == d0, m12 = s2 == s1 + 1 && d2 == d1;
                            f0 = s0; c0 = d0;
                            if (m01 && m12) { l0 = s2; nparts = 1; }
                            else if (m01) { l0 = s1; f1 = l1 = s2; c1 = d2; nparts = 2; }
                            else if (m12) { l0 = s0; f1 = s1; l1 = s2; c1 = d1; nparts = 2; }
                            else { l0 = s0; f1 = l1 = s1; c1 = d1; f2 = l2 = s2; c2 = d2; nparts = 3; }
                            rk = 0;
                        }
                    }
                    if (have_n) {
                        const int sa = rk == 0 ? f0 : (rk == 1 ? f1 : f2), sb = (rk == 0 ? l0 : (rk == 1 ? l1 : l2)) + 1;
                        code_n = rk == 0 ? c0 : (rk == 1 ? c1 : c2);
                        ++rk;
                        jn = cell_off[sa]; jen = cell_off[sb];   // consumed at the next switch
                    }
                }
            } while (--pend > 0);
            pend = 1;
            const bool work = j < je;
            if (!__any(work || have_n)) break;
            float4 pj[SU];
#pragma unroll
            for (int u = 0; u < SU; ++u) pj[u] = posf_s[work ? min(j + u, je - 1) : i];   // independent loads in flight
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                const int jj = j + u;
                const float dx = qx - pj[u].x, dy = qy - pj[u].y, dz = qz - pj[u].z;
                const float r2 = dx * dx + dy * dy + dz * dz;
                if (jj < je && r2 < rcut2_pre && jj != i) {
                    queue[qn * TPB + tid] = (unsigned)jj | (code << 27);
                    ++qn;
                }
            }
            j += SU;
            // drain together: a lane-private "queue full" branch would serialise the wave once per lane
            if (__any(qn > QC - SU)) drain();
        }
    }
    drain();
    out_s[i] = make_double4(ux, uy, uz, 0.0);
    if (TWO) {
        out2_s[i] = make_double4(wx, wy, wz, 0.0);
        if (DEV && dr.stage_hi) {   // rows of the last layers: parked for the exchange with the right neighbour
            const int lb = dr.lr->last_begin, no = dr.lr->n_own;
            if (i >= lb && i < no && i - lb < dr.stage_cap) dr.stage_hi[i - lb] = make_double4(wx, wy, wz, 0.0);   // (k_local_scatter refuses a step whose last layers exceed the capacity; the bound is the belt to its braces)
        }
        if (sums0) {    // the sums of Lanczos iteration 0 (x = psi, y = M psi): x.x and x.y per wavefront (was k_lz_dots: one more pass over both)
            const double4 v2 = vec2_s[i];
            const double a = padding ? 0.0 : v2.x * v2.x + v2.y * v2.y + v2.z * v2.z, b = padding ? 0.0 : v2.x * wx + v2.y * wy + v2.z * wz;
            const double sa = wave_sum(a), sb = wave_sum(b);
            if ((tid & 63) == 0) {
                const int slot = blockIdx.x * (TPB / 64) + (tid >> 6);
                sums0[slot] = sa; sums0[sums0_cap + slot] = sb; sums0[2 * sums0_cap + slot] = 0.0;
            }
        }
    }
    if (LIST) {
        if (total > nb.cap) total = -1;   // the row did not fit: the mat-vecs of this step walk the cells for it
        nb.cnt[i] = total;
    }
    if (VL) {
        if (vtotal > vl.cap) { vtotal = -1; vl.flags[1] = 1; }
        vl.cnt[i] = vtotal;
    }
}

// The near-field pass of a step that REUSES the neighbour list: no cell walk -- every row reads its entries (groups of four,
// one 16-byte load), gathers the neighbours' (position, vec) records (+ vec2), takes the minimum image itself (particles may
// have crossed the periodic boundary since the build) and evaluates f, g densely; pairs beyond rcut (about a quarter at
// skin = 0.4) contribute zero.  LIST: writes the step's pair list for the Lanczos mat-vecs, exactly as the cell pass does.
// PK: pv holds (position, vec_s) records (three 16-byte gathers per neighbour instead of four).  F64: as in k_mreal_cells.
template <bool LIST, bool TWO, bool PK, bool F64 = false>
__global__ void __launch_bounds__(TPB)
k_mreal_verlet(const double4 *__restrict__ pos_s, const double2 *__restrict__ pv, const double4 *__restrict__ vec_s,
               double4 *__restrict__ out_s, int N, DBox box, double rcut2, double self, const double *__restrict__ coef_g, int ncoef,
               NbList nb, VerletList vl, const double4 *__restrict__ vec2_s, double4 *__restrict__ out2_s, Gate gate) {
    if (gate.closed()) return;
    extern __shared__ double scoef[];
    const int tid = threadIdx.x;
    for (int q = tid; q < ncoef; q += TPB) scoef[(q / (2 * RS_NCOEF)) * (2 * RS_NCOEF + 1) + q % (2 * RS_NCOEF)] = coef_g[q];
    __syncthreads();
    const int i = xcd_block(blockIdx.x, gridDim.x) * TPB + tid;
    if (i >= N) return;
    const double4 pi = pos_s[i];
    const double4 vi = vec_s[i];
    double ux = self * vi.x, uy = self * vi.y, uz = self * vi.z;
    double wx = 0.0, wy = 0.0, wz = 0.0;
    if (TWO) { const double4 v2 = vec2_s[i]; wx = self * v2.x; wy = self * v2.y; wz = self * v2.z; }
    const int lane = i & 63, cnt = vl.cnt[i];
    const char *vrec = (const char *)vl.idx + (size_t)(i >> 6) * (vl.cap / 4) * 1024;
    char *rec = LIST ? nb.data + (size_t)(i >> 6) * nb.cap * NB_REC : nullptr;
    double4 *rec64 = (LIST && F64) ? nb.c64 + (size_t)(i >> 6) * nb.cap * 64 : nullptr;
    int total = 0;
    constexpr int U = 4;
    for (int s0 = 0; s0 < cnt; s0 += U) {
        const uint4 e4 = ((const uint4 *)(vrec + (size_t)(s0 >> 2) * 1024))[lane];
        unsigned e[U] = {e4.x, e4.y, e4.z, e4.w};
        double2 a[U], b[U], c[U];
        double4 G[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u && s0 + u >= cnt) e[u] = e[0];          // slots past the row's count were never written
            if (PK) {
                const double2 *r = pv + 3 * (size_t)e[u];
                a[u] = r[0]; b[u] = r[1]; c[u] = r[2];
            } else {
                const double4 pj = pos_s[e[u]], Fj = vec_s[e[u]];
                a[u] = make_double2(pj.x, pj.y); b[u] = make_double2(pj.z, Fj.x); c[u] = make_double2(Fj.y, Fj.z);
            }
            if (TWO) G[u] = vec2_s[e[u]];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double dx = pi.x - a[u].x, dy = pi.y - a[u].y, dz = pi.z - b[u].x;
            const double ny = rint(dy * box.iLy);
            dy -= ny * box.Ly; dx -= ny * box.xy * box.Ly;
            const double nx = rint(dx * box.iLx), nz = rint(dz * box.iLz);
            dx -= nx * box.Lx; dz -= nz * box.Lz;
            const double r2 = dx * dx + dy * dy + dz * dz;
            const bool in = s0 + u < cnt && r2 < rcut2 && r2 > 0.0;
            double f, h;
            eval_fg<2 * RS_NCOEF + 1>(fmin(r2, rcut2), scoef, f, h);
            if (!in) { f = 0.0; h = 0.0; }
            const double Fx = b[u].y, Fy = c[u].x, Fz = c[u].y;
            if (!LIST || TWO) {
                const double rd = (dx * Fx + dy * Fy + dz * Fz) * h;
                ux += f * Fx + rd * dx; uy += f * Fy + rd * dy; uz += f * Fz + rd * dz;
            }
            if (LIST && F64) {
                const PairCoef64 pc = pair_coef64(f, h, dx, dy, dz);
                if (TWO) pair_apply64(pc, G[u].x, G[u].y, G[u].z, wx, wy, wz);
                else pair_apply64(pc, Fx, Fy, Fz, ux, uy, uz);
                if (in) {
                    if (total < nb.cap) nb_store64(rec, rec64, total, lane, e[u], pc);
                    ++total;
                }
            } else if (LIST) {   // (as the cell pass: the vector of the Lanczos iteration sees the coefficients the list carries)
                const PairCoef pc = pair_coef(f, h, dx, dy, dz);
                if (TWO) pair_apply(pc, G[u].x, G[u].y, G[u].z, wx, wy, wz);
                else pair_apply(pc, Fx, Fy, Fz, ux, uy, uz);
                if (in) {
                    if (total < nb.cap) nb_store(rec, total, lane, e[u], pc);
                    ++total;
                }
            } else if (TWO) {
                const double sd = (dx * G[u].x + dy * G[u].y + dz * G[u].z) * h;
                wx += f * G[u].x + sd * dx; wy += f * G[u].y + sd * dy; wz += f * G[u].z + sd * dz;
            }
        }
    }
    out_s[i] = make_double4(ux, uy, uz, 0.0);
    if (TWO) out2_s[i] = make_double4(wx, wy, wz, 0.0);
    if (LIST) nb.cnt[i] = total > nb.cap ? -1 : total;   // -1: the mat-vecs of this step walk the neighbour list for this row
}

// eval_fg with the Horner steps as a rolled loop (the same operations in the same order: bit-identical results): for the rare rows of
// the pair-list mat-vec that did not fit the list -- unrolled, its twenty coefficient loads in flight set the register count of the
// whole kernel (126), which the list loop itself does not need
__device__ __forceinline__ void eval_fg_lean(double r2, const double *__restrict__ coef, double &f, double &gmf_r2) {
    const double ir = rsqrt(r2), r = r2 * ir, ir2 = ir * ir;
    double f0, g0;
    if (r > 2.0) { const double ir3 = ir * ir2; f0 = 0.75 * ir + 0.5 * ir3; g0 = 1.5 * ir - ir3; }
    else { f0 = 1.0 - 0.28125 * r; g0 = 1.0 - 0.1875 * r; }
    const double s = r * RS_PER_UNIT;
    const int k = (int)s;
    const double t = 2.0 * (s - k) - 1.0;
    const double *c = coef + (size_t)k * (2 * RS_NCOEF);
    double fw = c[RS_DEG], gw = c[RS_NCOEF + RS_DEG];
#pragma unroll 1
    for (int q = RS_DEG - 1; q >= 0; --q) {
        fw = fma(fw, t, c[q]);
        gw = fma(gw, t, c[RS_NCOEF + q]);
    }
    f = f0 - fw;
    gmf_r2 = ((g0 - gw) - f) * ir2;
}

// mat-vec from the pair list (one thread per particle, ELL layout: slot-major so a wave reads contiguous rows).
// Per pair 16 B of list from HBM -- row | sign | fr | s, see nb_pack -- plus the neighbour's vector row gathered through L2 (24 bytes
// of doubles, or 16 from its mirror: VQ): no positions, no image shifts.  FUSE adds the Lanczos epilogue (see LzFuse).
// WSP = 4: the four waves of a workgroup share ONE block of 64 rows and take every fourth group of slots each (partial sums
// through LDS): the waves resident on a CU then gather from a quarter as many neighbourhoods (the kernel is bound by L1 misses).
// FUSE: 0 none; 1 the three sums of the one-step iteration; 2 the Gram sums of a two-step block (this launch is its SECOND
// mat-vec: vec = w1 = M q, result w2); 3 the sums of a single step in the two-step driver (vec = q, result w1); 4 the one-step
// iteration of a single GPU from j = 1 on: x.y alone (slot 1 of the partials) -- x.x and x.x_{j-1} come from the k_lz_update that
// wrote x (LzFuse.upd), so x_{j-1} is not read here at all.
// VQ: the neighbours' rows come from the 16-byte mirror of the vector (vq_pack, pse_device.h): ONE gather per pair instead of two.
// F64: the fp64 operator -- the coefficients from the 32-byte plane nb.c64 (the 16-byte record gives the row and the sign of h), the
// neighbours' rows as doubles (never VQ), the rows that did not fit the list through pair_coef64: 48 B of list per pair instead of 16.
// packed: vec_s and / or out_s hold 24-byte rows (a rows24 handle: the basis and the results of these mat-vecs); every read of vec_s --
// the own row, the neighbours of a row that walks the cells or the kept list, the gathers without VQ -- and the one store go by it.
template <int FUSE, int UNROLL, int NT, int WSP = 1, bool VQ = false, bool F64 = false>
__global__ void __launch_bounds__(NT, (WSP == 4 ? 5 : 1))   // the split kernel: <= 96 VGPRs, five workgroups per CU (it is bound by the round trips its waves have in flight)
k_mreal_list(const double4 *__restrict__ pos_s, const double4 *__restrict__ vec_s, double4 *__restrict__ out_s, RowMap rm_arg,
             DBox box, double self, NbList nb, LzFuse lz,
             const int *__restrict__ cell_off, DCells nc, double rcut2, const double *__restrict__ coef, VerletList vl,
             const int *__restrict__ stop, DevRowArgs dr, const vq4 *__restrict__ vec_q = nullptr, int packed = 0) {
    if (stop && *stop) return;   // the Lanczos iteration has ended (device-side decision)
    // packed (uniform over the launch): bit 0 -- vec_s holds 24-byte rows, bit 1 -- out_s does (pse_device.h VecIn / VecOut)
    const VecIn vin{reinterpret_cast<const double *>(vec_s), packed & 1};
    const VecOut vout{reinterpret_cast<double *>(out_s), (packed >> 1) & 1};
    const RowMapRegs rm(rm_arg, dr.rm);
    int nb_live = gridDim.x;
    if (dr.rm) {   // an owned-particle rank: rows from device memory; workgroups past the last one still own a slot of the partial sums
        nb_live = (rm.list_rows() + (WSP > 1 ? 64 : NT) - 1) / (WSP > 1 ? 64 : NT);
        if ((int)blockIdx.x >= nb_live) {
            if (FUSE && threadIdx.x == 0)
                for (int t = 0; t < (FUSE == 2 || FUSE == 3 ? (int)LZ_NGRAM : 3); ++t) lz.partials[(size_t)t * lz.npart_cap + blockIdx.x] = 0.0;
            return;
        }
    }
    __shared__ double sh[4];
    static_assert(WSP == 1 || NT == 64 * WSP, "split rows: one wave per slot phase");
    const int wv = WSP > 1 ? (int)(threadIdx.x >> 6) : 0;
    const int lr = WSP > 1 ? xcd_block(blockIdx.x, nb_live) * 64 + (int)(threadIdx.x & 63)
                           : xcd_block(blockIdx.x, nb_live) * NT + (int)threadIdx.x;
    const int i = rm.row(lr);
    const bool active = i >= 0;
    double ux = 0.0, uy = 0.0, uz = 0.0;
    double4 vi = make_double4(0.0, 0.0, 0.0, 0.0);
    if (active) {
        row_load(vin, i, vi.x, vi.y, vi.z);
        const int cnt = nb.cnt[i];
        if (cnt >= 0) {
            if (wv == 0) { ux = self * vi.x; uy = self * vi.y; uz = self * vi.z; }
            const int lane = lr & 63;
            const char *rec = nb.data + (size_t)(lr >> 6) * nb.cap * NB_REC;
            // software-pipelined by hand: the list entries of UNROLL slots, then their gathers, then the arithmetic -- left to the
            // compiler every slot waited for its own load -> gather chain (the kernel was latency-bound at 1.9 TB/s).  Branch-free:
            // slots past cnt re-read the last valid one with zero coefficients.
            static_assert(UNROLL == 4, "one list group per iteration");
            for (int s0 = UNROLL * wv; s0 < cnt; s0 += UNROLL * WSP) {
                const char *grp = rec + (size_t)(s0 >> 2) * (4 * NB_REC);
                // streamed once: non-temporal, so the list does not evict the neighbour rows the gathers reuse from L1
                unsigned e[UNROLL];
                nb4 c[UNROLL];
                d4v c64[F64 ? UNROLL : 1];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    c[u] = __builtin_nontemporal_load((const nb4 *)grp + u * 64 + lane);
                    if (F64) c64[u] = __builtin_nontemporal_load((const d4v *)nb.c64 + (size_t)(lr >> 6) * nb.cap * 64 + (size_t)(s0 >> 2) * 256 + u * 64 + lane);
                    e[u] = c[u].x;
                    if (u && s0 + u >= cnt) e[u] = e[0];          // slots past the row's count were never written
                }
                double2 vxy[UNROLL];
                double vz[UNROLL];
                vq4 vq[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    if (VQ && !F64) { vq[u] = vec_q[e[u] & JMASK]; continue; }   // the row in 16 bytes: one gather
                    if (vin.packed) { row24_load(vin.p, e[u] & JMASK, vxy[u].x, vxy[u].y, vz[u]); continue; }
                    const double4 *vj = vec_s + (e[u] & JMASK);   // 24 of the row's 32 bytes: a 16- and an 8-byte gather from one line
                    vxy[u] = *reinterpret_cast<const double2 *>(vj);
                    vz[u] = vj->z;
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const bool ok = s0 + u < cnt;
                    if (F64) {   // (selects, not products: the slots past cnt hold whatever the memory held)
                        const PairCoef64 pc{ok ? c64[u].x : 0.0, ok ? c64[u].y : 0.0, ok ? c64[u].z : 0.0, ok ? c64[u].w : 0.0, (c[u].x & NB_NEG) != 0u};
                        pair_apply64(pc, vxy[u].x, vxy[u].y, vz[u], ux, uy, uz);
                        continue;
                    }
                    const PairCoef pc = nb_unpack(c[u], ok);
                    if (VQ) { vq_unpack(vq[u], vxy[u].x, vxy[u].y, vz[u]); }
                    pair_apply(pc, vxy[u].x, vxy[u].y, vz[u], ux, uy, uz);
                }
            }
        } else if (wv != 0) {
            // overflow rows are computed whole by the first wave
        } else if (vl.idx) {
            // the row did not fit the pair list and the step runs on the kept neighbour list (the cells are those of its build)
            const double4 pi = pos_s[i];
            ux = self * vi.x; uy = self * vi.y; uz = self * vi.z;
            const int lane = i & 63, vc = vl.cnt[i];
            const char *vrec = (const char *)vl.idx + (size_t)(i >> 6) * (vl.cap / 4) * 1024;
            for (int sl = 0; sl < vc; ++sl) {
                const unsigned j = ((const unsigned *)(vrec + (size_t)(sl >> 2) * 1024))[lane * 4 + (sl & 3)];
                const double4 pj = pos_s[j];
                double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                min_image(box, dx, dy, dz);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (r2 < rcut2 && r2 > 0.0) {
                    double f, h;
                    eval_fg_lean(r2, coef, f, h);
                    double3 Fj;
                    row_load(vin, j, Fj.x, Fj.y, Fj.z);
                    if (F64) pair_apply64(pair_coef64(f, h, dx, dy, dz), Fj.x, Fj.y, Fj.z, ux, uy, uz);
                    else pair_apply(pair_coef(f, h, dx, dy, dz), Fj.x, Fj.y, Fj.z, ux, uy, uz);   // (the coefficients the list would have carried)
                }
            }
        } else {
            // the row did not fit the list (dense cluster): walk the cells, as the pass that built the list did
            const double4 pi = pos_s[i];
            ux = self * vi.x; uy = self * vi.y; uz = self * vi.z;
            double fx, fy, fz;
            frac_coords(box, pi.x, pi.y, pi.z, fx, fy, fz);
            const int cx = cell_coord(fx, nc.nx), cy = cell_coord(fy, nc.ny), cz = cell_coord(fz, nc.nz);
            for_each_run(nc, cell_off, cx, cy, cz, [&](int jb, int je, unsigned) {
                for (int j = jb; j < je; ++j) {
                    const double4 pj = pos_s[j];
                    double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                    min_image(box, dx, dy, dz);
                    const double r2 = dx * dx + dy * dy + dz * dz;
                    if (r2 < rcut2 && j != i && r2 > 0.0) {
                        double f, h;
                        eval_fg_lean(r2, coef, f, h);
                        double3 Fj;
                        row_load(vin, j, Fj.x, Fj.y, Fj.z);
                        if (F64) pair_apply64(pair_coef64(f, h, dx, dy, dz), Fj.x, Fj.y, Fj.z, ux, uy, uz);
                        else pair_apply(pair_coef(f, h, dx, dy, dz), Fj.x, Fj.y, Fj.z, ux, uy, uz);
                    }
                }
            });
        }
    }
    if (WSP > 1) {   // the other waves' shares of the rows
        __shared__ double red[WSP > 1 ? (WSP - 1) * 3 * 64 : 1];
        const int ln = threadIdx.x & 63;
        if (wv > 0) { red[((wv - 1) * 3 + 0) * 64 + ln] = ux; red[((wv - 1) * 3 + 1) * 64 + ln] = uy; red[((wv - 1) * 3 + 2) * 64 + ln] = uz; }
        __syncthreads();
        if (wv > 0) return;
        for (int w = 0; w < WSP - 1; ++w) { ux += red[(w * 3 + 0) * 64 + ln]; uy += red[(w * 3 + 1) * 64 + ln]; uz += red[(w * 3 + 2) * 64 + ln]; }
    }
    if (FUSE == 2 || FUSE == 3) {   // two-step driver: the sums the block scalars are derived from (see k_lz_block), slots LZG_*
        double g[LZ_NGRAM];
#pragma unroll
        for (int t = 0; t < LZ_NGRAM; ++t) g[t] = 0.0;
        if (active) {
            auto dot = [](const double4 &x, double yx, double yy, double yz) { return x.x * yx + x.y * yy + x.z * yz; };
            const double4 z4 = make_double4(0.0, 0.0, 0.0, 0.0);
            const double4 p = lz.p ? lz.p[i] : z4;
            if (FUSE == 2) {   // vi = w1, (ux, uy, uz) = w2
                const double4 q = lz.q[i], u = lz.u ? lz.u[i] : z4;
                g[LZG_QW1] = dot(q, vi.x, vi.y, vi.z); g[LZG_W1W1] = dot(vi, vi.x, vi.y, vi.z); g[LZG_W1W2] = dot(vi, ux, uy, uz);
                g[LZG_W2W2] = ux * ux + uy * uy + uz * uz; g[LZG_PW1] = dot(p, vi.x, vi.y, vi.z);
                g[LZG_PW2] = dot(p, ux, uy, uz); g[LZG_UW2] = dot(u, ux, uy, uz); g[LZG_QQ] = dot(q, q.x, q.y, q.z);
            } else {           // vi = q, (ux, uy, uz) = w1
                g[LZG_QW1] = dot(vi, ux, uy, uz); g[LZG_W1W1] = ux * ux + uy * uy + uz * uz; g[LZG_PW1] = dot(p, ux, uy, uz);
                g[LZG_QQ] = dot(vi, vi.x, vi.y, vi.z);
            }
        }
        static_assert(FUSE < 2 || FUSE == 4 || NT == 64 || WSP > 1, "Gram sums: one wave per block of rows");
#pragma unroll
        for (int t = 0; t < LZ_NGRAM; ++t) {
            if (FUSE == 3 && t != LZG_QW1 && t != LZG_W1W1 && t != LZG_PW1 && t != LZG_QQ) { if (threadIdx.x == 0) lz.partials[(size_t)t * lz.npart_cap + blockIdx.x] = 0.0; continue; }   // (compile-time: the loop is unrolled)
            const double v = wave_sum(g[t]);
            if (threadIdx.x == 0) lz.partials[(size_t)t * lz.npart_cap + blockIdx.x] = v;
        }
    } else if (FUSE == 4) {   // x.y alone
        static_assert(FUSE != 4 || NT == 64 || WSP > 1, "one wave per block of rows");
        const double b = wave_sum(active ? vi.x * ux + vi.y * uy + vi.z * uz : 0.0);
        if (threadIdx.x == 0) lz.partials[lz.npart_cap + blockIdx.x] = b;
    } else if (FUSE) {   // x = vec (unnormalised Lanczos vector), y = M x: partial sums of x.x, x.y, x.x_{j-1}
        double a = 0.0, b = 0.0, c = 0.0;
        if (active) {
            a = vi.x * vi.x + vi.y * vi.y + vi.z * vi.z;
            b = vi.x * ux + vi.y * uy + vi.z * uz;
            if (lz.vprev) {
                const double4 m = lz.vprev[i];
                c = vi.x * m.x + vi.y * m.y + vi.z * m.z;
            }
        }
        if (NT == 64 || WSP > 1) { a = wave_sum(a); b = wave_sum(b); c = wave_sum(c); }
        else { a = block_sum(a, sh); __syncthreads(); b = block_sum(b, sh); __syncthreads(); c = block_sum(c, sh); }
        if (threadIdx.x == 0) {
            lz.partials[blockIdx.x] = a; lz.partials[lz.npart_cap + blockIdx.x] = b; lz.partials[2 * lz.npart_cap + blockIdx.x] = c;
        }
    }
    if (active) {
        row_store(vout, i, ux, uy, uz);
        if (dr.stage_hi) {   // rows of the last layers: parked for the exchange with the right neighbour
            const int lb = dr.lr->last_begin, no = dr.lr->n_own;
            if (i >= lb && i < no && i - lb < dr.stage_cap) dr.stage_hi[i - lb] = make_double4(ux, uy, uz, 0.0);
        }
    }
}

static size_t mreal_lds_bytes(int ncoef) { return (size_t)(ncoef / (2 * RS_NCOEF)) * (2 * RS_NCOEF + 1) * sizeof(double); }   // padded copy
bool mreal_table_in_lds(int ncoef) { return mreal_lds_bytes(ncoef) <= 14 * 1024; }   // with the 44 KB queue: three workgroups per CU up to 9 KB of table, two beyond

void launch_mreal(const double4 *pos_s, const float4 *posf_s, const double4 *vec_s, double4 *out_s, RowMap rm,
                  const int *cell_off, DBox box, DCells nc, double rcut, double self, const double *coef, int ncoef, NbList nb,
                  int mode, hipStream_t s, const double4 *vec2_s, double4 *out2_s, VerletList vl, int vl_mode, const double2 *pv,
                  double *sums0, int sums0_cap, double *scal, Gate gate, DevRowArgs dr) {
    const int rows = dr.rm ? dr.rows_cap : rm.list_rows();
    if (rows <= 0) return;
    const dim3 g(nblocks(rows, TPB)), b(TPB);
    const size_t cb = mreal_lds_bytes(ncoef);
    const bool cl = mreal_table_in_lds(ncoef);
    const bool f64 = nb.c64 != nullptr;   // the fp64 Lanczos operator (the instantiations with F64)
    if (mode == MREAL_USE_LIST) {
        if (f64) hipLaunchKernelGGL((k_mreal_list<0, 4, TPB, 1, false, true>), g, b, 0, s, pos_s, vec_s, out_s, rm, box, self, nb, LzFuse{}, cell_off, nc, rcut * rcut, coef,
                                    vl_mode == VL_USE ? vl : VerletList{}, nullptr, DevRowArgs{}, nullptr);
        else hipLaunchKernelGGL((k_mreal_list<0, 4, TPB>), g, b, 0, s, pos_s, vec_s, out_s, rm, box, self, nb, LzFuse{}, cell_off, nc, rcut * rcut, coef,
                                vl_mode == VL_USE ? vl : VerletList{}, nullptr, DevRowArgs{});
        return;
    }
    const bool list = mode == MREAL_BUILD_LIST, two = list && vec2_s != nullptr;
    if (vl_mode == VL_USE) {   // rows [0, N) of a single rank; the table is in LDS (the caller checked mreal_table_in_lds)
        const int hi = rm.hi[0];
#define PSE_VERLET(L, T, F) do { if (pv) hipLaunchKernelGGL((k_mreal_verlet<L, T, true, F>), g, b, cb, s, pos_s, pv, vec_s, out_s, hi, box, rcut * rcut, self, coef, ncoef, nb, vl, two ? vec2_s : nullptr, out2_s, gate); \
        else hipLaunchKernelGGL((k_mreal_verlet<L, T, false, F>), g, b, cb, s, pos_s, pv, vec_s, out_s, hi, box, rcut * rcut, self, coef, ncoef, nb, vl, two ? vec2_s : nullptr, out2_s, gate); } while (0)
        if (list && two) { if (f64) PSE_VERLET(true, true, true); else PSE_VERLET(true, true, false); }
        else if (list) { if (f64) PSE_VERLET(true, false, true); else PSE_VERLET(true, false, false); }
        else PSE_VERLET(false, false, false);
#undef PSE_VERLET
        return;
    }
    // pre-filter cutoff: coordinates (and image-shifted coordinates) are below 1.5 (Lx + |xy| Ly + Ly + Lz), rounded to
    // 2^-24 relative a few times on the way to a separation component
    const bool wr = vl_mode == VL_WRITE && cl;
    const double cmax = 1.5 * (box.Lx + std::fabs(box.xy) * box.Ly + box.Ly + box.Lz);
    const double rpre = (wr ? vl.rskin : rcut) + 16.0 * cmax * 5.97e-8;
    const float rcut2_pre = (float)(rpre * rpre * (1.0 + 1e-6));
#define PSE_CELLS_F(L, C, T, V, F) hipLaunchKernelGGL((k_mreal_cells<L, C, T, V, false, false, F>), g, b, (C) ? cb : 0, s, pos_s, posf_s, vec_s, out_s, rm, cell_off, box, nc, rcut * rcut, rcut2_pre, self, coef, ncoef, nb, two ? vec2_s : nullptr, out2_s, vl, (two && (C)) ? sums0 : nullptr, sums0_cap, gate, dr, nullptr)
#define PSE_CELLS_PK_F(L, T, D, F) hipLaunchKernelGGL((k_mreal_cells<L, true, T, false, D, true, F>), g, b, cb, s, pos_s, posf_s, vec_s, out_s, rm, cell_off, box, nc, rcut * rcut, rcut2_pre, self, coef, ncoef, nb, two ? vec2_s : nullptr, out2_s, vl, (two && !(D)) ? sums0 : nullptr, sums0_cap, gate, dr, pv)
    // (only the passes that write the pair list have an F64 twin: the others apply the exact f, h to F alone)
#define PSE_CELLS(L, C, T, V) do { if ((L) && f64) PSE_CELLS_F(L, C, T, V, (L)); else PSE_CELLS_F(L, C, T, V, false); } while (0)
#define PSE_CELLS_PK(L, T, D) do { if ((L) && f64) PSE_CELLS_PK_F(L, T, D, (L)); else PSE_CELLS_PK_F(L, T, D, false); } while (0)
    if (dr.rm) {   // owned-particle ranks (table in LDS, no kept list, packed records): the two passes of pse_team_step_local
        if (list && two) PSE_CELLS_PK(true, true, true); else PSE_CELLS_PK(false, false, true);
        return;
    }
    if (pv && cl && !wr && vl_mode != VL_USE && (two || !list)) {   // the hot passes of a single GPU: packed (position, vector) records
        if (list) PSE_CELLS_PK(true, true, false); else PSE_CELLS_PK(false, false, false);
    } else if (list) {
        if (cl && two) { if (wr) PSE_CELLS(true, true, true, true); else PSE_CELLS(true, true, true, false); }
        else if (cl) { if (wr) PSE_CELLS(true, true, false, true); else PSE_CELLS(true, true, false, false); }
        else PSE_CELLS(true, false, false, false);
    } else if (cl) { if (wr) PSE_CELLS(false, true, false, true); else PSE_CELLS(false, true, false, false); }
    else PSE_CELLS(false, false, false, false);
#undef PSE_CELLS_PK
#undef PSE_CELLS
#undef PSE_CELLS_PK_F
#undef PSE_CELLS_F
    if (sums0 && list && two && cl)   // one partial per wavefront of the pass -> scal[LZ_TMP .. LZ_TMP + 2]
        launch_lz_reduce(sums0, (int)g.x * (TPB / 64), sums0_cap, 3, scal, nullptr, s);
}

int mreal_partials_needed(int rows) { return nblocks(std::max(rows, 1), 64); }   // one per 64 rows (the split mat-vec); the plain one uses a quarter
void launch_mreal_lanczos(const double4 *pos_s, VecIn vec, VecOut out, RowMap rm, const int *cell_off,
                          DBox box, DCells nc, double rcut, double self, const double *coef, NbList nb, LzFuse lz,
                          double *scal, hipEvent_t ev_begin, hipEvent_t ev_end, hipStream_t s, VerletList vl,
                          int sums, const int *stop, DevRowArgs dr, const void *vec_q, bool no_reduce) {
    // the kernel takes plain pointers and the two layouts as one launch-uniform word
    const double4 *vec_s = reinterpret_cast<const double4 *>(vec.p);
    double4 *w = reinterpret_cast<double4 *>(out.p);
    const int packed = (vec.packed ? 1 : 0) | (out.packed ? 2 : 0);
    const int rows = std::max(dr.rm ? dr.rows_cap : rm.list_rows(), 1);
    if (ev_begin) (void)hipEventRecord(ev_begin, s);
    // Four waves per block of 64 rows, each taking every fourth group of slots: 0.166 ms against 0.191 with four blocks of rows
    // per workgroup (two waves: 0.182, eight: 0.196).
    const int nb64 = nblocks(rows, 64);
#define PSE_LIST(F) hipLaunchKernelGGL((k_mreal_list<F, 4, 256, 4>), dim3(nb64), dim3(256), 0, s, pos_s, vec_s, w, rm, box, self, nb, lz, cell_off, nc, rcut * rcut, coef, vl, stop, dr, nullptr, packed)
#define PSE_LIST64(F) hipLaunchKernelGGL((k_mreal_list<F, 4, 256, 4, false, true>), dim3(nb64), dim3(256), 0, s, pos_s, vec_s, w, rm, box, self, nb, lz, cell_off, nc, rcut * rcut, coef, vl, stop, dr, nullptr, packed)
    if (nb.c64) {   // the fp64 operator: the neighbours' rows as doubles, the mirror vec_q is not read
        if (sums == 0) PSE_LIST64(0); else if (sums == 1) PSE_LIST64(1); else if (sums == 2) PSE_LIST64(2); else if (sums == 3) PSE_LIST64(3); else PSE_LIST64(4);
    } else if (sums == 1 && vec_q)
        hipLaunchKernelGGL((k_mreal_list<1, 4, 256, 4, true>), dim3(nb64), dim3(256), 0, s, pos_s, vec_s, w, rm, box, self, nb, lz, cell_off, nc, rcut * rcut, coef, vl, stop, dr,
                           (const vq4 *)vec_q, packed);
    else if (sums == 4 && vec_q)
        hipLaunchKernelGGL((k_mreal_list<4, 4, 256, 4, true>), dim3(nb64), dim3(256), 0, s, pos_s, vec_s, w, rm, box, self, nb, lz, cell_off, nc, rcut * rcut, coef, vl, stop, dr,
                           (const vq4 *)vec_q, packed);
    else if (sums == 0) PSE_LIST(0); else if (sums == 1) PSE_LIST(1); else if (sums == 2) PSE_LIST(2); else if (sums == 3) PSE_LIST(3); else PSE_LIST(4);
#undef PSE_LIST64
#undef PSE_LIST
    if (ev_end) (void)hipEventRecord(ev_end, s);
    if (no_reduce) return;   // (pse_debug_matvec_ms: the mat-vec kernel alone, back to back)
    if (sums == 4) launch_lz_reduce_split(lz.partials + lz.npart_cap, nb64, lz.upd, lz.n_upd, scal, stop, s);
    else if (sums >= 1) launch_lz_reduce(lz.partials, nb64, lz.npart_cap, sums == 1 ? 3 : (int)LZ_NGRAM, scal, stop, s);
}

__global__ void k_eval_fg(const double *__restrict__ r, int n, const double *__restrict__ coef, double *f, double *g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double ff, h;
    const double r2 = r[i] * r[i];
    eval_fg(r2, coef, ff, h);
    f[i] = ff;
    g[i] = ff + h * r2;
}
void launch_eval_fg(const double *r, int n, const double *coef, double *f, double *g, hipStream_t s) {
    hipLaunchKernelGGL(k_eval_fg, dim3(nblocks(n, TPB)), dim3(TPB), 0, s, r, n, coef, f, g);
}

}  // namespace pse
