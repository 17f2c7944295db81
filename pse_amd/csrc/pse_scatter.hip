// Intermediate scattering functions (pse_isf_sample, pse_isf_correlate; include/pse_amd.h): the self part F_s and the collective part
// F of the density correlations in time, on the integer modes of the box's reciprocal lattice.  Kernels only; the object and its
// entry points are in pse_objects.hip.  The densities rho_a(m) of a sample are those of the structure-factor pass (pse_analysis.hip),
// called as it is; what is new here is the self part.  gfx950, wave64, fp64.
#include "pse_scatter.h"

namespace pse {

// k_isf_planes: one lane per group member; s = (fma(-xy, y, x) / Lx, y / Ly, z / Lz) -- the bits k_sf_partial stages -- into the three
// planes of the current buffer, at the caller-order index.  An index >= n_max is skipped (nothing read, nothing written).
__global__ void __launch_bounds__(TPB)
k_isf_planes(const double4 *__restrict__ pos, const unsigned *__restrict__ group, int N, DBox box, double *__restrict__ planes, size_t n_max) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i >= N) return;
    const unsigned idx = group ? group[i] : (unsigned)i;
    if (idx >= n_max) return;
    const double4 p = pos[idx];
    planes[idx] = fma(-box.xy, p.y, p.x) / box.Lx;
    planes[n_max + idx] = p.y / box.Ly;
    planes[2 * n_max + idx] = p.z / box.Lz;
}

// Self part: self_a(m; pair) = sum over the members j of type a of exp(-2 pi i m.(s_j(now) - s_j(slot))): N x nk x npairs unit phasors.
// k_isf_self.  An ITEM is a (pair, segment) -- the segments are those of the structure-factor plan (structure_factor_plan):
// arithmetic progressions m0 + t d of len <= SF_RUN distinct modes --, the items are ordered pair-major, a LANE owns an item and keeps
// its R complex sums in registers; a workgroup is ONE wave, 64 consecutive items (a tile), which belong to npw <= 64 consecutive
// pairs, and walks a span of particles -- row `row` of the workspace -- in chunks of C = ISF_STAGE / npw particles: the lanes stage
// ds_c = s_c(now) - s_c(slot), one subtraction per component, for every (pair of the wave, particle of the chunk) in LDS, the
// particles of pair k at k (C | 1) so that lanes of different pairs read different banks, and the type of every particle; then all lanes walk the chunk together.  The
// particle index is wave-uniform, a lane reads the ds of its own pair, and there is NO reduction across lanes: the sum of a
// (pair, mode) is formed by one lane in particle order.  Per particle and item: f_c = fma(m_c, ds_c, -rint(m_c ds_c)) takes the
// integer part off every product exactly, t = (f_x + f_y) + f_z, t -= rint(t), sincospi(-2 t) is the seed; the same for the step d;
// then R - 1 complex multiplications (isf_phase and the loop are sf_phase and the loop of k_sf_partial).  Nothing takes sin or cos of a large argument; no images, no unwrapping:
// a particle that wrapped by a lattice vector changed ds by integers, which the reduction removes.
// Types: as k_sf_partial -- the pass runs once per type over the span and skips the particles of the other types by a wave-uniform
// branch on a byte from LDS, restaging the chunks per type.  A caller index >= n_max is staged as type 255 and never counts.
// Row (row, pair, a) of the workspace, one complex number per distinct mode at its canonical position, is written whole, zeros
// for a type that is absent: the finish reads no stale word.  The segments of more than SF_SHORT modes and the short ones are two
// launches (R = SF_RUN and R = SF_SHORT), as for the structure factor.  Two barriers per chunk; no lane leaves before a barrier: a
// lane past the last item walks a segment of len 0 of the wave's first pair and writes nothing.
// k_isf_self_finish: one wave per (pair, type, distinct mode); lane l of 64 adds the rows l, l + 64, ... in ascending order from
// +0.0, re and im apart, the wave adds its lanes with the xor butterfly (every lane adds the lane l xor o, o = 32, 16, ..., 1), lane
// 0 adds the sum to self at every caller position of the mode (perm[uoff[u]] ...: a mode listed twice has the same bits in both
// places).  No floating-point atomics: equal inputs give equal bits.
constexpr int ISF_TILE = 64;      // items per workgroup of k_isf_self: one wave
constexpr int ISF_STAGE = 192;    // (pair, particle) entries staged per barrier pair
constexpr int ISF_LDS = ISF_STAGE + ISF_MAX_PAIRS;   // npw (C | 1) <= ISF_STAGE + npw: 6 KB of LDS for the three components
__device__ __forceinline__ void isf_phase(double mx, double my, double mz, double sx, double sy, double sz, double &c, double &s) {
    const double fx = fma(mx, sx, -rint(mx * sx)), fy = fma(my, sy, -rint(my * sy)), fz = fma(mz, sz, -rint(mz * sz));
    double t = fx + fy + fz;
    t -= rint(t);
    sincospi(-2.0 * t, &s, &c);   // exp(-2 pi i t)
}
template <int R>
__global__ void __launch_bounds__(ISF_TILE)
k_isf_self(const double *__restrict__ cur, const double *__restrict__ slots, size_t n_max, size_t buf, const unsigned *__restrict__ group, int N,
           const unsigned char *__restrict__ types, unsigned ntyped, int ntypes, const int4 *__restrict__ segs, int nseg, int ntiles, int span,
           int nu, ScatterPairs pairs, double2 *__restrict__ part /* [nrows][npairs][ntypes][nu] */) {
    __shared__ double dsx[ISF_LDS], dsy[ISF_LDS], dsz[ISF_LDS];
    __shared__ unsigned char st[ISF_STAGE];
    const int lane = threadIdx.x, tile = blockIdx.x % ntiles, row = blockIdx.x / ntiles;
    const int nitem = pairs.npairs * nseg, item = tile * ISF_TILE + lane;
    const int p_lo = tile * ISF_TILE / nseg, p_hi = min(nitem - 1, tile * ISF_TILE + ISF_TILE - 1) / nseg;   // the pairs of the wave
    const int npw = p_hi - p_lo + 1, C = ISF_STAGE / npw, stride = C | 1;
    int pr = p_lo;
    int4 a0 = make_int4(0, 0, 0, 0), a1 = make_int4(0, 0, 0, 0);
    if (item < nitem) {
        pr = item / nseg;
        const int seg = item - pr * nseg;
        a0 = segs[2 * seg]; a1 = segs[2 * seg + 1];
    }
    const double mx = a0.x, my = a0.y, mz = a0.z, dx = a1.x, dy = a1.y, dz = a1.z;
    const int len = a0.w, first = a1.w, mine = (pr - p_lo) * stride;
    const long jb = (long)row * span, je = min((long)N, jb + span);
    for (int a = 0; a < ntypes; ++a) {
        double re[R], im[R];
#pragma unroll
        for (int t = 0; t < R; ++t) re[t] = im[t] = 0.0;
        for (long base = jb; base < je; base += C) {
            const int cnt = (int)min((long)C, je - base);
            __syncthreads();   // the walk of the chunk before is over
            for (int e = lane; e < npw * cnt; e += ISF_TILE) {
                const int k = e / cnt, q = e - k * cnt;
                const unsigned idx = group ? group[base + q] : (unsigned)(base + q);
                const bool in = idx < n_max;
                double x = 0.0, y = 0.0, z = 0.0;
                if (in) {
                    const double *__restrict__ now = cur + idx, *__restrict__ org = slots + (size_t)pairs.slot[p_lo + k] * buf + idx;
                    x = now[0] - org[0]; y = now[n_max] - org[n_max]; z = now[2 * n_max] - org[2 * n_max];
                }
                dsx[k * stride + q] = x; dsy[k * stride + q] = y; dsz[k * stride + q] = z;
                if (k == 0) st[q] = in ? (idx < ntyped ? types[idx] : (unsigned char)0) : (unsigned char)255;
            }
            __syncthreads();
            for (int q = 0; q < cnt; ++q) {
                if (__builtin_amdgcn_readfirstlane((int)st[q]) != a) continue;   // (wave-uniform: a scalar branch)
                const double x = dsx[mine + q], y = dsy[mine + q], z = dsz[mine + q];
                double cr, ci, wr, wi;
                isf_phase(mx, my, mz, x, y, z, cr, ci);
                isf_phase(dx, dy, dz, x, y, z, wr, wi);
#pragma unroll
                for (int t = 0; t < R; ++t) {
                    re[t] += cr; im[t] += ci;
                    const double nr = cr * wr - ci * wi;
                    ci = cr * wi + ci * wr;
                    cr = nr;
                }
            }
        }
        double2 *__restrict__ out = part + (((size_t)row * pairs.npairs + pr) * ntypes + a) * nu + first;
#pragma unroll
        for (int t = 0; t < R; ++t)
            if (t < len) out[t] = make_double2(re[t], im[t]);
    }
}
__global__ void __launch_bounds__(TPB)
k_isf_self_finish(const double2 *__restrict__ part, int nrows, int ncol, int ntypes, int nu, int nk, const unsigned *__restrict__ perm,
                  const unsigned *__restrict__ uoff, ScatterPairs pairs, double *__restrict__ self) {
    const int c = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= ncol) return;   // (a whole wave)
    double x = 0.0, y = 0.0;
    for (int r = lane; r < nrows; r += 64) { const double2 v = part[(size_t)r * ncol + c]; x += v.x; y += v.y; }
    x = wave_sum(x); y = wave_sum(y);
    if (lane != 0) return;
    const int p = c / (ntypes * nu), a = (c - p * ntypes * nu) / nu, u = c - (p * ntypes + a) * nu;
    double *__restrict__ dst = self + 2 * ((size_t)pairs.row[p] * ntypes + a) * nk;
    for (unsigned e = uoff[u]; e < uoff[u + 1]; ++e) { dst[2 * (size_t)perm[e]] += x; dst[2 * (size_t)perm[e] + 1] += y; }
}

// Collective part: coll[((row ntypes + a) ntypes + b) nk + q] += re_a re_b + im_a im_b = Re(rho_a(m_q; now) conj rho_b(m_q; slot)), from
// the rho of the current buffer and of the slot (the bits the structure-factor pass wrote: a mode listed twice has the same rho in
// both places, so the same product).  One thread per (pair, a, b, q); the rows of a call are distinct: no two threads share a word.
__global__ void __launch_bounds__(TPB)
k_isf_coll(const double *__restrict__ cur_rho, const double *__restrict__ slot_rho /* of slot 0 */, size_t buf, int ntypes, int nk,
           ScatterPairs pairs, double *__restrict__ coll) {
    const long t = (long)blockIdx.x * TPB + threadIdx.x, per = (long)ntypes * ntypes * nk;
    if (t >= pairs.npairs * per) return;
    const int p = (int)(t / per);
    const long r = t - p * per;
    const int a = (int)(r / ((long)ntypes * nk)), b = (int)((r - (long)a * ntypes * nk) / nk), q = (int)(r - ((long)a * ntypes + b) * nk);
    const double *__restrict__ now = cur_rho + 2 * ((size_t)a * nk + q);
    const double *__restrict__ org = slot_rho + (size_t)pairs.slot[p] * buf + 2 * ((size_t)b * nk + q);
    coll[(size_t)pairs.row[p] * per + r] += now[0] * org[0] + now[1] * org[1];
}

// The span of the self pass, by the rule of sf_span: a multiple of ISF_UNIT, the smallest with which one complex number per (span,
// listed pair, type, mode) -- for ISF_MAX_PAIRS pairs, whatever the number of slots: a slot may be listed for several rows -- stays
// within 2^24 complex numbers = 256 MB (at least 8 rows fit: ntypes nk <= 2^15)
int isf_span(unsigned n_max, int ntypes, int nk) {
    const long units = nblocks((long)n_max, ISF_UNIT);
    const long per = ((long)1 << 24) / ((long)ISF_MAX_PAIRS * ntypes * nk);
    return (int)(ISF_UNIT * ((units + per - 1) / per));
}
size_t isf_workspace(unsigned n_max, int ntypes, int nk) {
    return (size_t)nblocks((long)n_max, isf_span(n_max, ntypes, nk)) * ISF_MAX_PAIRS * ntypes * nk;
}
void launch_isf_sample(const double4 *pos, const unsigned *group, int N, DBox box, const Scatter &sc, double *static_sums, hipStream_t s) {
    hipLaunchKernelGGL(k_isf_planes, dim3(nblocks(N, TPB)), dim3(TPB), 0, s, pos, group, N, box, sc.cur, sc.n_max);
    launch_structure_factor(pos, group, N, box, sc.sf, sc.cur + 3 * sc.n_max, static_sums, s);
}
void launch_isf_self(const Scatter &sc, const unsigned *group, int N, const ScatterPairs &pairs, double *self, hipStream_t s) {
    static_assert(ISF_TILE == 64 && ISF_STAGE >= ISF_MAX_PAIRS, "a workgroup of k_isf_self is one wave, and a chunk holds a particle of each of its pairs");
    const StructureFactor &sf = sc.sf;
    const int nrows = nblocks(N, sc.span), nshort = sf.nseg - sf.nlong;
    if (sf.nlong) {
        const int ntiles = nblocks((long)pairs.npairs * sf.nlong, ISF_TILE);
        hipLaunchKernelGGL(k_isf_self<SF_RUN>, dim3((unsigned)(nrows * ntiles)), dim3(ISF_TILE), 0, s, sc.cur, sc.slots, sc.n_max, sc.buf, group, N,
                           sf.types, sf.n, sf.ntypes, sf.segs, sf.nlong, ntiles, sc.span, sf.nu, pairs, sc.part);
    }
    if (nshort) {
        const int ntiles = nblocks((long)pairs.npairs * nshort, ISF_TILE);
        hipLaunchKernelGGL(k_isf_self<SF_SHORT>, dim3((unsigned)(nrows * ntiles)), dim3(ISF_TILE), 0, s, sc.cur, sc.slots, sc.n_max, sc.buf, group,
                           N, sf.types, sf.n, sf.ntypes, sf.segs + 2 * sf.nlong, nshort, ntiles, sc.span, sf.nu, pairs, sc.part);
    }
    const int ncol = pairs.npairs * sf.ntypes * sf.nu;
    hipLaunchKernelGGL(k_isf_self_finish, dim3(nblocks(ncol, TPB / 64)), dim3(TPB), 0, s, sc.part, nrows, ncol, sf.ntypes, sf.nu, sf.nk, sf.perm,
                       sf.uoff, pairs, self);
}
void launch_isf_coll(const Scatter &sc, const ScatterPairs &pairs, double *coll, hipStream_t s) {
    const StructureFactor &sf = sc.sf;
    const long n = (long)pairs.npairs * sf.ntypes * sf.ntypes * sf.nk;
    hipLaunchKernelGGL(k_isf_coll, dim3(nblocks(n, TPB)), dim3(TPB), 0, s, sc.cur + 3 * sc.n_max, sc.slots + 3 * sc.n_max, sc.buf, sf.ntypes, sf.nk,
                       pairs, coll);
}

}  // namespace pse
