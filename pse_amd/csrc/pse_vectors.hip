// The vector kernels of the PSE engine for gfx950 (CDNA4, wave64): the particle noise (K14), the Lanczos iteration and its decision
// on the device (K10-K13), the sums and scatters of the velocity, the integrator (K15) and the copies of a team's exchanges.  Each
// kernel names the reference kernel it replaces.  All arithmetic is fp64.
#include "pse_vectors.h"

namespace pse {

// ------------------------------------------------------------------------------------------------ vectors
// K14 gpu_stokes_BrownianGenerate_kernel (PSEv1/Brownian.cu:99-130), keyed by the particle's global index
__global__ void k_psi(double4 *__restrict__ psi_s, const unsigned *__restrict__ tag_s, int N, uint32_t seed,
                      uint32_t timestep, CellRanges need, const int *__restrict__ cell_off) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= N || !need.row(s, cell_off)) return;
    uint32_t r[4];
    philox4x32(tag_s[s], 0u, timestep, DOMAIN_PARTICLE, seed, PHILOX_KEY1, r);
    const double q = 1.7320508075688772;  // sqrt(3): variance 1
    psi_s[s] = make_double4(uniform_pm(r[0], q), uniform_pm(r[1], q), uniform_pm(r[2], q), 0.0);
}
void launch_psi(double4 *psi_s, const unsigned *tag_s, int N, uint32_t seed, uint32_t timestep, hipStream_t s, CellRanges need,
                const int *cell_off) {
    hipLaunchKernelGGL(k_psi, dim3(nblocks(N, TPB)), dim3(TPB), 0, s, psi_s, tag_s, N, seed, timestep, need, cell_off);
}

static inline int vec_grid(int N) { return std::min(LZ_NPART, std::max(1, nblocks(N, TPB))); }

// Lanczos (PSEv1/Brownian.cu:440-521) with device-resident scalars: no host round trip inside an iteration.
// ---- Lanczos iteration (PSEv1/Brownian.cu:440-521) with deferred normalisation --------------------------------------
// Each rank owns rows [lo, hi) of every vector (a single GPU owns them all).  The mat-vec runs on the UNNORMALISED vector
// x_j (v_j = x_j / beta_j, beta_j = |x_j|): with y = M x_j the three sums  s1 = x_j.x_j, s2 = x_j.y, s3 = x_j.x_{j-1}
// give  beta_j = sqrt(s1)  and  alpha_j = v_j.(M v_j - beta_j v_{j-1}) = s2/s1 - s3/beta_{j-1}  -- the reference's K10-K12
// sequence (w = M v - beta v_prev; alpha = v.w; w -= alpha v; beta' = |w|) with ONE reduction per iteration (one 3-scalar
// all-reduce when sharded) and one vector pass: x_{j+1} = (y - alpha_j x_j)/beta_j - (beta_j/beta_{j-1}) x_{j-1}.
// The normalised v_j are never stored (round 3): the basis keeps the x_j and the final combination divides by beta_j -- one
// 32-byte write per row and iteration less.  beta_0 = |psi| is the norm the result is rescaled with (Brownian.cu:440-452,739).
__global__ void __launch_bounds__(TPB)
k_lz_dots(const double4 *__restrict__ x, const double4 *__restrict__ y, const double4 *__restrict__ vprev, int lo, int hi,
          double *__restrict__ partials, int cap) {
    __shared__ double sh[4];
    double a = 0.0, b = 0.0, c = 0.0;
    for (int i = lo + blockIdx.x * TPB + threadIdx.x; i < hi; i += gridDim.x * TPB) {
        const double4 p = x[i];
        a += p.x * p.x + p.y * p.y + p.z * p.z;
        if (y) { const double4 q = y[i]; b += p.x * q.x + p.y * q.y + p.z * q.z; }
        if (vprev) { const double4 m = vprev[i]; c += p.x * m.x + p.y * m.y + p.z * m.z; }
    }
    a = block_sum(a, sh);
    __syncthreads();
    b = block_sum(b, sh);
    __syncthreads();
    c = block_sum(c, sh);
    if (threadIdx.x == 0) { partials[blockIdx.x] = a; partials[cap + blockIdx.x] = b; partials[2 * cap + blockIdx.x] = c; }
}
// this rank's partial sums -> scal[LZ_TMP .. LZ_TMP + nsum) (then all-reduced over the ranks)
// upd (nullable; then nsum = 3 and `partials` holds sum 1 alone): sums 0 and 2 are those of upd[0 .. n_upd) and
// upd[LZ_NPART .. LZ_NPART + n_upd), the partials the k_lz_update that wrote the vector left (launch_lz_reduce_split)
__global__ void __launch_bounds__(1024)
k_lz_reduce(const double *__restrict__ partials, int npart, int cap, int nsum, double *__restrict__ scal, const int *__restrict__ stop,
            const double *__restrict__ upd, int n_upd) {
    if (stop && *stop) return;
    __shared__ double sh[16];
    const int q = blockIdx.x;                         // one workgroup per sum, fixed summation order
    const double *p = partials + (size_t)q * cap;
    if (upd) { p = q == 1 ? partials : upd + (q == 2 ? LZ_NPART : 0); if (q != 1) npart = n_upd; }
    double v = 0.0;
    for (int i = threadIdx.x; i < npart; i += 1024) v += p[i];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += sh[w];
        scal[LZ_TMP + q] = t;
    }
}
void launch_lz_reduce(const double *partials, int npart, int cap, int nsum, double *scal, const int *stop, hipStream_t s) {
    hipLaunchKernelGGL(k_lz_reduce, dim3(nsum), dim3(1024), 0, s, partials, npart, cap, nsum, scal, stop, (const double *)nullptr, 0);
}
void launch_lz_reduce_split(const double *xy, int n_xy, const double *upd, int n_upd, double *scal, const int *stop, hipStream_t s) {
    hipLaunchKernelGGL(k_lz_reduce, dim3(3), dim3(1024), 0, s, xy, n_xy, 0, 3, scal, stop, upd, n_upd);
}
// alpha_j, beta_j from the reduced sums; x_{j+1} on the given rows, and (next_sums) what it contributes to two sums of iteration j + 1
__global__ void __launch_bounds__(TPB)
k_lz_update(VecIn xin, VecIn y, VecIn xprev, VecOut xnext, int j, double *__restrict__ scal, RowRanges rg,
            const double *__restrict__ sums_all, int nranks, double *__restrict__ sch, const int *__restrict__ stop, vq4 *__restrict__ xq,
            double *__restrict__ next_sums) {
    if (stop && *stop) return;
    // the three sums: this GPU's (single GPU), or the ranks' partial sums added in rank order -- every rank holds all of them
    // (they travel with the ghost rows: no separate all-reduce) and adds them in the same order: identical scalars everywhere
    double s1 = 0.0, s2 = 0.0, s3raw = 0.0;
    if (nranks > 0) for (int r = 0; r < nranks; ++r) { s1 += sums_all[r * LZ_NGRAM]; s2 += sums_all[r * LZ_NGRAM + 1]; s3raw += sums_all[r * LZ_NGRAM + 2]; }
    else { s1 = scal[LZ_TMP]; s2 = scal[LZ_TMP + 1]; s3raw = scal[LZ_TMP + 2]; }
    const double bprev = j == 1 ? scal[LZ_NORM] : (j > 1 ? scal[LZ_BETA + j - 1] : 0.0);   // |x_{j-1}|
    const double ibprev = bprev > 0.0 ? 1.0 / bprev : 0.0;
    const double beta = s1 > 0.0 ? sqrt(s1) : 0.0;
    const double inv = beta > 0.0 ? 1.0 / beta : 0.0;
    const double alpha = s1 > 0.0 ? s2 / s1 - s3raw * ibprev : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        scal[LZ_ALPHA + j] = alpha;
        if (j == 0) { scal[LZ_NORM] = beta; scal[LZ_BETA] = 0.0; } else scal[LZ_BETA + j] = beta;
        if (sch) {   // the host's copy (mapped pinned memory): what the convergence check reads -- no device-to-host copy is queued
            sch[LZ_ALPHA + j] = alpha;
            if (j == 0) { sch[LZ_NORM] = beta; sch[LZ_BETA] = 0.0; } else sch[LZ_BETA + j] = beta;
        }
    }
    const double cp = beta * ibprev;   // beta_j / beta_{j-1}
    const int n0 = rg.hi[0] - rg.lo[0], n1 = rg.n > 1 ? rg.hi[1] - rg.lo[1] : 0, n2 = rg.n > 2 ? rg.hi[2] - rg.lo[2] : 0;
    double nn = 0.0, np = 0.0;   // x_{j+1}.x_{j+1} and x_{j+1}.x_j over this thread's rows: two of the three sums of iteration j + 1
    for (int t = blockIdx.x * TPB + threadIdx.x; t < n0 + n1 + n2; t += gridDim.x * TPB) {
        const int i = t < n0 ? rg.lo[0] + t : (t < n0 + n1 ? rg.lo[1] + (t - n0) : rg.lo[2] + (t - n0 - n1));
        double3 p, q;   // (each array in its own layout, uniform over the launch: psi and the build pass's M psi are double4)
        row_load(xin, i, p.x, p.y, p.z); row_load(y, i, q.x, q.y, q.z);
        double nx = (q.x - alpha * p.x) * inv, ny = (q.y - alpha * p.y) * inv, nz = (q.z - alpha * p.z) * inv;
        if (xprev.p) { double3 m; row_load(xprev, i, m.x, m.y, m.z); nx -= cp * m.x; ny -= cp * m.y; nz -= cp * m.z; }
        row_store(xnext, i, nx, ny, nz);
        if (xq) xq[i] = vq_pack(nx, ny, nz);   // the 16-byte mirror the next pair-list mat-vec gathers its neighbours from
        nn += nx * nx + ny * ny + nz * nz;
        np += nx * p.x + ny * p.y + nz * p.z;
    }
    if (next_sums) {   // (uniform over the launch) one pair per workgroup, both through LDS in one pass
        __shared__ double sh[2][4];
        nn = wave_sum(nn); np = wave_sum(np);
        if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = nn; sh[1][threadIdx.x >> 6] = np; }
        __syncthreads();
        if (threadIdx.x == 0) {
            next_sums[blockIdx.x] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
            next_sums[LZ_NPART + blockIdx.x] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
        }
    }
}
// ---- two Lanczos iterations per exchange (teams) ---------------------------------------------------------------------------
// A slab rank pays one exchange (an all-reduce of the sums + the ghost rows of the mat-vec results) per Lanczos iteration, and at
// 1/8 of the rows an exchange costs as much as the mat-vec.  The two-step block needs ONE per two iterations: with q = v_j,
// p = v_{j-1}, u = M p known on the own rows and TWO ghost cell layers,
//     w1 = M q   on the own rows and one ghost layer (redundantly: the neighbours compute those rows too),
//     w2 = M w1  on the own rows,
// the Gram sums of {p, q, u, w1, w2} over the own rows (one all-reduce of LZ_NGRAM numbers) give alpha_j, beta_{j+1}, alpha_{j+1},
// beta_{j+2} in closed form (M is symmetric: q.w2 = w1.w1, p.w2 = u.w1, ...; every product is summed explicitly all the same):
//     r1 = w1 - alpha q - beta p,            beta'^2 = w1.w1 - alpha^2 - 2 beta p.w1 + beta^2,        v' = r1 / beta'
//     z1 = M v' = (w2 - alpha w1 - beta u) / beta',   alpha' = v'.z1,
//     r2 = z1 - alpha' v' - beta' q,         beta''^2 = z1.z1 - alpha'^2 - 2 beta' q.z1 + beta'^2,    v'' = r2 / beta''
// and with the ghost rows of w1, w2 (the same exchange) every rank forms v', v'', z1 on its own AND its ghost rows -- the state
// of the next block (p = v', q = v'', u = z1).  In exact arithmetic these are the alpha, beta of PSEv1/Brownian.cu:440-521; the
// sums cost a relative 1e-14 in beta (cancellation against O(1) terms).  q of block 0 is psi unnormalised: s = 1 / |q| from q.q.
// The basis V holds the NORMALISED v_j here (the one-step path keeps unnormalised x_j).
template <bool FULL>
__global__ void __launch_bounds__(TPB)
k_lz_block(LzBlockArgs a, double *__restrict__ scal, RowRanges rg, const double *__restrict__ sums_all, int nranks, double *__restrict__ sch,
           const RowRanges *__restrict__ rg_dev, int vectors_off, const int *__restrict__ stop) {
    if (stop && *stop) return;
    if (rg_dev) { rg = *rg_dev; if (vectors_off) rg.n = 0; }   // an owned-particle rank: the ranges are known on the device only
    __shared__ double sG[LZ_NGRAM];   // the ranks' partial sums added in rank order (they came with the ghost rows: see k_lz_update):
    if (threadIdx.x < LZ_NGRAM) {     // one lane per sum, once per workgroup
        double v = 0.0;
        for (int r = 0; r < nranks; ++r) v += sums_all[r * LZ_NGRAM + threadIdx.x];
        sG[threadIdx.x] = nranks > 0 ? v : scal[LZ_TMP + threadIdx.x];
    }
    __syncthreads();
    double G[LZ_NGRAM];
#pragma unroll
    for (int t = 0; t < LZ_NGRAM; ++t) G[t] = sG[t];
    const int j = a.j;
    const double n0 = G[LZG_QQ], s2 = n0 > 0.0 ? 1.0 / n0 : 0.0, sc = sqrt(s2);
    const double beta = j > 0 ? scal[LZ_BETA + j] : 0.0, alpha_prev = j > 0 ? scal[LZ_ALPHA + j - 1] : 0.0;
    const double ga = G[LZG_QW1] * s2, gb = G[LZG_W1W1] * s2, gf = G[LZG_PW1] * sc;   // q.w1, w1.w1, p.w1 (= q.u) of the normalised q
    const double alpha = ga;
    const double bp2 = gb - alpha * alpha - 2.0 * beta * gf + beta * beta;
    const double bp = bp2 > 0.0 ? sqrt(bp2) : 0.0, ibp = bp > 1e-12 ? 1.0 / bp : 0.0;
    double alpha1 = 0.0, bpp = 0.0, ibpp = 0.0, uu_next = 0.0;
    if (FULL) {
        const double gc = G[LZG_W1W2] * s2, gd = G[LZG_W2W2] * s2, ge = gb /* q.w2 = w1.w1 */, gg = G[LZG_PW2] * sc, gg2 = gg /* u.w1 = p.w2 */,
                     gh = G[LZG_UW2] * sc, gk = j > 0 ? scal[LZ_UU + j] : 0.0, gf2 = gf /* q.u = p.w1 */;
        const double r1w2 = gc - alpha * ge - beta * gg, r1w1 = gb - alpha * ga - beta * gf, r1u = gg2 - alpha * gf2 - beta * alpha_prev;
        alpha1 = (r1w2 - alpha * r1w1 - beta * r1u) * ibp * ibp;
        const double zz = (gd + alpha * alpha * gb + beta * beta * gk - 2.0 * alpha * gc - 2.0 * beta * gh + 2.0 * alpha * beta * gg2) * ibp * ibp;
        const double qz = (ge - alpha * ga - beta * gf2) * ibp;
        const double bpp2 = zz - alpha1 * alpha1 - 2.0 * bp * qz + bp * bp;
        bpp = bpp2 > 0.0 ? sqrt(bpp2) : 0.0;
        ibpp = bpp > 1e-12 ? 1.0 / bpp : 0.0;
        uu_next = zz;                              // |M v_{j+1}|^2: the u.u of the block that starts at j + 2
    } else {
        uu_next = gb;                              // a single step leaves u = M v_j = w1
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (j == 0) { scal[LZ_NORM] = n0 > 0.0 ? sqrt(n0) : 0.0; scal[LZ_BETA] = 0.0; }
        scal[LZ_ALPHA + j] = alpha;
        scal[LZ_BETA + j + 1] = bp;
        if (FULL) { scal[LZ_ALPHA + j + 1] = alpha1; scal[LZ_BETA + j + 2] = bpp; }
        scal[LZ_UU + j + (FULL ? 2 : 1)] = uu_next;   // another slot than the one this launch reads
        if (sch) {   // the host's copy (mapped pinned memory)
            if (j == 0) { sch[LZ_NORM] = n0 > 0.0 ? sqrt(n0) : 0.0; sch[LZ_BETA] = 0.0; }
            sch[LZ_ALPHA + j] = alpha;
            sch[LZ_BETA + j + 1] = bp;
            if (FULL) { sch[LZ_ALPHA + j + 1] = alpha1; sch[LZ_BETA + j + 2] = bpp; }
        }
    }
    const int n0r = rg.n > 0 ? rg.hi[0] - rg.lo[0] : 0, n1r = rg.n > 1 ? rg.hi[1] - rg.lo[1] : 0, n2r = rg.n > 2 ? rg.hi[2] - rg.lo[2] : 0;
    for (int t = blockIdx.x * TPB + threadIdx.x; t < n0r + n1r + n2r; t += gridDim.x * TPB) {
        const int i = t < n0r ? rg.lo[0] + t : (t < n0r + n1r ? rg.lo[1] + (t - n0r) : rg.lo[2] + (t - n0r - n1r));
        const double4 q = a.q[i], w1 = a.w1[i];
        double4 p = make_double4(0.0, 0.0, 0.0, 0.0), u = p;
        if (j > 0) { p = a.p[i]; if (FULL) u = a.u[i]; }
        const double qx = sc * q.x, qy = sc * q.y, qz_ = sc * q.z, ax = sc * w1.x, ay = sc * w1.y, az = sc * w1.z;
        const double v1x = (ax - alpha * qx - beta * p.x) * ibp, v1y = (ay - alpha * qy - beta * p.y) * ibp, v1z = (az - alpha * qz_ - beta * p.z) * ibp;
        a.v1[i] = make_double4(v1x, v1y, v1z, 0.0);
        double nx = v1x, ny = v1y, nz = v1z;
        if (FULL) {
            const double4 w2 = a.w2[i];
            const double z1x = (sc * w2.x - alpha * ax - beta * u.x) * ibp, z1y = (sc * w2.y - alpha * ay - beta * u.y) * ibp,
                         z1z = (sc * w2.z - alpha * az - beta * u.z) * ibp;
            nx = (z1x - alpha1 * v1x - bp * qx) * ibpp; ny = (z1y - alpha1 * v1y - bp * qy) * ibpp; nz = (z1z - alpha1 * v1z - bp * qz_) * ibpp;
            a.v2[i] = make_double4(nx, ny, nz, 0.0);
            a.u[i] = make_double4(z1x, z1y, z1z, 0.0);
        } else {
            a.u[i] = make_double4(ax, ay, az, 0.0);   // M v_j: the u of a block that starts at j + 1
        }
    }
}
void launch_lz_block(const LzBlockArgs &a, bool full, double *scal, const int (*rg)[2], int nrg, hipStream_t s, const double *sums_all, int nranks, double *sch,
                     const RowRanges *rg_dev, int rows_cap, bool vectors_off, const int *stop) {
    RowRanges r{};
    r.n = nrg;
    int total = 0;
    for (int q = 0; q < nrg && q < 3; ++q) { r.lo[q] = rg[q][0]; r.hi[q] = rg[q][1]; total += rg[q][1] - rg[q][0]; }
    if (rg_dev) total = vectors_off ? 1 : rows_cap;
    const dim3 g(vec_grid(std::max(1, total)));
    if (full) hipLaunchKernelGGL(k_lz_block<true>, g, dim3(TPB), 0, s, a, scal, r, sums_all, nranks, sch, rg_dev, vectors_off ? 1 : 0, stop);
    else hipLaunchKernelGGL(k_lz_block<false>, g, dim3(TPB), 0, s, a, scal, r, sums_all, nranks, sch, rg_dev, vectors_off ? 1 : 0, stop);
}


// ---- the Lanczos decision on the device (LzState / LzDecide in pse_vectors.h) ------------------------------------------------------
// One wavefront: eigen-decomposition of the m x m tridiagonal (alpha[0..m), beta[1..m)) by implicit QL with Wilkinson shifts -- the
// algorithm of tridiag_eigen (pse_params.cpp; it replaces LAPACKE_spteqr, PSEv1/Brownian.cu:540), statement by statement -- and
// t = Z sqrt(Lambda) Z^T e_1 (PSEv1/Brownian.cu:563-582).  The scalar recurrence runs redundantly in every lane (identical values);
// lane 0 stores d and e; row k of the eigenvector matrix belongs to lane k mod 64 (columns in LDS, stride m).  m <= 2 x 64.
__device__ __forceinline__ void lz_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// d and e live in REGISTERS, entry i in lane i mod 64 of one of two registers (m <= 128): the recurrence reads them with v_readlane
// at a wave-uniform index and the owning lane stores -- no LDS round trip on the serial chain (with d, e in LDS the decision of
// sizes 6 and 7 took 21 us, most of it waiting for ds_read).  Only the eigenvector columns are in LDS; their update is off the chain.
struct LzReg {
    double lo, hi;   // entries lane and 64 + lane
    __device__ __forceinline__ double get(int i) const {   // ALL lanes of the wave must be running: the select below is a vector instruction
        const double v = i < 64 ? lo : hi;
        const int l = i & 63;
        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
    }
    __device__ __forceinline__ void set(int i, double v) {
        const int lane = threadIdx.x & 63;
        if (lane == (i & 63)) { if (i < 64) lo = v; else hi = v; }
    }
};
__device__ bool lz_sqrt_e1(int m, const double *__restrict__ alpha, const double *__restrict__ beta, double *z, double *t_out) {
    const int lane = threadIdx.x & 63;
    LzReg d, e;
    d.lo = lane < m ? alpha[lane] : 0.0; d.hi = lane + 64 < m ? alpha[lane + 64] : 0.0;
    e.lo = lane + 1 < m ? beta[lane + 1] : 0.0; e.hi = lane + 65 < m ? beta[lane + 65] : 0.0;
    for (int c = 0; c < m; ++c)
        for (int k = lane; k < m; k += 64) z[c * m + k] = c == k ? 1.0 : 0.0;
    bool ok = true;
    for (int l = 0; l < m && ok; ++l) {
        int iter = 0, mm;
        do {
            for (mm = l; mm < m - 1; ++mm) {
                const double dd = fabs(d.get(mm)) + fabs(d.get(mm + 1));
                if (fabs(e.get(mm)) <= 2.3e-16 * dd) break;
            }
            if (mm != l) {
                if (iter++ == 200) { ok = false; break; }
                const double dl = d.get(l), el = e.get(l);
                double g = (d.get(l + 1) - dl) / (2.0 * el);
                double r = sqrt(g * g + 1.0);
                g = d.get(mm) - dl + el / (g + (g >= 0 ? r : -r));
                double s = 1.0, c = 1.0, p = 0.0;
                int i;
                for (i = mm - 1; i >= l; --i) {
                    const double ei = e.get(i);
                    double f = s * ei, b = c * ei;
                    r = sqrt(f * f + g * g);
                    e.set(i + 1, r);
                    if (r == 0.0) { d.set(i + 1, d.get(i + 1) - p); e.set(mm, 0.0); break; }
                    const double ir = 1.0 / r;
                    s = f * ir; c = g * ir;
                    g = d.get(i + 1) - p;
                    r = (d.get(i) - g) * s + 2.0 * c * b;
                    p = s * r;
                    d.set(i + 1, g + p);
                    g = c * r - b;
                    for (int k = lane; k < m; k += 64) {
                        const double zk1 = z[(i + 1) * m + k], zk0 = z[i * m + k];
                        z[(i + 1) * m + k] = s * zk0 + c * zk1;
                        z[i * m + k] = c * zk0 - s * zk1;
                    }
                }
                if (r == 0.0 && i >= l) continue;
                d.set(l, d.get(l) - p); e.set(l, g); e.set(mm, 0.0);
            }
        } while (mm != l);
    }
    lz_wave_sync();
    if (!ok) return false;
    // The trip count is the WAVE's, not the lane's: d.get selects lo or hi with a vector instruction before it reads the owning lane,
    // so every lane must be running where it is called.  (With `for (i = lane; i < m; i += 64)` the second pass of a size above 64
    // ran on lanes 0 .. m - 65 alone and d.get(j) returned, for every j whose lane sat the pass out, what that lane's copy of the
    // selected register held from the pass before: t[64 ..] of every size above 64 was wrong by about its own magnitude.)
    for (int i0 = 0; i0 < m; i0 += 64) {
        const int i = i0 + lane;
        double t = 0.0;
        for (int j = 0; j < m; ++j) {
            const double w = sqrt(fmax(d.get(j), 0.0)) * z[j * m];
            if (i < m) t += z[j * m + i] * w;
        }
        if (i < m) t_out[i] = t;
    }
    lz_wave_sync();
    return true;
}
__global__ void __launch_bounds__(128)
k_lz_decide(LzDecide a, double *__restrict__ scal, LzState *__restrict__ st, double *__restrict__ sch, double seq) {
    extern __shared__ double lds[];
    __shared__ double tbuf[2][104];
    __shared__ int okf[2];
    if (a.first) { if (threadIdx.x == 0) { st->done = 0; st->m_final = 0; st->checked = 0; st->status = 0; st->stepnorm = 1.0; } }
    else if (st->done) return;
    __syncthreads();
    const int wv = threadIdx.x >> 6, nm = a.m_hi - a.m_lo + 1;
    const double *alpha = scal + LZ_ALPHA, *beta = scal + LZ_BETA;
    const double norm = scal[LZ_NORM];
    const bool dead = !(norm > 0.0) || !isfinite(norm);          // psi == 0: the result is zero
    if (wv < nm && !dead) {
        const int m = a.m_lo + wv;
        double *base = lds + (wv == 0 ? 0 : (size_t)a.m_lo * a.m_lo);
        const bool ok = lz_sqrt_e1(m, alpha, beta, base, tbuf[wv]);
        if ((threadIdx.x & 63) == 0) okf[wv] = ok ? 1 : 0;
    }
    // what the walk below reads, fetched by all lanes at once: thread 0 alone paid a dependent global round trip per coefficient
    // (alpha, beta, the previous size's t: ~20 of them in a row, a third of the kernel's 24-28 us)
    __shared__ double s_alpha[104], s_beta[104], s_prev[104];
    __shared__ int s_checked;
    __shared__ double s_stepnorm;
    for (int q = threadIdx.x; q <= min(a.m_hi, 103); q += blockDim.x) { s_alpha[q] = scal[LZ_ALPHA + q]; s_beta[q] = scal[LZ_BETA + q]; s_prev[q] = st->t_prev[q]; }
    if (threadIdx.x == 0) { s_checked = a.first ? 0 : st->checked; s_stepnorm = a.first ? 1.0 : st->stepnorm; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    alpha = s_alpha; beta = s_beta;
    int m_final = 0, status = 0, checked = s_checked;
    double stepnorm = s_stepnorm;
    const double *t_fin = nullptr;
    if (dead) { m_final = -1; }
    else if (a.pending_beta > 0 && beta[a.pending_beta] < 1e-8) {   // |x_m| of the vector the previous batch ended on: invariant subspace
        m_final = a.pending_beta; stepnorm = 0.0; t_fin = s_prev;
    } else {
        for (int w = 0; w < nm && !m_final; ++w) {               // walk m upward as the reference's while loop does (PSEv1/Brownian.cu:606-724)
            const int m = a.m_lo + w;
            const bool have_beta = m < a.done_iters || a.have_last_beta;
            if (!isfinite(alpha[m - 1]) || (have_beta && !isfinite(beta[m])) || !okf[w]) { m_final = max(checked, 1); status = 2; t_fin = checked ? s_prev : tbuf[w]; break; }
            const double *tc = tbuf[w];
            if (m < a.done_iters && beta[m] < 1e-8) { m_final = m; stepnorm = 0.0; t_fin = tc; break; }   // invariant subspace (Brownian.cu:503)
            if (checked == m - 1 && checked > 0) {
                double s2 = tc[m - 1] * tc[m - 1];
                for (int q = 0; q < m - 1; ++q) { const double dq = tc[q] - s_prev[q]; s2 += dq * dq; }
                stepnorm = sqrt(s2 / alpha[0]);                   // Brownian.cu:719-724; psi.M.psi / |psi|^2 = alpha_0
                if (stepnorm <= a.tol || m >= a.m_max) { m_final = m; t_fin = tc; break; }
            }
            if (a.have_last_beta && m == a.done_iters && beta[m] < 1e-8) { m_final = m; stepnorm = 0.0; t_fin = tc; break; }
            for (int q = 0; q < m; ++q) { st->t_prev[q] = tc[q]; s_prev[q] = tc[q]; }
            checked = m;
        }
        if (!m_final && (a.last || a.done_iters >= a.m_max)) {     // nothing more is queued: end with what there is
            m_final = checked; t_fin = s_prev; status = a.done_iters >= a.m_max ? 0 : 1;
        }
    }
    st->checked = checked;
    st->stepnorm = stepnorm;
    if (m_final) {
        const int m = max(m_final, 0);
        for (int q = 0; q < m; ++q) st->coef[q] = t_fin[q] / (q == 0 ? norm : (a.normalised ? 1.0 : beta[q]));
        st->m_final = m; st->status = status;
        st->done = 1;                                            // (read by LATER launches only: the kernel boundary orders it)
        if (sch) {
            sch[LZ_HOST_M] = (double)m; sch[LZ_HOST_STEPNORM] = stepnorm; sch[LZ_HOST_STATUS] = (double)status; sch[LZ_HOST_SEQ] = seq;
            if (status != 0) sch[LZ_HOST_OPEN] = sch[LZ_HOST_OPEN] + 1.0;   // (sticky: a loop that reads pse_info only now and then still learns of it)
        }
    }
}
static size_t lz_decide_lds(int m_lo, int m_hi) {
    size_t n = (size_t)m_lo * m_lo;
    if (m_hi != m_lo) n += (size_t)m_hi * m_hi;
    return n * sizeof(double);
}
bool lz_decide_supported(int m_hi) { return m_hi >= 1 && m_hi <= 100 && lz_decide_lds(std::max(1, m_hi - 1), m_hi) <= 150 * 1024; }
void launch_lz_decide(const LzDecide &d, double *scal, LzState *st, double *sch, double seq, hipStream_t s) {
    const size_t lds = lz_decide_lds(d.m_lo, d.m_hi);
    static LdsAttr attr;
    if (lds > 48 * 1024 && attr.need(150 * 1024)) (void)hipFuncSetAttribute((const void *)k_lz_decide, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    hipLaunchKernelGGL(k_lz_decide, dim3(1), dim3(128), lds, s, d, scal, st, sch, seq);
}

void launch_lz_dots(const double4 *x, const double4 *y, const double4 *vprev, int lo, int hi, double *partials, int cap,
                    double *scal, hipStream_t s) {
    const int g = vec_grid(std::max(1, hi - lo));
    hipLaunchKernelGGL(k_lz_dots, dim3(g), dim3(TPB), 0, s, x, y, vprev, lo, hi, partials, cap);
    launch_lz_reduce(partials, g, cap, y ? 3 : 1, scal, nullptr, s);
}
void launch_lz_update(VecIn xin, VecIn y, VecIn xprev, VecOut xnext, int j,
                      double *scal, const int (*rg)[2], int nrg, hipStream_t s, const double *sums_all, int nranks, double *sch,
                      const int *stop, void *xq, double *next_sums) {
    RowRanges r{};
    r.n = nrg;
    int total = 0;
    for (int q = 0; q < nrg && q < 3; ++q) { r.lo[q] = rg[q][0]; r.hi[q] = rg[q][1]; total += rg[q][1] - rg[q][0]; }
    if (total <= 0) next_sums = nullptr;   // scalars only: x_{j+1} is not formed; its sums come with the launch that forms it
    hipLaunchKernelGGL(k_lz_update, dim3(vec_grid(std::max(1, total))), dim3(TPB), 0, s, xin, y, xprev, xnext, j, scal, r, sums_all, nranks, sch, stop, (vq4 *)xq, next_sums);
}
int lz_update_grid(int rows) { return vec_grid(std::max(1, rows)); }
__global__ void k_vq_roundtrip(const double *__restrict__ in, double *__restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double x, y, z;
    vq_unpack(vq_pack(in[3 * i], in[3 * i + 1], in[3 * i + 2]), x, y, z);
    out[3 * i] = x; out[3 * i + 1] = y; out[3 * i + 2] = z;
}
void launch_vq_roundtrip(const double *in, double *out, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_vq_roundtrip, dim3(nblocks(n, TPB)), dim3(TPB), 0, s, in, out, n);
}
// out[i] = a[i] + b[i] + c[i] on rows [lo, hi)  (each may be null)
__global__ void k_sum_rows(const double4 *__restrict__ a, const double4 *__restrict__ b, const double4 *__restrict__ c,
                           double4 *__restrict__ out, int lo, int hi, const unsigned *__restrict__ tag_s) {
    const int i = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hi) return;
    double x = 0, y = 0, z = 0;
    if (a) { const double4 v = a[i]; x += v.x; y += v.y; z += v.z; }
    if (b) { const double4 v = b[i]; x += v.x; y += v.y; z += v.z; }
    if (c) { const double4 v = c[i]; x += v.x; y += v.y; z += v.z; }
    out[i] = make_double4(x, y, z, tag_s ? (double)tag_s[i] : 0.0);   // an index below 2^32 is exact in a double
}
void launch_sum_rows(const double4 *a, const double4 *b, const double4 *c, double4 *out, int lo, int hi, hipStream_t s,
                     const unsigned *tag_s) {
    if (hi > lo) hipLaunchKernelGGL(k_sum_rows, dim3(nblocks(hi - lo, TPB)), dim3(TPB), 0, s, a, b, c, out, lo, hi, tag_s);
}
// row boundaries of the cell slabs: out[r] = cell_off[r * stride] for r = 0..n-1
__global__ void k_pick(const int *__restrict__ cell_off, const int *__restrict__ idx, int n, int *__restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) out[r] = cell_off[idx[r]];
}
void launch_pick(const int *cell_off, const int *idx, int n, int *out, hipStream_t s) {
    hipLaunchKernelGGL(k_pick, dim3(nblocks(n, TPB)), dim3(TPB), 0, s, cell_off, idx, n, out);
}

// K13 gpu_stokes_MatVecMultiply_kernel (PSEv1/Helper.cu:251-279) + the final rescale (PSEv1/Brownian.cu:739) -- and, round 4, what used to
// be the next launch: with a sink the Brownian part is added to the far-field and near-field velocities of the row on the fly and
// goes straight to where the step wants the sum (a team: the row of the all-gathered array, tag in .w; a single GPU: vel[tag].xyz),
// so ub_s is neither written nor read back (K10 gpu_stokes_LinearCombination_kernel, PSEv1/Helper.cu:113-133)
__global__ void __launch_bounds__(TPB)
k_basis_combine(VecIn x0, VecIn V, size_t stride, BasisCoef tc, int m,
                const double *__restrict__ scal, double scale, int use_norm, double4 *__restrict__ out, int lo, int N, CombineSink sink,
                const LzState *__restrict__ st) {
    const double *t = tc.t;   // kernel arguments: no host-to-device copy whose source the host would have to keep alive
    if (st) { m = st->m_final; t = st->coef; }   // ... or what the device-side decision left (queue-only calls)
    const double sc = use_norm ? scale * scal[LZ_NORM] : scale;
    for (int i = lo + blockIdx.x * TPB + threadIdx.x; i < N; i += gridDim.x * TPB) {
        double x = 0, y = 0, z = 0;
        for (int q = 0; q < m; ++q) {
            double3 v;   // x_0 = psi was never copied into the basis; stride: rows of one basis vector, in either layout
            if (q == 0) row_load(x0, i, v.x, v.y, v.z); else row_load(V, (size_t)q * stride + i, v.x, v.y, v.z);
            const double tq = t[q];
            x += tq * v.x; y += tq * v.y; z += tq * v.z;
        }
        x *= sc; y *= sc; z *= sc;
        if (!sink.on) { out[i] = make_double4(x, y, z, 0.0); continue; }
        // a + b + c in the order the separate pass added them: far field, near field, Brownian
        double sx = 0.0, sy = 0.0, sz = 0.0;
        if (sink.add_a) { const double4 v = sink.add_a[i]; sx += v.x; sy += v.y; sz += v.z; }
        if (sink.add_b) { const double4 v = sink.add_b[i]; sx += v.x; sy += v.y; sz += v.z; }
        sx += x; sy += y; sz += z;
        const unsigned idx = sink.tag_s[i];
        if (sink.vel) { double4 o = sink.vel[idx]; o.x = sx; o.y = sy; o.z = sz; sink.vel[idx] = o; }
        else sink.rows[i] = make_double4(sx, sy, sz, (double)idx);
    }
}
void launch_basis_combine(VecIn x0, VecIn V, size_t stride, const BasisCoef &t_dev, int m, const double *scal,
                          double scale, int use_norm, double4 *out_s, int lo, int hi, hipStream_t s, CombineSink sink, const LzState *st) {
    hipLaunchKernelGGL(k_basis_combine, dim3(std::min(2048, std::max(1, nblocks(hi - lo, TPB)))), dim3(TPB), 0, s, x0, V, stride,
                       t_dev, m, scal, scale, use_norm, out_s, lo, hi, sink, st);
}

// K10 gpu_stokes_LinearCombination_kernel (PSEv1/Helper.cu:113-133) as the final un-sort: vel.xyz = a + b + c, keep w
__global__ void k_scatter_sum(const double4 *__restrict__ a, const double4 *__restrict__ b,
                              const double4 *__restrict__ c, const unsigned *__restrict__ tag_s, int N,
                              double4 *__restrict__ vel) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= N) return;
    double x = 0, y = 0, z = 0;
    if (a) { const double4 v = a[s]; x += v.x; y += v.y; z += v.z; }
    if (b) { const double4 v = b[s]; x += v.x; y += v.y; z += v.z; }
    if (c) { const double4 v = c[s]; x += v.x; y += v.y; z += v.z; }
    const unsigned idx = tag_s ? tag_s[s] : (unsigned)a[s].w;
    double4 o = vel[idx];
    o.x = x; o.y = y; o.z = z;
    vel[idx] = o;
}
void launch_scatter_sum(const double4 *a, const double4 *b, const double4 *c, const unsigned *tag_s, int N,
                        double4 *vel, hipStream_t s) {
    hipLaunchKernelGGL(k_scatter_sum, dim3(nblocks(N, TPB)), dim3(TPB), 0, s, a, b, c, tag_s, N, vel);
}

// K15 gpu_stokes_step_one_kernel (PSEv1/Stokes.cu:137-192)
__global__ void k_integrate(double4 *__restrict__ pos, const double4 *__restrict__ vel, double3 *__restrict__ accel,
                            int3 *__restrict__ image, const double4 *__restrict__ force,
                            const unsigned *__restrict__ group, int N, DBox box, double dt, double shear_rate) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= N) return;
    const unsigned idx = group ? group[g] : (unsigned)g;
    double4 p = pos[idx];
    const double4 v = vel[idx];
    const double4 F = force[idx];
    p.x += (v.x + shear_rate * p.y) * dt;   // Stokes.cu:164-171
    p.y += v.y * dt;
    p.z += v.z * dt;
    int3 im = image[idx];
    // triclinic wrap (HOOMD BoxDim::wrap): z, then y (a y image shifts x by xy*Ly), then x
    double n = floor(p.z * box.iLz + 0.5);
    p.z -= n * box.Lz; im.z += (int)n;
    n = floor(p.y * box.iLy + 0.5);
    p.y -= n * box.Ly; p.x -= n * box.xy * box.Ly; im.y += (int)n;
    n = floor((p.x - box.xy * p.y) * box.iLx + 0.5);
    p.x -= n * box.Lx; im.x += (int)n;
    const double im_ = 1.0 / v.w;            // mass in vel.w (Stokes.cu:160,174)
    accel[idx] = make_double3(F.x * im_, F.y * im_, F.z * im_);
    pos[idx] = p;
    image[idx] = im;
}
void launch_integrate(double4 *pos, const double4 *vel, double3 *accel, int3 *image, const double4 *force,
                      const unsigned *group, int N, DBox box, double dt, double shear_rate, hipStream_t s) {
    hipLaunchKernelGGL(k_integrate, dim3(nblocks(N, TPB)), dim3(TPB), 0, s, pos, vel, accel, image, force, group, N,
                       box, dt, shear_rate);
}
// the exchanges of a team: the sum of a received buffer into its target, and the copies of one exchange as one launch
__global__ void k_axpy_inplace(double *__restrict__ a, const double *__restrict__ b, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) a[i] += b[i];
}
__global__ void __launch_bounds__(TPB) k_copy_list(CopyList l) {
    const int it = blockIdx.y;
    const double *__restrict__ src = l.src[it];
    double *__restrict__ dst = l.dst[it];
    const unsigned n = l.cnt[it];
    if ((((size_t)src | (size_t)dst) & 15) == 0) {   // 16-byte pieces where both ends allow
        const unsigned n2 = n >> 1;
        for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < n2; i += gridDim.x * TPB) ((double2 *)dst)[i] = ((const double2 *)src)[i];
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) dst[n - 1] = src[n - 1];
    } else {
        for (unsigned i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) dst[i] = src[i];
    }
}
void launch_copy_list(const CopyList &l, hipStream_t s) {
    if (l.n <= 0) return;
    unsigned mx = 0;
    for (int i = 0; i < l.n; ++i) mx = std::max(mx, l.cnt[i]);
    const int gx = std::max(1, std::min(256, nblocks((long)(mx / 2 + 1), TPB)));
    hipLaunchKernelGGL(k_copy_list, dim3(gx, l.n), dim3(TPB), 0, s, l);
}
void launch_add_inplace(double *a, const double *b, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_axpy_inplace, dim3(std::min<long>(2048, nblocks((long)n, TPB))), dim3(TPB), 0, s, a, b, n);
}

}  // namespace pse
