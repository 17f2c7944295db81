// The transforms of the far field on gfx950 (CDNA4, wave64): the k-space operator (K1 + K5 + K6), the x passes fused with it, the own
// y passes, the z pass of 256 / 512 points (the general one is pse_zfft.hip) and the pack / unpack of a slab rank's all-to-all
// blocks.  Each kernel names the reference kernel it replaces.  All arithmetic is fp64.
#include "pse_fft.h"
#include "pse_dft.h"

namespace pse {

constexpr double TWO_PI = 6.283185307179586476925286766559;

// K1+K5+K6 fused: gpu_stokes_SetGridk_kernel (PSEv1/Helper.cu:285-332), gpu_stokes_Green_kernel
// (PSEv1/Mobility.cu:264-299) and gpu_stokes_BrownianGridGenerate_kernel (PSEv1/Brownian.cu:153-345) on the
// real-to-complex half spectrum.  Wave vectors are computed in registers (no gridk array).
struct KOp {
    double kx, ky, kz, ik2, B, c;  // 1 / k^2, B = w sinc^2 (deterministic), c = noise_fac sqrt(w) sinc
};
__device__ __forceinline__ KOp make_kop(int i, int j, int k, const DGrid &G, const DBox &box, double xi, double eta,
                                        double noise_fac) {
    KOp o;
    const int ki = i < (G.Nx + 1) / 2 ? i : i - G.Nx;     // FFT index folding, PSEv1/Helper.cu:307-312
    const int kj = j < (G.Ny + 1) / 2 ? j : j - G.Ny;
    const int kk = k < (G.Nz + 1) / 2 ? k : k - G.Nz;
    o.kx = TWO_PI * ki * box.iLx;
    o.ky = TWO_PI * (kj * box.iLy - box.xy * ki * box.iLx);   // sheared reciprocal lattice, Helper.cu:308
    o.kz = TWO_PI * kk * box.iLz;
    // one reciprocal square root serves 1 / k^2, |k| and 1 / |k|; the loop-invariant reciprocals are hoisted by the compiler
    const double k2 = o.kx * o.kx + o.ky * o.ky + o.kz * o.kz;
    const double rk = rsqrt(k2), kn = k2 * rk;
    o.ik2 = rk * rk;
    const double q = k2 * (1.0 / (4.0 * xi * xi));
    const double ing = 1.0 / ((double)G.Nx * (double)G.Ny * (double)G.Nz);
    const double w = 6.0 * M_PI * (1.0 + q) * exp_neg(-(1.0 - eta) * q) * (o.ik2 * ing);   // Helper.cu:326
    const double sinc = sin_lean(kn) * rk;                                            // Mobility.cu:290 (a = 1)
    o.B = w * sinc * sinc;
    o.c = noise_fac != 0.0 ? noise_fac * sqrt(w) * sinc : 0.0;                        // Brownian.cu:197,274-276
    return o;
}
// out += B (I - kk) f + c (I - kk) psi    (complex 3-vectors)
__device__ __forceinline__ void apply_kop(const KOp &o, const double2 f[3], const double2 psi[3], bool noise,
                                          double scale, double2 out[3]) {
    const double ik2 = o.ik2;
    double2 v[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        v[a].x = o.B * f[a].x;
        v[a].y = o.B * f[a].y;
        if (noise) { v[a].x += o.c * psi[a].x; v[a].y += o.c * psi[a].y; }
    }
    const double dr = (o.kx * v[0].x + o.ky * v[1].x + o.kz * v[2].x) * ik2;
    const double di = (o.kx * v[0].y + o.ky * v[1].y + o.kz * v[2].y) * ik2;
    const double kv[3] = {o.kx, o.ky, o.kz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out[a].x += scale * (v[a].x - kv[a] * dr);
        out[a].y += scale * (v[a].y - kv[a] * di);
    }
}

// What K5 + K6 do to one node (i,j,k) of the half spectrum: f -> B (I - kk) f + c (I - kk) psi.
__device__ __forceinline__ void scale_node(int i, int j, int k, const double2 f[3], const DGrid &G, const DBox &box,
                                           const ScaleArgs &a, double2 out[3]) {
    out[0] = out[1] = out[2] = make_double2(0, 0);
    if (i == 0 && j == 0 && k == 0) return;   // k = 0 mode is dropped (Helper.cu:321-323, Mobility.cu:287)
    // Hermitian bookkeeping.  The reference fills the FULL complex grid, every node with the folded wave vector of its own index
    // (PSEv1/Helper.cu:307-315), transforms back with a C2C FFT and keeps the real part (PSEv1/Mobility.cu:447) -- i.e. the
    // Hermitian part 1/2 (G(k) + conj G(partner)) of what it wrote.  The equivalent on the half spectrum of a C2R inverse is the
    // symmetrised operator (S(k_node) + S(k_partner)) / 2, k_partner the folded wave vector of index (-i, -j, -k) mod N.
    // Wherever an index is a Nyquist index (even N) the folding gives node and partner the SAME sign in that component, so the
    // two operators differ (a whole x line for j = Ny/2, a node per line for i = Nx/2, the plane kz = Nz/2); elsewhere
    // k_partner = -k_node, S is even in k, and one evaluation serves.  Held to the reference's kernels by
    // tests/golden/reference_kernels.json.gz (Green and noise, even / odd / mixed grids).
    const bool plane = (k == 0) || ((G.Nz % 2 == 0) && (k == G.Nz / 2));
    const int ip = (G.Nx - i) % G.Nx, jp = (G.Ny - j) % G.Ny;
    double2 psi[3] = {{0, 0}, {0, 0}, {0, 0}};
    if (a.noise) {
        // K6: complex psi with Re, Im ~ U(-sqrt(3/2), sqrt(3/2)) (variance 1/2 each, Brownian.cu:178-189), keyed by the
        // canonical member of each conjugate pair so both members reconstruct the same draw; self-conjugate nodes are
        // real with variance 1 (x sqrt2, Brownian.cu:255-268).
        const unsigned long long own = ((unsigned long long)i * G.Ny + j) * G.Nz + k;
        const unsigned long long par = ((unsigned long long)ip * G.Ny + jp) * G.Nz + k;
        const bool selfc = plane && par == own;
        const bool flip = plane && par < own;
        const unsigned long long canon = (plane && par < own) ? par : own;
        uint32_t ra[4], rb[4];
        const uint32_t ts = a.ts_off ? a.timestep + *a.ts_off : a.timestep;
        philox4x32((uint32_t)canon, (uint32_t)(canon >> 32), ts, DOMAIN_GRID_A, a.seed, PHILOX_KEY1, ra);
        philox4x32((uint32_t)canon, (uint32_t)(canon >> 32), ts, DOMAIN_GRID_B, a.seed, PHILOX_KEY1, rb);
        const double s = 1.2247448713915890;  // sqrt(3/2)
        const double re[3] = {uniform_pm(ra[0], s), uniform_pm(ra[1], s), uniform_pm(ra[2], s)};
        const double im[3] = {uniform_pm(ra[3], s), uniform_pm(rb[0], s), uniform_pm(rb[1], s)};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (selfc) psi[c] = make_double2(1.4142135623730951 * re[c], 0.0);
            else       psi[c] = make_double2(re[c], flip ? -im[c] : im[c]);
        }
    }
    const KOp o1 = make_kop(i, j, k, G, box, a.xi, a.eta, a.noise_fac);
    const bool nyq = plane || ((G.Nx % 2 == 0) && (i == G.Nx / 2)) || ((G.Ny % 2 == 0) && (j == G.Ny / 2));
    if (nyq) {
        const KOp o2 = make_kop(ip, jp, (G.Nz - k) % G.Nz, G, box, a.xi, a.eta, a.noise_fac);
        apply_kop(o1, f, psi, a.noise, 0.5, out);
        apply_kop(o2, f, psi, a.noise, 0.5, out);
    } else {
        apply_kop(o1, f, psi, a.noise, 1.0, out);
    }
}

// debug: the k-space operator of given nodes (i, j, k) as the scaling kernels evaluate it: kx, ky, kz, B = w sinc^2,
// c / noise_fac = sqrt(w) sinc  (what K1 gpu_stokes_SetGridk_kernel tabulates and K5 / K6 apply, PSEv1/Helper.cu:300-327)
__global__ void k_debug_kop(const int *__restrict__ ijk, int n, DGrid G, DBox box, double xi, double eta, double *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int i = ijk[3 * t], j = ijk[3 * t + 1], k = ijk[3 * t + 2];
    KOp o = make_kop(i, j, k, G, box, xi, eta, 1.0);
    if (i == 0 && j == 0 && k == 0) { o.B = 0.0; o.c = 0.0; }
    out[5 * t] = o.kx; out[5 * t + 1] = o.ky; out[5 * t + 2] = o.kz; out[5 * t + 3] = o.B; out[5 * t + 4] = o.c;
}
void launch_debug_kop(const int *ijk, int n, DGrid G, DBox box, double xi, double eta, double *out, hipStream_t s) {
    hipLaunchKernelGGL(k_debug_kop, dim3(nblocks(n, TPB)), dim3(TPB), 0, s, ijk, n, G, box, xi, eta, out);
}

__global__ void __launch_bounds__(TPB)
k_scale(double2 *__restrict__ X, double2 *__restrict__ Y, double2 *__restrict__ Z, DGrid G, DBox box, ScaleArgs a) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t rows = a.transposed ? (size_t)a.nyl * G.Nx : (size_t)G.nxl * G.Ny;
    if (tid >= rows * G.Nzp) return;
    const int k = (int)(tid % G.Nzp);
    if (k >= G.Nzh) return;                                  // padding of the row
    const size_t row = tid / G.Nzp;
    int i, j;
    if (a.transposed) { i = (int)(row / a.nyl); j = a.y0 + (int)(row % a.nyl); }   // [Nx][ny_local][Nzh]
    else              { i = G.x0 + (int)(row / G.Ny); j = (int)(row % G.Ny); }
    const double2 f[3] = {X[tid], Y[tid], Z[tid]};
    double2 out[3];
    scale_node(i, j, k, f, G, box, a, out);
    X[tid] = out[0]; Y[tid] = out[1]; Z[tid] = out[2];
}

void launch_scale(double2 *X, double2 *Y, double2 *Z, DGrid G, DBox box, ScaleArgs a, hipStream_t s) {
    const size_t rows = a.transposed ? (size_t)a.nyl * G.Nx : (size_t)G.nxl * G.Ny;
    hipLaunchKernelGGL(k_scale, dim3(nblocks((long)(rows * G.Nzp), TPB)), dim3(TPB), 0, s, X, Y, Z, G, box, a);
}

// ---- fused x pass -----------------------------------------------------------------------------------------------
// For a power-of-two Nx the last forward axis pass, the k-space scaling (+ noise) and the first inverse axis pass are one
// kernel: a workgroup owns KB consecutive kz columns of one y row for all three components ([3][KB][Nx] complex in LDS),
// runs the forward x transforms (Stockham radix-4/2, in place through registers), applies scale_node, runs the inverse
// transforms and stores -- the spectra cross HBM once instead of three times (rocFFT x pass, k_scale, rocFFT x pass).
// Both transforms are unnormalised: the 1/Ng lives in the scale factor (Helper.cu:325-326).

template <int LOGN, int KB, int NTH, bool INVERSE>
__device__ __forceinline__ void lds_fft_x(double2 *__restrict__ d, const double2 *__restrict__ tw) {
    constexpr int N = 1 << LOGN, NCOL = 3 * KB, CS = N + 1;   // padded column stride: columns start on different banks
    const int tid = threadIdx.x;
    int ns = 1;
#pragma unroll
    for (int done = 0; done < LOGN;) {
        if (LOGN - done >= 2) {
            constexpr int R = 4, NB = NCOL * (N / R), PER = (NB + NTH - 1) / NTH;
            double2 v[PER][R];
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int bfly = tid + q * NTH;
                if (bfly < NB) {
                    const int col = bfly / (N / R), jj = bfly - col * (N / R), kk = jj & (ns - 1);
                    const double2 *src = d + col * CS + jj;
                    const int tstep = kk * (N / (ns * R));
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        double2 x = src[r * (N / R)];
                        if (r) { double2 w = tw[r * tstep]; if (INVERSE) w.y = -w.y; x = cmul(x, w); }
                        v[q][r] = x;
                    }
                    const double2 a0 = make_double2(v[q][0].x + v[q][2].x, v[q][0].y + v[q][2].y);
                    const double2 a1 = make_double2(v[q][0].x - v[q][2].x, v[q][0].y - v[q][2].y);
                    const double2 a2 = make_double2(v[q][1].x + v[q][3].x, v[q][1].y + v[q][3].y);
                    const double2 t = make_double2(v[q][1].x - v[q][3].x, v[q][1].y - v[q][3].y);
                    const double2 a3 = INVERSE ? make_double2(-t.y, t.x) : make_double2(t.y, -t.x);   // +-i (v1 - v3)
                    v[q][0] = make_double2(a0.x + a2.x, a0.y + a2.y);
                    v[q][1] = make_double2(a1.x + a3.x, a1.y + a3.y);
                    v[q][2] = make_double2(a0.x - a2.x, a0.y - a2.y);
                    v[q][3] = make_double2(a1.x - a3.x, a1.y - a3.y);
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int bfly = tid + q * NTH;
                if (bfly < NB) {
                    const int col = bfly / (N / R), jj = bfly - col * (N / R), kk = jj & (ns - 1);
                    double2 *dst = d + col * CS + (jj - kk) * R + kk;
#pragma unroll
                    for (int r = 0; r < R; ++r) dst[r * ns] = v[q][r];
                }
            }
            __syncthreads();
            ns *= 4; done += 2;
        } else {
            constexpr int R = 2, NB = NCOL * (N / R), PER = (NB + NTH - 1) / NTH;
            double2 v[PER][R];
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int bfly = tid + q * NTH;
                if (bfly < NB) {
                    const int col = bfly / (N / R), jj = bfly - col * (N / R), kk = jj & (ns - 1);
                    const double2 *src = d + col * CS + jj;
                    double2 w = tw[kk * (N / (ns * R))];
                    if (INVERSE) w.y = -w.y;
                    const double2 x0 = src[0], x1 = cmul(src[N / R], w);
                    v[q][0] = make_double2(x0.x + x1.x, x0.y + x1.y);
                    v[q][1] = make_double2(x0.x - x1.x, x0.y - x1.y);
                }
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                const int bfly = tid + q * NTH;
                if (bfly < NB) {
                    const int col = bfly / (N / R), jj = bfly - col * (N / R), kk = jj & (ns - 1);
                    double2 *dst = d + col * CS + (jj - kk) * R + kk;
                    dst[0] = v[q][0];
                    dst[ns] = v[q][1];
                }
            }
            __syncthreads();
            ns *= 2; done += 1;
        }
    }
}

template <int LOGN, int KB, int NTH>
__global__ void __launch_bounds__(NTH, (NTH == 256 ? 3 : 1))   // 256 threads: <= 168 VGPRs so that three workgroups share a CU
k_xfft_scale(double2 *__restrict__ X, double2 *__restrict__ Y, double2 *__restrict__ Z, DGrid G, DBox box, ScaleArgs a,
             const double2 *__restrict__ twiddle) {
    constexpr int N = 1 << LOGN, CS = N + 1;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double2 *d = reinterpret_cast<double2 *>(smem_raw);      // [3][KB][N + 1]
    double2 *tw = d + 3 * KB * CS;                            // [N]  exp(-2 pi i m / N)
    const int tid = threadIdx.x;
    const int nkb = (G.Nzh + KB - 1) / KB;
    // layout [Nx][rows][Nzh] per component: all Ny rows on a single GPU, the nyl rows [y0, y0 + nyl) of this rank after
    // the slab transpose
    const int rows = a.transposed ? a.nyl : G.Ny;
    // neighbouring kz blocks of a row share 128-byte lines (a block's pieces are 64 or 32 bytes): keep them on one XCD, so the
    // second one finds the line in that XCD's L2 (round-robin placement fetched every line from memory twice)
    const int bid = xcd_block(blockIdx.x, gridDim.x);
    const int jl = bid / nkb, k0 = (bid - jl * nkb) * KB;
    const int j = a.transposed ? a.y0 + jl : jl;
    const int kv = min(KB, G.Nzh - k0);
    double2 *comp[3] = {X, Y, Z};
    const size_t xstride = (size_t)rows * G.Nzp, base = (size_t)jl * G.Nzp + k0;
    for (int e = tid; e < N; e += NTH) tw[e] = twiddle[e];
    {   // every load of a lane in flight before the first is parked in LDS (a load -> store loop pays the latency per element)
        constexpr int PER = (3 * N * KB + NTH - 1) / NTH;
        double2 v[PER];
#pragma unroll
        for (int it = 0; it < PER; ++it) {                    // KB consecutive kz are contiguous in memory (128 B at KB = 8)
            const int e = tid + it * NTH, c = e / (N * KB), r = e - c * (N * KB), x = r / KB, q = r - x * KB;
            v[it] = make_double2(0, 0);
            if (e < 3 * N * KB && q < kv) v[it] = comp[c][(size_t)x * xstride + base + q];
        }
#pragma unroll
        for (int it = 0; it < PER; ++it) {
            const int e = tid + it * NTH, c = e / (N * KB), r = e - c * (N * KB), x = r / KB, q = r - x * KB;
            if (e < 3 * N * KB) d[(c * KB + q) * CS + x] = v[it];
        }
    }
    __syncthreads();
    lds_fft_x<LOGN, KB, NTH, false>(d, tw);
    for (int e = tid; e < N * KB; e += NTH) {
        const int x = e / KB, q = e - x * KB;
        if (q < kv) {
            const double2 f[3] = {d[q * CS + x], d[(KB + q) * CS + x], d[(2 * KB + q) * CS + x]};
            double2 out[3];
            scale_node(x, j, k0 + q, f, G, box, a, out);
            d[q * CS + x] = out[0]; d[(KB + q) * CS + x] = out[1]; d[(2 * KB + q) * CS + x] = out[2];
        }
    }
    __syncthreads();
    lds_fft_x<LOGN, KB, NTH, true>(d, tw);
    for (int e = tid; e < 3 * N * KB; e += NTH) {
        const int c = e / (N * KB), r = e - c * (N * KB), x = r / KB, q = r - x * KB;
        if (q < kv) comp[c][(size_t)x * xstride + base + q] = d[(c * KB + q) * CS + x];
    }
}


// ---- any Nx = 2^a 3^b 5^c (the grids the reference's rule produces, PSEv1/Stokes.cc:147-199) ---------------------------------
// Mixed-radix Stockham passes (radix 5, 4, 3, 2) between two LDS buffers: a butterfly reads its R points from one buffer and
// writes them to the other, so nothing is held across the barrier and the number of butterflies per lane may be anything.
struct FftPlanX { int n, nstage, radix[10]; unsigned mns[10], mnr[10]; };   // + reciprocals ceil(2^32 / ns), ceil(2^32 / (n / R)) of every stage
__device__ __forceinline__ int fast_quot(int a, unsigned m) { return (int)__umulhi((unsigned)a, m); }   // a / d for a d < 2^31, m = ceil(2^32 / d)

// one pass over NCOL columns of n points (column stride cs): in -> out
template <int R, bool INVERSE>
__device__ __forceinline__ void fft_pass(const double2 *__restrict__ in, double2 *__restrict__ out, const double2 *__restrict__ tw,
                                         int n, int cs, int ncol, int ns, int nth, unsigned mns, unsigned mnr) {
    const int nr = n / R, nb = ncol * nr, tstep = n / (ns * R);
    for (int bfly = threadIdx.x; bfly < nb; bfly += nth) {
        const int col = fast_quot(bfly, mnr), jj = bfly - col * nr, kk = ns == 1 ? 0 : jj - fast_quot(jj, mns) * ns;   // no runtime divisions (ns = 1: the reciprocal 2^32 does not fit)
        const double2 *src = in + col * cs + jj;
        double2 v[9];
        // W^{r kk tstep} for r = 1 .. R - 1 as powers of ONE table entry: a read of the twiddle table per point was a third of the
        // LDS traffic of a pass, and the passes are what bounds the mixed-radix kernels (error: R - 2 <= 7 roundings)
        double2 w1 = tw[kk * tstep];                                 // kk * tstep < n
        if (INVERSE) w1.y = -w1.y;
        double2 w = w1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double2 x = src[r * nr];
            if (r) {
                x = cmul(x, w);
                if (r + 1 < R) w = cmul(w, w1);
            }
            v[r] = x;
        }
        dft_small<R, INVERSE>(v);
        double2 *dst = out + col * cs + (jj - kk) * R + kk;
#pragma unroll
        for (int r = 0; r < R; ++r) dst[r * ns] = v[r];
    }
}

template <bool INVERSE>
__device__ __forceinline__ double2 *fft_mixed(double2 *a, double2 *b, const double2 *tw, const FftPlanX &pl, int cs, int ncol, int nth) {
    int ns = 1;
    for (int st = 0; st < pl.nstage; ++st) {
        const int R = pl.radix[st];
        if (R == 9) fft_pass<9, INVERSE>(a, b, tw, pl.n, cs, ncol, ns, nth, pl.mns[st], pl.mnr[st]);
        else if (R == 8) fft_pass<8, INVERSE>(a, b, tw, pl.n, cs, ncol, ns, nth, pl.mns[st], pl.mnr[st]);
        else if (R == 5) fft_pass<5, INVERSE>(a, b, tw, pl.n, cs, ncol, ns, nth, pl.mns[st], pl.mnr[st]);
        else if (R == 4) fft_pass<4, INVERSE>(a, b, tw, pl.n, cs, ncol, ns, nth, pl.mns[st], pl.mnr[st]);
        else if (R == 3) fft_pass<3, INVERSE>(a, b, tw, pl.n, cs, ncol, ns, nth, pl.mns[st], pl.mnr[st]);
        else fft_pass<2, INVERSE>(a, b, tw, pl.n, cs, ncol, ns, nth, pl.mns[st], pl.mnr[st]);
        __syncthreads();
        double2 *t = a; a = b; b = t;
        ns *= R;
    }
    return a;                                                        // the buffer that holds the result
}

// The same passes with the length and the radices known at compile time (the sizes the reference's rule picks at the BASELINE
// configurations: 360, 270, 180, 375, 500, ...).  The fused x pass is bound by vector-instruction issue (57 % of the cycles, 3 170
// instructions per wave at 360: profiles/r04_x360_counters.txt); here the index arithmetic is constant-folded, the butterflies of a
// lane are unrolled so that the loads of the second are in flight during the first, the first pass (all twiddles 1) multiplies
// nothing, and later passes read their twiddles from the table (no product chain: arithmetic is what this kernel is short of).
template <int N_, int R0, int R1 = 1, int R2 = 1, int R3 = 1>
struct CtPlan { static constexpr int N = N_, NST = 1 + (R1 > 1) + (R2 > 1) + (R3 > 1); };
struct RtPlan { static constexpr int N = 0; };

template <int R, bool INVERSE, int N, int NS, int NCOL, int NTH>
__device__ __forceinline__ void fft_pass_ct(const double2 *__restrict__ in, double2 *__restrict__ out, const double2 *__restrict__ tw) {
    constexpr int NR = N / R, NB = NCOL * NR, TSTEP = N / (NS * R), CS = N + 1, ITER = (NB + NTH - 1) / NTH;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int bfly = (int)threadIdx.x + it * NTH;
        if (NB % NTH == 0 || bfly < NB) {
            const int col = bfly / NR, jj = bfly - col * NR, kk = NS == 1 ? 0 : jj % NS;
            const double2 *src = in + col * CS + jj;
            double2 v[9];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                double2 x = src[r * NR];
                if (r && NS > 1) {
                    double2 w = tw[r * kk * TSTEP];              // r kk TSTEP < R NS TSTEP = N
                    if (INVERSE) w.y = -w.y;
                    x = cmul(x, w);
                }
                v[r] = x;
            }
            dft_small<R, INVERSE>(v);
            double2 *dst = out + col * CS + (jj - kk) * R + kk;
#pragma unroll
            for (int r = 0; r < R; ++r) dst[r * NS] = v[r];
        }
    }
}
template <int R, bool INVERSE, int N, int NS, int NCOL, int NTH>
__device__ __forceinline__ void fft_stage_ct(double2 *&a, double2 *&b, const double2 *tw) {
    if constexpr (R > 1) {
        fft_pass_ct<R, INVERSE, N, NS, NCOL, NTH>(a, b, tw);
        __syncthreads();
        double2 *t = a; a = b; b = t;
    }
}
template <class P> struct CtRadices;
template <int N_, int R0, int R1, int R2, int R3>
struct CtRadices<CtPlan<N_, R0, R1, R2, R3>> { static constexpr int r0 = R0, r1 = R1, r2 = R2, r3 = R3; };
template <class P, bool INVERSE, int NCOL, int NTH>
__device__ __forceinline__ double2 *fft_mixed_ct(double2 *a, double2 *b, const double2 *tw) {
    using Rd = CtRadices<P>;
    fft_stage_ct<Rd::r0, INVERSE, P::N, 1, NCOL, NTH>(a, b, tw);
    fft_stage_ct<Rd::r1, INVERSE, P::N, Rd::r0, NCOL, NTH>(a, b, tw);
    fft_stage_ct<Rd::r2, INVERSE, P::N, Rd::r0 * Rd::r1, NCOL, NTH>(a, b, tw);
    fft_stage_ct<Rd::r3, INVERSE, P::N, Rd::r0 * Rd::r1 * Rd::r2, NCOL, NTH>(a, b, tw);
    return a;
}

// ---- N = R0 x R1 x R2 with ONE component in LDS at a time (512 = 8 x 8 x 8, 360 = 10 x 6 x 6, 256 = 4 x 8 x 8) ---------------------
// The kernels above keep the three components of a block of columns in LDS, which caps a 512-point block at two kz columns
// (32-byte pieces of every 128-byte line: 2.4 TB/s; the 256-point kernel loses the same 30 % when it is given two columns) and
// sends a point through LDS four times per transform.  Here the data live in registers, LDS holds one component of the block
// while it changes hands, and a workgroup owns KB = 4 kz columns (64-byte pieces; 8 = whole 128-byte pieces needs the kernel in 128
// registers, which it is not: 225 spilled, 3.3 ms at 512^3):
//   layout A (global memory side): thread (q, n) = (tid % KB, tid / KB), n < N / R0, holds x[n + (N / R0) r] of column q -- the
//            loads and stores of KB lanes cover one contiguous piece; stage 1 (decimation in frequency) is the radix-R0 transform over r;
//   layout B: wave w = column w; lanes (k0, n'') run stage 2 (radix R1 inside the N / R0-point transform k0), lanes (k0, k1) stage 3
//            (radix R2), with one exchange in between that stays inside the wave (LDS instructions of a wave execute in order: no
//            barrier).  Stage 3 leaves X[k0 + R0 k1 + R0 R1 k2] in register k2 of lane R1 k0 + k1 for all three components, so the
//            k-space operator works on registers (PARK: the third component waits in the lane's own LDS slots meanwhile -- the
//            operator needs ~100 registers of its own), and the inverse (decimation in time) runs the same stages backwards from
//            that digit-reversed order.
// Per transform a point crosses LDS twice; 10 barriers per block; every load of the block is in flight at once and a stage's
// twiddles are fetched once for the three components (stage by stage over the components: a variant that took a component
// through all stages before the next -- fewer live registers -- was 15 % slower at 512^3: three times the twiddle fetches).
// Every stage has registers of its own, defined in ALL lanes: where only some lanes take part in a layout (360: 144 of 256
// threads in A, 60 of 64 lanes in B) values left in the others would stay alive across the whole kernel (291 registers spilled).
// Global addresses are a uniform base plus a 32-bit byte offset per lane, recomputed at the stores (the launcher checks < 4 GiB
// per component): 64-bit addresses kept from the loads to the stores were spilled too.
// Positions in a column: B[k0][n] at P0 k0 + n, C[k0][k1][n] at P0 k0 + P1 k1 + n -- every access is a per-lane base plus a
// compile-time offset; P0, P1 and the column stride CS come from tools/debug/lds_banks_xcols.py (every access conflict-free but the
// layout A read of the inverse, two-way).
// 512^3: 1.5 ms = 4.3 TB/s in some processes, 1.77 ms in others (both kernels of this file show the two modes, whatever the
// plane stride: 128 bytes to 64 KB appended to every x plane changed nothing) against 2.77 ms; 360^3: 0.80 ms against 1.05.
// 256 = 8 x 8 x 4 through this kernel (one column per wave, 64-byte pieces): 0.25 - 0.27 ms at 256^3, no better than k_xfft_scale256;
// 256 = 4 x 8 x 8 with two columns per wave (CPW = 2, 128-byte pieces): 0.201 ms against 0.226 -- dispatched.
// Also measured and dropped: a table of the operator's scalars per node (what the reference keeps in gridk.w) instead of the
// exponential, sine and reciprocal square root per node: 256^3 0.25 -> 0.30 ms, 512^3 +20 % (a dependent load in the middle of
// the block costs more than the 150 instructions it saves).
template <int N, int R0, int R1, int KB, int WPS, bool PARK, int P0, int P1, int CS, int CPW = 1>
__global__ void __launch_bounds__(64 * KB / CPW, WPS)
k_xfft_scale_cols(double2 *__restrict__ X, double2 *__restrict__ Y, double2 *__restrict__ Z, DGrid G, DBox box, ScaleArgs a,
                  const double2 *__restrict__ twiddle) {
    // CPW = 2 (256 = 4 x 8 x 8): TWO columns per wave in layout B (32 lanes each), so that a workgroup of four waves owns eight kz
    // columns = whole 128-byte pieces; a thread of layout A then runs NBA = 2 butterflies (n and n + NTH / KB)
    constexpr int M1 = N / R0, R2 = M1 / R1, L2 = R0 * R2, L3 = R0 * R1, TA = KB * M1, LC = 64 / CPW, NTH = 64 * KB / CPW;
    constexpr int NBA = (TA + NTH - 1) / NTH, NSTEP = NTH / KB;
    static_assert(R0 * R1 * R2 == N && L2 <= LC && L3 <= LC && NTH % KB == 0 && (NBA == 1 || TA == NBA * NTH) && CS >= LC * R2, "plan");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double2 *buf = reinterpret_cast<double2 *>(smem_raw);    // [KB][CS]: one component of the block
    double2 *twS = buf + KB * CS;                            // exp(-2 pi i m / M1), m < M1
    const int tid = threadIdx.x;
    const int nkb = (G.Nzh + KB - 1) / KB;
    const int rows = a.transposed ? a.nyl : G.Ny;
    const int bid = xcd_block(blockIdx.x, gridDim.x);        // rows are not multiples of 128 bytes: neighbouring blocks share lines
    const int jl = bid / nkb, kz0 = (bid - jl * nkb) * KB;
    const int j = a.transposed ? a.y0 + jl : jl;
    const int kv = min(KB, G.Nzh - kz0);
    // global addresses: a component's block base (uniform) + a 32-bit byte offset per lane (the launcher checks that a component is
    // below 4 GiB), recomputed where it is used: 64-bit addresses of every point kept from the loads to the stores were most of
    // the register spills of this kernel
    const size_t xstride = (size_t)rows * G.Nzp, base = (size_t)jl * G.Nzp + kz0;
    char *comp[3] = {reinterpret_cast<char *>(X + base), reinterpret_cast<char *>(Y + base), reinterpret_cast<char *>(Z + base)};
    const unsigned xs16 = (unsigned)(xstride * sizeof(double2));
    const int q = tid % KB;                                  // layout A
    const bool actA = TA >= NTH || tid < TA;
    const int n1 = actA ? tid / KB : 0;                      // (+ NSTEP for the second butterfly)
    const int w = (tid >> 6) * CPW + (tid & 63) / LC, l = (tid & 63) % LC;   // layout B: column, lane of the column
    const bool act2 = L2 == LC || l < L2, act3 = L3 == LC || l < L3;
    const int kp2 = act2 ? l / R2 : 0, nn = l % R2, kp3 = act3 ? l / R1 : 0, k1 = l % R1;
    double2 *pA = buf + q * CS + n1;                         // + P0 k0 (+ NSTEP)
    double2 *pB = buf + w * CS + P0 * kp2 + nn;              // + R2 s (B), + P1 k1 (C)
    double2 *pC = buf + w * CS + P0 * kp3 + P1 * k1;         // + n'' (C of lane (k0, k1))
    double2 *pP = buf + w * CS + l;                          // + LC k2: the lane's own slots
    double2 ld[3][NBA][R0], v[3][R2];                        // layout A points of a component; its final values (every stage has registers of
                                                             // its own, defined in all lanes: what a stage leaves behind must not stay alive)
    const double2 zero = make_double2(0, 0);
    auto offset0 = [&]() __attribute__((always_inline)) {
        unsigned o = (unsigned)n1 * xs16 + (unsigned)q * (unsigned)sizeof(double2);
        asm volatile("" : "+v"(o));                           // not a common subexpression of the other uses
        return o;
    };
    auto load = [&](int c) __attribute__((always_inline)) {
        const unsigned o = offset0();
#pragma unroll
        for (int u = 0; u < NBA; ++u)
#pragma unroll
            for (int r = 0; r < R0; ++r) {
                ld[c][u][r] = make_double2(0, 0);
                if (actA && q < kv) ld[c][u][r] = *reinterpret_cast<const double2 *>(comp[c] + (size_t)(o + (unsigned)(M1 * r + NSTEP * u) * xs16));
            }
    };
    load(0); load(1); load(2);                               // every load of the block in flight at once
    if (tid < M1) twS[tid] = twiddle[R0 * tid];
    // ---- forward: stage 1 over r -> k0, times W_N^{n k0}
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int u = 0; u < NBA; ++u) dft_small<R0, false>(ld[c][u]);
#pragma unroll
    for (int u = 0; u < NBA; ++u)
#pragma unroll
        for (int k = 1; k < R0; ++k) {
            const double2 t = twiddle[(n1 + NSTEP * u) * k];
#pragma unroll
            for (int c = 0; c < 3; ++c) ld[c][u][k] = cmul(ld[c][u][k], t);
        }
    double2 b[3][R1];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c) __syncthreads();                               // every wave has read the previous component
        if (actA) {
#pragma unroll
            for (int u = 0; u < NBA; ++u)
#pragma unroll
                for (int k = 0; k < R0; ++k) pA[P0 * k + NSTEP * u] = ld[c][u][k];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < R1; ++s) b[c][s] = act2 ? pB[R2 * s] : zero;
    }
    // stage 2 over s -> k1, times W_M1^{n'' k1}
#pragma unroll
    for (int c = 0; c < 3; ++c) dft_small<R1, false>(b[c]);
#pragma unroll
    for (int k = 1; k < R1; ++k) {
        const double2 t = twS[nn * k];
#pragma unroll
        for (int c = 0; c < 3; ++c) b[c][k] = cmul(b[c][k], t);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {                             // inside the wave's own column: no barrier
        if (act2) {
#pragma unroll
            for (int k = 0; k < R1; ++k) pB[P1 * k] = b[c][k];
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int n = 0; n < R2; ++n) v[c][n] = act3 ? pC[n] : zero;
        __builtin_amdgcn_wave_barrier();
        dft_small<R2, false>(v[c]);                           // stage 3 over n'' -> k2
    }
    // ---- the k-space operator on X[k0 + R0 k1 + R0 R1 k2]
    if (PARK) {                                               // the third component waits in the lane's own slots: room for the operator's temporaries
#pragma unroll
        for (int k2 = 0; k2 < R2; ++k2) pP[LC * k2] = v[2][k2];
    }
    if (w < kv && act3) {
#pragma unroll
        for (int k2 = 0; k2 < R2; ++k2) {
            const double2 f[3] = {v[0][k2], v[1][k2], PARK ? pP[LC * k2] : v[2][k2]};
            double2 out[3];
            scale_node(kp3 + R0 * k1 + R0 * R1 * k2, j, kz0 + w, f, G, box, a, out);
            v[0][k2] = out[0]; v[1][k2] = out[1];
            if (PARK) pP[LC * k2] = out[2]; else v[2][k2] = out[2];
            __builtin_amdgcn_sched_barrier(0);                // one node at a time
        }
    }
    if (PARK) {
#pragma unroll
        for (int k2 = 0; k2 < R2; ++k2) v[2][k2] = pP[LC * k2];
        __builtin_amdgcn_wave_barrier();
    }
    // ---- inverse: stage 3 backwards over k2 -> n'', times conj W_M1^{n'' k1}
#pragma unroll
    for (int c = 0; c < 3; ++c) dft_small<R2, true>(v[c]);
#pragma unroll
    for (int n = 1; n < R2; ++n) {
        double2 t = twS[n * k1]; t.y = -t.y;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][n] = cmul(v[c][n], t);
    }
    double2 bi[3][R1];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (act3) {
#pragma unroll
            for (int n = 0; n < R2; ++n) pC[n] = v[c][n];
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < R1; ++k) bi[c][k] = act2 ? pB[P1 * k] : zero;
        __builtin_amdgcn_wave_barrier();
        dft_small<R1, true>(bi[c]);                           // stage 2 backwards over k1 -> s
    }
#pragma unroll
    for (int s = 0; s < R1; ++s) {                            // times conj W_N^{(R2 s + n'') k0}
        double2 t = twiddle[(R2 * s + nn) * kp2]; t.y = -t.y;
#pragma unroll
        for (int c = 0; c < 3; ++c) bi[c][s] = cmul(bi[c][s], t);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c) __syncthreads();                               // the layout A reads of the previous component are done
        if (act2) {
#pragma unroll
            for (int s = 0; s < R1; ++s) pB[R2 * s] = bi[c][s];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NBA; ++u) {
            double2 st[R0];
#pragma unroll
            for (int k = 0; k < R0; ++k) st[k] = actA ? pA[P0 * k + NSTEP * u] : zero;
            dft_small<R0, true>(st);                          // stage 1 backwards over k0 -> r
            if (actA && q < kv) {
                const unsigned o = offset0();
#pragma unroll
                for (int r = 0; r < R0; ++r) *reinterpret_cast<double2 *>(comp[c] + (size_t)(o + (unsigned)(M1 * r + NSTEP * u) * xs16)) = st[r];
            }
        }
    }
}

template <int N, int R0, int R1, int KB, int WPS, bool PARK, int P0, int P1, int CS, int CPW = 1>
static void launch_xfft_cols(double2 *X, double2 *Y, double2 *Z, DGrid G, DBox box, ScaleArgs a, const double2 *tw, hipStream_t s) {
    const size_t lds = (size_t)(KB * CS + N / R0) * sizeof(double2);
    const int nkb = (G.Nzh + KB - 1) / KB;
    const int rows = a.transposed ? a.nyl : G.Ny;
    launch_lds<k_xfft_scale_cols<N, R0, R1, KB, WPS, PARK, P0, P1, CS, CPW>>(dim3(rows * nkb), dim3(64 * KB / CPW), lds, s, X, Y, Z, G, box, a, tw);
}

template <int KB, int NTH, class PLAN = RtPlan>
__global__ void __launch_bounds__(NTH)
k_xfft_scale_mixed(double2 *__restrict__ X, double2 *__restrict__ Y, double2 *__restrict__ Z, DGrid G, DBox box, ScaleArgs a,
                   const double2 *__restrict__ twiddle, FftPlanX pl) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr bool CT = PLAN::N > 0;
    const int N = CT ? PLAN::N : pl.n, CS = N + 1;
    constexpr int NCOL = 3 * KB;
    double2 *bufa = reinterpret_cast<double2 *>(smem_raw), *bufb = bufa + NCOL * CS;   // [3][KB][N + 1] each
    double2 *tw = bufb + NCOL * CS;                                                     // [N]
    const int tid = threadIdx.x;
    const int nkb = (G.Nzh + KB - 1) / KB;
    const int rows = a.transposed ? a.nyl : G.Ny;
    // neighbouring kz blocks of a row share 128-byte lines (a block's pieces are 64 or 32 bytes): keep them on one XCD, so the
    // second one finds the line in that XCD's L2 (round-robin placement fetched every line from memory twice)
    const int bid = xcd_block(blockIdx.x, gridDim.x);
    const int jl = bid / nkb, k0 = (bid - jl * nkb) * KB;
    const int j = a.transposed ? a.y0 + jl : jl;
    const int kv = min(KB, G.Nzh - k0);
    double2 *comp[3] = {X, Y, Z};
    const size_t xstride = (size_t)rows * G.Nzp, base = (size_t)jl * G.Nzp + k0;
    for (int e = tid; e < N; e += NTH) tw[e] = twiddle[e];
    const int total = 3 * N * KB;
    for (int e0 = 0; e0 < total; e0 += 4 * NTH) {             // four loads of a lane in flight at a time
        double2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * NTH + tid, c = e / (N * KB), r = e - c * (N * KB), x = r / KB, q = r - x * KB;
            v[u] = make_double2(0, 0);
            if (e < total && q < kv) v[u] = comp[c][(size_t)x * xstride + base + q];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * NTH + tid, c = e / (N * KB), r = e - c * (N * KB), x = r / KB, q = r - x * KB;
            if (e < total) bufa[(c * KB + q) * CS + x] = v[u];
        }
    }
    __syncthreads();
    double2 *d;
    if constexpr (CT) d = fft_mixed_ct<PLAN, false, NCOL, NTH>(bufa, bufb, tw);
    else d = fft_mixed<false>(bufa, bufb, tw, pl, CS, NCOL, NTH);
    for (int e = tid; e < N * KB; e += NTH) {
        const int x = e / KB, q = e - x * KB;
        if (q < kv) {
            const double2 f[3] = {d[q * CS + x], d[(KB + q) * CS + x], d[(2 * KB + q) * CS + x]};
            double2 out[3];
            scale_node(x, j, k0 + q, f, G, box, a, out);
            d[q * CS + x] = out[0]; d[(KB + q) * CS + x] = out[1]; d[(2 * KB + q) * CS + x] = out[2];
        }
    }
    __syncthreads();
    if constexpr (CT) d = fft_mixed_ct<PLAN, true, NCOL, NTH>(d, d == bufa ? bufb : bufa, tw);
    else d = fft_mixed<true>(d, d == bufa ? bufb : bufa, tw, pl, CS, NCOL, NTH);
    for (int e = tid; e < total; e += NTH) {
        const int c = e / (N * KB), r = e - c * (N * KB), x = r / KB, q = r - x * KB;
        if (q < kv) comp[c][(size_t)x * xstride + base + q] = d[(c * KB + q) * CS + x];
    }
}

static bool plan_x(int n, FftPlanX &pl) {
    pl.n = n; pl.nstage = 0;
    int m = n;
    for (int r : {9, 8, 5, 4, 3, 2})   // few, wide passes: 360 = 9 8 5
        while (m % r == 0) { if (pl.nstage == 10) return false; pl.radix[pl.nstage++] = r; m /= r; }
    // the first pass scatters with a stride of R points: free of LDS bank conflicts for odd R only -- lead with an odd radix if there is one
    for (int st = 1; st < pl.nstage && (pl.radix[0] & 1) == 0; ++st)
        if (pl.radix[st] & 1) std::swap(pl.radix[0], pl.radix[st]);
    unsigned ns = 1;
    for (int st = 0; st < pl.nstage; ++st) {
        const unsigned nr = (unsigned)n / (unsigned)pl.radix[st];
        pl.mns[st] = (unsigned)((0x100000000ull + ns - 1) / ns);
        pl.mnr[st] = (unsigned)((0x100000000ull + nr - 1) / nr);
        ns *= (unsigned)pl.radix[st];
    }
    return m == 1;
}

template <int KB, int NTH, class PLAN = RtPlan>
static void launch_xfft_mixed(double2 *X, double2 *Y, double2 *Z, DGrid G, DBox box, ScaleArgs a, const double2 *tw, const FftPlanX &pl, hipStream_t s) {
    const size_t lds = (size_t)(2 * 3 * KB * (pl.n + 1) + pl.n) * sizeof(double2);
    const int nkb = (G.Nzh + KB - 1) / KB;
    const int rows = a.transposed ? a.nyl : G.Ny;
    launch_lds<k_xfft_scale_mixed<KB, NTH, PLAN>>(dim3(rows * nkb), dim3(NTH), lds, s, X, Y, Z, G, box, a, tw, pl);
}

// ---- own y pass (round 4): complex transforms along y of the half spectra, in place, for grids 2^a 3^b 5^c that are not powers of
// two.  rocFFT's strided pass over y is its slow one there (360^2: 0.93 ms of the 1.40 ms of its 2-D transform, the z pass takes
// 0.48 ms = what its bytes cost); here a workgroup takes KB consecutive kz of one x plane (KB * 16-byte pieces, neighbouring blocks on
// one XCD as in the x pass) and all Ny rows, through the same mixed-radix passes as the x pass.  The z passes stay rocFFT's (1-D).
// MAP (slab ranks of a team): the transform also does the reordering between the plane layout [3][nxl][Ny][Nzp] and the layout of the
// all-to-all blocks [3][G][nxl][nyl][Nzp] (y = q nyl + jl goes to rank q) -- 1: plane layout in, block layout out (forward: what
// k_slab_pack did in a pass of its own); 2: block layout in, plane layout out (inverse: the unpack).  0: in place, plane layout.
template <int KB, int NTH, bool INVERSE, int MAP = 0, class PLAN = RtPlan>
__global__ void __launch_bounds__(NTH)
k_fft_cols(double2 *__restrict__ data, FftPlanX pl, const double2 *__restrict__ twiddle, int nkb, int Nzh, int Nzp, size_t plane_stride,
           double2 *__restrict__ other = nullptr, int nxl = 0, int nyl = 0) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr bool CT = PLAN::N > 0;
    const int N = CT ? PLAN::N : pl.n, CS = N + 1;
    double2 *bufa = reinterpret_cast<double2 *>(smem_raw), *bufb = bufa + KB * CS;   // [KB][N + 1] each
    double2 *tw = bufb + KB * CS;                                                     // [N]
    const int tid = threadIdx.x;
    const int bid = xcd_block(blockIdx.x, gridDim.x);
    const int plane = bid / nkb, k0 = (bid - plane * nkb) * KB;
    const int kv = min(KB, Nzh - k0);
    double2 *base = data + (size_t)plane * plane_stride + k0;
    // the same (plane, y) in the block layout: component c = plane / nxl, plane lx = plane % nxl of this rank, block q = y / nyl
    const int pc = MAP ? plane / nxl : 0, plx = MAP ? plane - pc * nxl : 0;
    auto blk = [&](int y) -> size_t {
        const int q = y / nyl, jl = y - q * nyl;
        return (size_t)pc * nxl * plane_stride + (((size_t)q * nxl + plx) * nyl + jl) * Nzp + k0;
    };
    for (int e = tid; e < N; e += NTH) tw[e] = twiddle[e];
    const int total = N * KB;
    constexpr int U = 6;                                       // loads of a lane in flight at a time
    for (int e0 = 0; e0 < total; e0 += U * NTH) {
        double2 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * NTH + tid, y = e / KB, q = e - y * KB;
            v[u] = make_double2(0, 0);
            if (e < total && q < kv) v[u] = MAP == 2 ? other[blk(y) + q] : base[(size_t)y * Nzp + q];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * NTH + tid, y = e / KB, q = e - y * KB;
            if (e < total) bufa[q * CS + y] = v[u];
        }
    }
    __syncthreads();
    const double2 *d;
    if constexpr (CT) d = fft_mixed_ct<PLAN, INVERSE, KB, NTH>(bufa, bufb, tw);
    else d = fft_mixed<INVERSE>(bufa, bufb, tw, pl, CS, KB, NTH);
    for (int e = tid; e < total; e += NTH) {
        const int y = e / KB, q = e - y * KB;
        if (q < kv) {
            if (MAP == 1) other[blk(y) + q] = d[q * CS + y];
            else base[(size_t)y * Nzp + q] = d[q * CS + y];
        }
    }
}
bool yfft_possible(int Ny) {    // any 2^a 3^b 5^c, 16..512 (slab ranks: the pass also packs / unpacks the all-to-all blocks)
    FftPlanX pl;
    return Ny >= 16 && Ny <= 512 && plan_x(Ny, pl);
}
bool yfft_supported(int Ny) {   // 2^a 3^b 5^c, 16..512, not a power of two (rocFFT's 2-D kernels are good at those)
    FftPlanX pl;
    return Ny >= 16 && Ny <= 512 && (Ny & (Ny - 1)) != 0 && plan_x(Ny, pl);
}
template <int KB, int NTH, class PLAN = RtPlan>
static void launch_fft_cols(double2 *data, const FftPlanX &pl, const double2 *tw, int nplanes, int Nzh, int Nzp, size_t plane_stride,
                            bool inverse, hipStream_t s) {
    const size_t lds = (size_t)(2 * KB * (pl.n + 1) + pl.n) * sizeof(double2);
    const int nkb = (Nzh + KB - 1) / KB;
    const dim3 g(nplanes * nkb), b(NTH);
    if (inverse) launch_lds<k_fft_cols<KB, NTH, true, 0, PLAN>>(g, b, lds, s, data, pl, tw, nkb, Nzh, Nzp, plane_stride, nullptr, 0, 0);
    else launch_lds<k_fft_cols<KB, NTH, false, 0, PLAN>>(g, b, lds, s, data, pl, tw, nkb, Nzh, Nzp, plane_stride, nullptr, 0, 0);
}
// slab ranks: forward = planes (cgrid) -> transformed blocks (blocks); inverse = blocks -> transformed planes
static bool yfft_slab_regs(double2 *cgrid, double2 *blocks, DGrid G, int nyl, bool inverse, const double2 *tw, hipStream_t s);   // Ny = 256, 512: the register pass
void launch_yfft_slab(double2 *cgrid, double2 *blocks, DGrid G, int nyl, bool inverse, const double2 *tw, hipStream_t s, bool regs) {
    if (regs && yfft_slab_regs(cgrid, blocks, G, nyl, inverse, tw, s)) return;
    FftPlanX pl;
    plan_x(G.Ny, pl);
    constexpr int KB = 4, NTH = 256;
    const size_t lds = (size_t)(2 * KB * (pl.n + 1) + pl.n) * sizeof(double2);
    const int nkb = (G.Nzh + KB - 1) / KB, nplanes = 3 * G.nxl;
    const size_t ps = (size_t)G.Ny * G.Nzp;
    const dim3 g(nplanes * nkb), b(NTH);
    if (inverse) launch_lds<k_fft_cols<KB, NTH, true, 2>>(g, b, lds, s, cgrid, pl, tw, nkb, G.Nzh, G.Nzp, ps, blocks, G.nxl, nyl);
    else launch_lds<k_fft_cols<KB, NTH, false, 1>>(g, b, lds, s, cgrid, pl, tw, nkb, G.Nzh, G.Nzp, ps, blocks, G.nxl, nyl);
}
// ---- the y pass of Ny = 256 = 8 x 8 x 4 with the data in registers ------------------------------------------------------------------
// The stages of k_xfft_scale_cols without the operator: one component, one direction, natural order in and out -- after stage 3
// the wave parks X[k0 + 8 k1 + 64 k2] at its natural position of the column (padded by one per eight: the strided writes and the
// layout A reads are conflict-free), one more barrier, and layout A stores whole pieces.  Three trips through LDS and two barriers
// per block; eight kz columns = 128-byte pieces at ~60 registers.  (Inverse = the same decimation in frequency with conjugate
// twiddles, unnormalised like rocFFT's.)
// MAP (slab ranks, as k_fft_cols): 1 the forward pass stores into the all-to-all blocks `other`, 2 the inverse pass loads from them
template <int N, int R0, int R1, int KB, bool INVERSE, int P0, int P1, int CS, int MAP = 0>
__global__ void __launch_bounds__(64 * KB)
k_yfft_regs(double2 *__restrict__ data, const double2 *__restrict__ twiddle, int nkb, int Nzh, int Nzp, size_t plane_stride,
            double2 *__restrict__ other = nullptr, int nxl = 0, int nyl = 0) {
    constexpr int M1 = N / R0, R2 = M1 / R1, L2 = R0 * R2, L3 = R0 * R1, TA = KB * M1, PN = M1 + M1 / 8;
    static_assert(R0 == 8 && R1 == 8 && R0 * R1 * R2 == N && L2 <= 64 && TA <= 64 * KB && CS >= N + N / 8, "plan");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double2 *buf = reinterpret_cast<double2 *>(smem_raw);    // [KB][CS]
    double2 *twS = buf + KB * CS;                            // exp(-2 pi i m / M1), m < M1
    const int tid = threadIdx.x;
    const int bid = xcd_block(blockIdx.x, gridDim.x);
    const int plane = bid / nkb, kz0 = (bid - plane * nkb) * KB, kv = min(KB, Nzh - kz0);
    char *base = reinterpret_cast<char *>(data + (size_t)plane * plane_stride + kz0);
    const unsigned row16 = (unsigned)Nzp * (unsigned)sizeof(double2);
    const int q = tid % KB;
    const bool actA = TA == 64 * KB || tid < TA;
    const int n1 = actA ? tid / KB : 0;
    const int w = tid >> 6, l = tid & 63;
    const bool act2 = L2 == 64 || l < L2;
    const int kp2 = act2 ? l / R2 : 0, nn = l % R2, kp3 = l / R1, k1 = l % R1;
    double2 *pA = buf + q * CS + n1;                         // + P0 k0
    double2 *pB = buf + w * CS + P0 * kp2 + nn;              // + R2 s (B), + P1 k1 (C)
    double2 *pC = buf + w * CS + P0 * kp3 + P1 * k1;         // + n''
    double2 *pN = buf + w * CS + kp3 + 9 * k1;               // + 72 k2: natural position ky + ky / 8 of ky = k0 + 8 k1 + 64 k2
    double2 *pO = buf + q * CS + n1 + (n1 >> 3);             // + PN r: natural position of y = n + M1 r
    const double2 zero = make_double2(0, 0);
    const unsigned o0 = (unsigned)n1 * row16 + (unsigned)q * (unsigned)sizeof(double2);
    // the same (plane, y) in the block layout: component pc = plane / nxl, plane plx of this rank, block y / nyl
    const int pc = MAP ? plane / nxl : 0, plx = MAP ? plane - pc * nxl : 0;
    auto blk = [&](int y) -> double2 * {
        const int qb = y / nyl, jl = y - qb * nyl;
        return other + (size_t)pc * nxl * plane_stride + (((size_t)qb * nxl + plx) * nyl + jl) * Nzp + kz0 + q;
    };
    double2 a[R0];
#pragma unroll
    for (int r = 0; r < R0; ++r) {
        a[r] = zero;
        if (actA && q < kv) a[r] = MAP == 2 ? *blk(n1 + M1 * r) : *reinterpret_cast<const double2 *>(base + (size_t)(o0 + (unsigned)(M1 * r) * row16));
    }
    if (tid < M1) twS[tid] = twiddle[R0 * tid];
    dft_small<R0, INVERSE>(a);                                // stage 1 over r -> k0, times W_N^{n k0}
#pragma unroll
    for (int k = 1; k < R0; ++k) { double2 t = twiddle[n1 * k]; if (INVERSE) t.y = -t.y; a[k] = cmul(a[k], t); }
    if (actA) {
#pragma unroll
        for (int k = 0; k < R0; ++k) pA[P0 * k] = a[k];
    }
    __syncthreads();
    double2 b[R1];
#pragma unroll
    for (int s = 0; s < R1; ++s) b[s] = act2 ? pB[R2 * s] : zero;
    dft_small<R1, INVERSE>(b);                                // stage 2 over s -> k1, times W_M1^{n'' k1}
#pragma unroll
    for (int k = 1; k < R1; ++k) { double2 t = twS[nn * k]; if (INVERSE) t.y = -t.y; b[k] = cmul(b[k], t); }
    if (act2) {
#pragma unroll
        for (int k = 0; k < R1; ++k) pB[P1 * k] = b[k];
    }
    __builtin_amdgcn_wave_barrier();
    double2 v[R2];
#pragma unroll
    for (int n = 0; n < R2; ++n) v[n] = pC[n];
    __builtin_amdgcn_wave_barrier();
    dft_small<R2, INVERSE>(v);                                // stage 3 over n'' -> k2
#pragma unroll
    for (int k2 = 0; k2 < R2; ++k2) pN[72 * k2] = v[k2];
    __syncthreads();
    if (actA && q < kv) {
#pragma unroll
        for (int r = 0; r < R0; ++r) {
            if (MAP == 1) *blk(n1 + M1 * r) = pO[PN * r];
            else *reinterpret_cast<double2 *>(base + (size_t)(o0 + (unsigned)(M1 * r) * row16)) = pO[PN * r];
        }
    }
}
template <int N, int R0, int R1, int KB, int P0, int P1, int CS>
static void launch_yfft_regs_slab(double2 *cgrid, double2 *blocks, DGrid G, int nyl, bool inverse, const double2 *tw, hipStream_t s) {
    const size_t lds = (size_t)(KB * CS + N / R0) * sizeof(double2);
    const int nkb = (G.Nzh + KB - 1) / KB, nplanes = 3 * G.nxl;
    const size_t ps = (size_t)G.Ny * G.Nzp;
    const dim3 g(nplanes * nkb), b(64 * KB);
    if (inverse) launch_lds<k_yfft_regs<N, R0, R1, KB, true, P0, P1, CS, 2>>(g, b, lds, s, cgrid, tw, nkb, G.Nzh, G.Nzp, ps, blocks, G.nxl, nyl);
    else launch_lds<k_yfft_regs<N, R0, R1, KB, false, P0, P1, CS, 1>>(g, b, lds, s, cgrid, tw, nkb, G.Nzh, G.Nzp, ps, blocks, G.nxl, nyl);
}
template <int N, int R0, int R1, int KB, int P0, int P1, int CS>
static void launch_yfft_regs(double2 *data, const double2 *tw, int nplanes, int Nzh, int Nzp, size_t plane_stride, bool inverse, hipStream_t s) {
    const size_t lds = (size_t)(KB * CS + N / R0) * sizeof(double2);
    const int nkb = (Nzh + KB - 1) / KB;
    const dim3 g(nplanes * nkb), b(64 * KB);
    if (inverse) launch_lds<k_yfft_regs<N, R0, R1, KB, true, P0, P1, CS>>(g, b, lds, s, data, tw, nkb, Nzh, Nzp, plane_stride, nullptr, 0, 0);
    else launch_lds<k_yfft_regs<N, R0, R1, KB, false, P0, P1, CS>>(g, b, lds, s, data, tw, nkb, Nzh, Nzp, plane_stride, nullptr, 0, 0);
}
// 256^3: forward 0.30 against 0.31 - 0.32 ms, inverse 0.32 against 0.34 (rocFFT's 2-D plan).  Not at 512: the pass itself equals rocFFT's
// strided one there (2.6 ms per direction either way), and rocFFT's 1-D real forward transform of 512 points, which would replace
// the z half of its 2-D plan, is slow (3.7 ms per direction at 512^3 instead of 2.6).
// Round 5: with the own z pass (k_zfft_rows) the register y pass also runs at 512 (8 x 8 x 8, four columns per workgroup).
bool yfft_regs_supported(int Ny, int Nz, bool own_z) { return (Ny == 256 && Nz <= 256) || (own_z && (Ny == 256 || Ny == 512)); }

static bool yfft_slab_regs(double2 *cgrid, double2 *blocks, DGrid G, int nyl, bool inverse, const double2 *tw, hipStream_t s) {
    if (G.Ny == 256) { launch_yfft_regs_slab<256, 8, 8, 8, 44, 5, 359>(cgrid, blocks, G, nyl, inverse, tw, s); return true; }
    if (G.Ny == 512) { launch_yfft_regs_slab<512, 8, 8, 4, 72, 9, 578>(cgrid, blocks, G, nyl, inverse, tw, s); return true; }
    return false;
}
// all three components: [3 Nx] planes of [Ny][Nzp]; tw[m] = exp(-2 pi i m / Ny)
// the kernel launch_yfft takes (also what pse_debug_fft_path reports): the register pass at 256 and, with the own z pass, at 512; k_fft_cols
// with kb = 2, 4 or 8 columns otherwise, by a compile-time plan where one exists (four columns, the sizes of the x pass)
FftChoice yfft_choice(const DGrid &G, int kb) {
    if (G.Ny == 256) return {YFFT_REGS, 8};   // (four columns: +3 %)
    if (G.Ny == 512 && yfft_regs_supported(G.Ny, G.Nz, zfft_supported(G.Nz))) return {YFFT_REGS, 4};
    if (kb == 8 || kb == 2) return {YFFT_COLS_RT, kb};
    if (kb == 4 && (G.Ny == 360 || G.Ny == 270 || G.Ny == 375 || G.Ny == 500)) return {YFFT_COLS_CT, 4};
    return {YFFT_COLS_RT, 4};
}
void launch_yfft(double2 *spectra, DGrid G, bool inverse, const double2 *tw, hipStream_t s, int kb) {
    FftPlanX pl;
    plan_x(G.Ny, pl);
    const int nplanes = 3 * G.nxl;
    const size_t ps = (size_t)G.Ny * G.Nzp;
    const FftChoice c = yfft_choice(G, kb);
    if (c.kernel == YFFT_REGS) {
        if (G.Ny == 256) launch_yfft_regs<256, 8, 8, 8, 44, 5, 359>(spectra, tw, nplanes, G.Nzh, G.Nzp, ps, inverse, s);
        else launch_yfft_regs<512, 8, 8, 4, 72, 9, 578>(spectra, tw, nplanes, G.Nzh, G.Nzp, ps, inverse, s);
    } else if (c.kernel == YFFT_COLS_CT) {   // compile-time plans, as in the x pass
        if (G.Ny == 360) launch_fft_cols<4, 256, CtPlan<360, 9, 8, 5>>(spectra, pl, tw, nplanes, G.Nzh, G.Nzp, ps, inverse, s);
        else if (G.Ny == 270) launch_fft_cols<4, 256, CtPlan<270, 9, 5, 3, 2>>(spectra, pl, tw, nplanes, G.Nzh, G.Nzp, ps, inverse, s);
        else if (G.Ny == 375) launch_fft_cols<4, 256, CtPlan<375, 5, 5, 5, 3>>(spectra, pl, tw, nplanes, G.Nzh, G.Nzp, ps, inverse, s);
        else launch_fft_cols<4, 256, CtPlan<500, 5, 5, 5, 4>>(spectra, pl, tw, nplanes, G.Nzh, G.Nzp, ps, inverse, s);
    } else if (c.kb == 8) launch_fft_cols<8, 256>(spectra, pl, tw, nplanes, G.Nzh, G.Nzp, ps, inverse, s);
    else if (c.kb == 2) launch_fft_cols<2, 256>(spectra, pl, tw, nplanes, G.Nzh, G.Nzp, ps, inverse, s);
    else launch_fft_cols<4, 256>(spectra, pl, tw, nplanes, G.Nzh, G.Nzp, ps, inverse, s);
}

// ---- the z pass: real rows <-> half spectra, one wavefront per row (round 5) -----------------------------------------------------
// rocFFT's 1-D real transforms take two kernels per direction (a complex transform of half the length + an r2c / c2r step) and,
// at 512 points, run well below the rate of its 2-D plan.  Here a wavefront owns a row: its N reals are N / 2 = R0 x 8 x 8 complex
// points z[n] = x[2n] + i x[2n + 1], lane l holds z[l + 64 r] (coalesced 16-byte loads of the row as it lies), three register
// stages with two trips through the wave's own LDS column (no workgroup barrier anywhere), then the real <-> half-spectrum step on
// the natural order and coalesced stores: the row crosses HBM once each way.  Unnormalised both ways, like rocFFT's real plans;
// tools/debug/zfft_model.py is the index algebra in NumPy, checked against numpy.fft.
//   forward:  X[k] = (Z[k] + conj Z[NC - k]) / 2 - i/2 W_N^k (Z[k] - conj Z[NC - k]),  k = 0 .. NC      (Z[NC] = Z[0])
//   inverse:  Z[k] = (X[k] + conj X[NC - k]) + i conj W_N^k (X[k] - conj X[NC - k]),   k = 0 .. NC - 1;  x = N x the true inverse
struct ZRows { double *real[3]; double2 *spec[3]; int rows; int Nz, Nzp; };   // `rows` rows per component, consecutive in both arrays
// A wavefront transforms RW = 64 / (8 R0) rows AT ONCE -- stages 2 and 3 are 8 R0 radix-8 butterflies per row, and with one row per
// wave three quarters of the lanes (256 points: half) did arithmetic for nothing: the kernel ran at 3.3 TB/s bound by vector
// instructions, not by memory -- and RPW such groups one after the other with the twiddles of its lanes loaded once.
template <int NC, int R0, bool INVERSE, int RPW>
__global__ void __launch_bounds__(256)
k_zfft_rows(ZRows zr, const double2 *__restrict__ tw /* exp(-2 pi i m / N), m < N = 2 NC */) {
    // a row's column in LDS: the stage layouts and, once stage 3 has read its points, the natural order on top of them
    constexpr int P0 = 72, P1 = 9, CSW = P0 * (R0 - 1) + P1 * 7 + 8, WB = CSW > NC ? CSW : NC, RW = 64 / (8 * R0);
    static_assert(NC == R0 * 64 && (R0 == 2 || R0 == 4) && RPW % RW == 0, "NC = R0 x 8 x 8");
    __shared__ __attribute__((aligned(16))) double2 lds[4 * RW * WB];
    __shared__ __attribute__((aligned(16))) double2 tw2[64];   // W_64^{nn k1} at [nn * 8 + k1]
    typedef double d2v __attribute__((ext_vector_type(2)));
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (threadIdx.x < 64) { double2 t = tw[(2 * NC / 64) * (l >> 3) * (l & 7)]; if (INVERSE) t.y = -t.y; tw2[l] = t; }
    __syncthreads();
    const long total = 3L * zr.rows, row0 = ((long)blockIdx.x * 4 + wv) * RPW;
    if (row0 >= total) return;                                 // (whole waves; nothing below synchronises across waves)
    const int nrow = (int)min((long)RPW, total - row0);
    double2 *const col = lds + wv * RW * WB;                   // + j WB: row j of the group
    double2 t1[R0], tp[R0];                                     // W_NC^{l k0} (stage 1), W_N^{l + 64 q} (the real <-> half-spectrum step)
#pragma unroll
    for (int q = 0; q < R0; ++q) {
        t1[q] = tw[2 * l * q]; tp[q] = tw[l + 64 * q];
        if (INVERSE) { t1[q].y = -t1[q].y; tp[q].y = -tp[q].y; }
    }
    auto rowptrs = [&](long row, double *&xr, double2 *&xs) __attribute__((always_inline)) {
        const int c = (int)(row / zr.rows);
        const long r = row - (long)c * zr.rows;
        xr = zr.real[c] + r * zr.Nz; xs = zr.spec[c] + r * zr.Nzp;
    };
    // stages 2 and 3: lane -> (row of the group, k0, low index)
    const int jrow = l / (8 * R0), tl = l % (8 * R0), k0 = tl >> 3, lo = tl & 7;
    double2 *const mycol = col + jrow * WB;
    for (int i = 0; i < nrow; i += RW) {
        const int ng = min(RW, nrow - i);                       // rows of this group (the last may be short; wave-uniform)
        double2 a[RW][R0];
        if (!INVERSE) {
#pragma unroll
            for (int j = 0; j < RW; ++j) {
                double *xr; double2 *xs;
                rowptrs(row0 + i + min(j, ng - 1), xr, xs);
#pragma unroll
                for (int q = 0; q < R0; ++q) { const d2v t = __builtin_nontemporal_load(reinterpret_cast<const d2v *>(xr) + l + 64 * q); a[j][q] = make_double2(t.x, t.y); }
            }
        } else {
#pragma unroll
            for (int j = 0; j < RW; ++j) {
                double *xr; double2 *xs;
                rowptrs(row0 + i + min(j, ng - 1), xr, xs);
#pragma unroll
                for (int q = 0; q < R0; ++q) {
                    const int k = l + 64 * q;                    // (k = 0 pairs with the Nyquist entry)
                    const d2v t = __builtin_nontemporal_load(reinterpret_cast<const d2v *>(xs) + k), u = __builtin_nontemporal_load(reinterpret_cast<const d2v *>(xs) + (NC - k));
                    const double2 sm = make_double2(t.x + u.x, t.y - u.y), df = make_double2(t.x - u.x, t.y + u.y);   // xk +- conj xc
                    const double2 w = cmul(tp[q], df);           // conj W_N^k (xk - conj xc)
                    a[j][q] = make_double2(sm.x - w.y, sm.y + w.x);   // sm + i w
                }
            }
        }
#pragma unroll
        for (int j = 0; j < RW; ++j) {
            dft_small<R0, INVERSE>(a[j]);                        // stage 1 over r -> k0, times W_NC^{l k0}
#pragma unroll
            for (int q = 1; q < R0; ++q) a[j][q] = cmul(a[j][q], t1[q]);
#pragma unroll
            for (int q = 0; q < R0; ++q) col[j * WB + P0 * q + l] = a[j][q];
        }
        __builtin_amdgcn_wave_barrier();
        double2 b[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) b[s] = mycol[P0 * k0 + lo + 8 * s];
        __builtin_amdgcn_wave_barrier();
        dft_small<8, INVERSE>(b);                                // stage 2 over s -> k1, times W_64^{nn k1}
#pragma unroll
        for (int k1 = 1; k1 < 8; ++k1) b[k1] = cmul(b[k1], tw2[lo * 8 + k1]);
#pragma unroll
        for (int k1 = 0; k1 < 8; ++k1) mycol[P0 * k0 + P1 * k1 + lo] = b[k1];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int n = 0; n < 8; ++n) b[n] = mycol[P0 * k0 + P1 * lo + n];   // lane (row, k0, k1 = lo)
        __builtin_amdgcn_wave_barrier();                         // (the natural order overwrites the stage layout)
        dft_small<8, INVERSE>(b);                                // stage 3 over nn -> k2: Z[k0 + R0 k1 + 8 R0 k2]
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) mycol[k0 + R0 * lo + 8 * R0 * k2] = b[k2];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < RW; ++j) {
            if (j >= ng) break;
            double *xr; double2 *xs;
            rowptrs(row0 + i + j, xr, xs);
            const double2 *nat = col + j * WB;
            if (!INVERSE) {
#pragma unroll
                for (int q = 0; q < R0; ++q) {
                    const int k = l + 64 * q;
                    const double2 zk = nat[k], zc0 = nat[(NC - k) & (NC - 1)];
                    const double2 sm = make_double2(zk.x + zc0.x, zk.y - zc0.y), df = make_double2(zk.x - zc0.x, zk.y + zc0.y);   // zk +- conj zc
                    const double2 t = cmul(tp[q], df);           // W_N^k (zk - conj zc)
                    d2v o; o.x = 0.5 * (sm.x + t.y); o.y = 0.5 * (sm.y - t.x);   // (sm - i t) / 2
                    __builtin_nontemporal_store(o, reinterpret_cast<d2v *>(xs) + k);
                }
                if (l == 0) { const double2 z0 = nat[0]; xs[NC] = make_double2(z0.x - z0.y, 0.0); }
            } else {
                d2v *z = reinterpret_cast<d2v *>(xr);
#pragma unroll
                for (int q = 0; q < R0; ++q) { const double2 t = nat[l + 64 * q]; d2v o; o.x = t.x; o.y = t.y; __builtin_nontemporal_store(o, z + l + 64 * q); }
            }
        }
        __builtin_amdgcn_wave_barrier();                         // (the next group's stage 1 overwrites the columns)
    }
}
constexpr int ZFFT_RPW = 8;
bool zfft_supported(int Nz) { return Nz == 256 || Nz == 512 || zfft_g_supported(Nz); }
int zfft_choice(int Nz) { return Nz == 256 || Nz == 512 ? ZFFT_ROWS : ZFFT_ROWS_G; }
void launch_zfft(double *const real[3], double2 *const spec[3], int rows, int Nz, int Nzp, bool inverse, const double2 *tw, hipStream_t s) {
    if (zfft_choice(Nz) == ZFFT_ROWS_G) { launch_zfft_g(real, spec, rows, Nz, Nzp, inverse, tw, s); return; }
    ZRows zr{};
    for (int c = 0; c < 3; ++c) { zr.real[c] = real[c]; zr.spec[c] = spec[c]; }
    zr.rows = rows; zr.Nz = Nz; zr.Nzp = Nzp;
    const dim3 g((unsigned)((3L * rows + 4 * ZFFT_RPW - 1) / (4 * ZFFT_RPW))), b(256);
    if (Nz == 512) {
        if (inverse) hipLaunchKernelGGL((k_zfft_rows<256, 4, true, ZFFT_RPW>), g, b, 0, s, zr, tw);
        else hipLaunchKernelGGL((k_zfft_rows<256, 4, false, ZFFT_RPW>), g, b, 0, s, zr, tw);
    } else {
        if (inverse) hipLaunchKernelGGL((k_zfft_rows<128, 2, true, ZFFT_RPW>), g, b, 0, s, zr, tw);
        else hipLaunchKernelGGL((k_zfft_rows<128, 2, false, ZFFT_RPW>), g, b, 0, s, zr, tw);
    }
}

bool xfuse_supported(int Nx) {   // 2^a 3^b 5^c, 16..512
    FftPlanX pl;
    return Nx >= 16 && Nx <= 512 && plan_x(Nx, pl);
}

template <int LOGN, int KB, int NTH>
static void launch_xfft_t(double2 *X, double2 *Y, double2 *Z, DGrid G, DBox box, ScaleArgs a, const double2 *tw, hipStream_t s) {
    constexpr int N = 1 << LOGN;
    const size_t lds = (size_t)(3 * KB * (N + 1) + N) * sizeof(double2);
    const int nkb = (G.Nzh + KB - 1) / KB;
    const int rows = a.transposed ? a.nyl : G.Ny;
    launch_lds<k_xfft_scale<LOGN, KB, NTH>>(dim3(rows * nkb), dim3(NTH), lds, s, X, Y, Z, G, box, a, tw);
}

// the kernel launch_xfft_scale takes (also what pse_debug_fft_path reports)
FftChoice xfft_choice(const DGrid &G, const ScaleArgs &a) {
    if (G.Nx & (G.Nx - 1)) {   // not a power of two: mixed-radix passes; 4 kz columns per workgroup while two buffers fit
        // (one kz column per workgroup, 128 or 256 threads: 1.34 / 1.35 ms at 360^3 against 1.34 with two columns and 256 threads; two
        // columns with 128 / 192 threads: 1.90 / 1.52 ms -- the pass is bound by instruction issue, not occupancy; variants removed)
        if (!a.runtime_plan) {   // compile-time plans for the sizes of the reference's rule at the BASELINE configurations (PSE_XMIX=1: runtime plan)
            switch (G.Nx) {
                case 360: return {XFFT_REGS, 4};   // 0.80 ms at 360^3 (10 x 6 x 6, no spills at two waves per SIMD; three waves: 66 spilled, 0.97); the passes in LDS: 1.05
                case 270: case 375: case 500: return {XFFT_MIXED_CT, 2};
                case 180: return {XFFT_MIXED_CT, 4};
                default: break;
            }
        }
        return {XFFT_MIXED_RT, G.Nx <= 200 ? 4 : 2};   // four columns, 512 threads, one workgroup per CU: 1.61 against 1.38 ms at 360^3
    }
    // small grids (BASELINE config 2: 64^3): with eight kz columns per workgroup the launch is a single, partly filled wave of
    // workgroups and its duration is one workgroup's latency chain (34 us at 64^3); two columns per workgroup give four times as
    // many, shorter chains (the 32-byte pieces of a line are fetched by neighbouring workgroups of one XCD)
    const int rows_ = a.transposed ? a.nyl : G.Ny;
    if (G.Nx <= 128) return {XFFT_LDS, (long)rows_ * ((G.Nzh + 7) / 8) < 1024 && !a.wide_small ? 2 : 8};   // 8 kz columns per workgroup = 128-byte pieces; LDS = 3*KB*(N+1)*16 B
    return {XFFT_REGS, G.Nx == 256 ? 8 : 4};
}

void launch_xfft_scale(double2 *X, double2 *Y, double2 *Z, DGrid G, DBox box, ScaleArgs a, const double2 *tw, hipStream_t s) {
    // (k_xfft_scale_cols addresses a component with 32-bit byte offsets: 512 x 512 x 264 complex numbers, the largest grid, are 1.1 GB)
    const FftChoice c = xfft_choice(G, a);
    if (c.kernel == XFFT_MIXED_CT || c.kernel == XFFT_MIXED_RT) {
        FftPlanX pl;
        plan_x(G.Nx, pl);
        if (c.kernel == XFFT_MIXED_RT) {
            if (c.kb == 4) launch_xfft_mixed<4, 256>(X, Y, Z, G, box, a, tw, pl, s);
            else launch_xfft_mixed<2, 256>(X, Y, Z, G, box, a, tw, pl, s);
            return;
        }
        switch (G.Nx) {
            case 270: launch_xfft_mixed<2, 256, CtPlan<270, 9, 5, 3, 2>>(X, Y, Z, G, box, a, tw, pl, s); break;
            case 375: launch_xfft_mixed<2, 256, CtPlan<375, 5, 5, 5, 3>>(X, Y, Z, G, box, a, tw, pl, s); break;
            case 500: launch_xfft_mixed<2, 256, CtPlan<500, 5, 5, 5, 4>>(X, Y, Z, G, box, a, tw, pl, s); break;
            default: launch_xfft_mixed<4, 256, CtPlan<180, 9, 5, 4>>(X, Y, Z, G, box, a, tw, pl, s); break;   // 180
        }
        return;
    }
    if (c.kernel == XFFT_LDS) {
        if (c.kb == 2) {
            switch (G.Nx) {
                case 16: launch_xfft_t<4, 2, 64>(X, Y, Z, G, box, a, tw, s); break;
                case 32: launch_xfft_t<5, 2, 64>(X, Y, Z, G, box, a, tw, s); break;
                case 64: launch_xfft_t<6, 2, 128>(X, Y, Z, G, box, a, tw, s); break;
                default: launch_xfft_t<7, 2, 256>(X, Y, Z, G, box, a, tw, s); break;   // 128
            }
            return;
        }
        switch (G.Nx) {
            case 16: launch_xfft_t<4, 8, 256>(X, Y, Z, G, box, a, tw, s); break;
            case 32: launch_xfft_t<5, 8, 256>(X, Y, Z, G, box, a, tw, s); break;
            case 64: launch_xfft_t<6, 8, 256>(X, Y, Z, G, box, a, tw, s); break;
            default: launch_xfft_t<7, 8, 512>(X, Y, Z, G, box, a, tw, s); break;   // 128
        }
        return;
    }
    switch (G.Nx) {   // the register passes
        case 360: launch_xfft_cols<360, 10, 6, 4, 2, false, 54, 9, 538>(X, Y, Z, G, box, a, tw, s); break;
        // 64-byte pieces (four kz): 3.87 TB/s at 256 x 512 x 512; 32-byte pieces (two kz, three workgroups per CU) 2.73; 128-byte pieces with
        // all three components in LDS (eight kz, one workgroup per CU) 2.71
        case 256:
            // 256 = 4 x 8 x 8 with TWO columns per wave: eight kz columns = 128-byte pieces at four waves per workgroup; 256^3: 0.201 against
            // 0.226 ms, with noise 0.214 against 0.243 (256 = 8 x 8 x 4 with one column per wave and 64-byte pieces only tied: 0.25 - 0.27)
            launch_xfft_cols<256, 4, 8, 8, 3, true, 72, 9, 295, 2>(X, Y, Z, G, box, a, tw, s);
            break;
        // 512: radix 16, 16, 2; two kz columns: three workgroups per CU (3.3 ms at 512^3; four columns, one workgroup: 3.8; radix 4/2 in LDS: 5.2)
        default:
            // one component in LDS at a time, four kz columns, three workgroups per CU: 1.50 ms at 512^3 (4.3 TB/s); eight columns at four
            // waves per SIMD (128 registers: 225 spilled) 3.3 ms, six columns 2.9 ms, four columns without parking the third component
            // during the operator (107 spilled) 2.27 ms; all three components in LDS, two columns (k_xfft_scale256, removed in round 5): 2.77 ms
            launch_xfft_cols<512, 8, 8, 4, 3, true, 72, 9, 578>(X, Y, Z, G, box, a, tw, s);
            break;
    }
}

// ------------------------------------------------------------------------------------------------ slab transposes
// Slab-decomposed far field (new design; the reference is single-GPU, PSEv1/Stokes.cc:104).  After the local 2-D
// transforms rank r holds [3][nxl][Ny][Nzh]; the block of y rows [q*nyl, (q+1)*nyl) goes to rank q.  pack lays the
// half spectrum out as [3][G][nxl][nyl][Nzh] so each destination's block is contiguous; on the receiving side the blocks
// of all source ranks line up as [3][Nx][nyl][Nzh] (x-major) with no further copy.  unpack is the inverse map.
__global__ void k_slab_pack(const double2 *__restrict__ cgrid, double2 *__restrict__ buf, int nxl, int Ny, int Nzh,
                            int nyl, int unpack) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)nxl * Ny * Nzh;
    if (tid >= 3 * per) return;
    const int c = (int)(tid / per);
    size_t r = tid - (size_t)c * per;
    const int k = (int)(r % Nzh); r /= Nzh;
    const int j = (int)(r % Ny);
    const int lx = (int)(r / Ny);
    const int q = j / nyl, jl = j - q * nyl;
    const size_t o = (size_t)c * per + (((size_t)q * nxl + lx) * nyl + jl) * Nzh + k;
    if (unpack) ((double2 *)cgrid)[tid] = buf[o];
    else buf[o] = cgrid[tid];
}
void launch_slab_pack(double2 *cgrid, double2 *buf, int nxl, int Ny, int Nzh, int nyl, int unpack, hipStream_t s) {
    const size_t n = (size_t)3 * nxl * Ny * Nzh;
    hipLaunchKernelGGL(k_slab_pack, dim3(nblocks((long)n, TPB)), dim3(TPB), 0, s, cgrid, buf, nxl, Ny, Nzh, nyl, unpack);
}

}  // namespace pse
