// Launch wrappers of the transform kernels (defined in pse_fft.hip; the general z pass in pse_zfft.hip).  All take the stream explicitly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pse_device.h"

namespace pse {

struct ScaleArgs {
    double xi, eta;
    int noise;               // add k-space Brownian noise (K6)
    double noise_fac;        // sqrt(2 kT / (dt h^3))
    uint32_t seed, timestep;
    const uint32_t *ts_off;  // nullable: the noise is drawn at timestep + *ts_off, read on the device (pse_set_timestep_offset)
    int transposed;          // layout [Nx][ny_local][Nzh] (slab mode, after the transpose) instead of [nx_local][Ny][Nzh]
    int y0, nyl;             // slab of y rows in transposed layout
    int runtime_plan;        // PSE_XMIX=1: the runtime radix plan also where a compile-time one exists (A/B)
    int wide_small;          // PSE_XFFT_SMALL_KB=8: eight kz columns per workgroup also on small grids (A/B)
};
void launch_scale(double2 *X, double2 *Y, double2 *Z, DGrid G, DBox box, ScaleArgs a, hipStream_t s);
// debug: kx, ky, kz, w sinc^2, sqrt(w) sinc of n nodes (i, j, k)
void launch_debug_kop(const int *ijk, int n, DGrid G, DBox box, double xi, double eta, double *out, hipStream_t s);
// fused forward-x FFT + scale + inverse-x FFT on [3][Nx][Ny][Nzh] (Nx a power of two, 16..512); tw[m] = exp(-2 pi i m/Nx)
bool xfuse_supported(int Nx);
// own in-place y transforms of the half spectra [3 nxl][Ny][Nzp] (Ny = 2^a 3^b 5^c, not a power of two); tw[m] = exp(-2 pi i m / Ny);
// kb: consecutive kz per workgroup (2, 4 or 8)
bool yfft_supported(int Ny);
bool yfft_regs_supported(int Ny, int Nz, bool own_z = false);   // the register y pass (k_yfft_regs) instead of rocFFT's strided pass: 256 (Nz <= 256), and 256 / 512 with the own z pass
// a slab rank's y transforms with the reordering of the all-to-all blocks folded in: forward reads the planes [3][nxl][Ny][Nzp] and writes
// [3][G][nxl][nyl][Nzp]; inverse the other way round (any Ny = 2^a 3^b 5^c in 16..512: yfft_possible)
bool yfft_possible(int Ny);
void launch_yfft_slab(double2 *cgrid, double2 *blocks, DGrid G, int nyl, bool inverse, const double2 *tw, hipStream_t s,
                      bool regs = true);   // regs: Ny = 256, 512 by the register pass (k_yfft_regs with the block map) instead of k_fft_cols
void launch_yfft(double2 *spectra, DGrid G, bool inverse, const double2 *tw, hipStream_t s, int kb = 4);
// own z pass (k_zfft_rows): `rows` real rows of Nz doubles per component <-> spectrum rows of Nzp complex numbers; tw[m] = exp(-2 pi i m / Nz)
bool zfft_supported(int Nz);
void launch_zfft(double *const real[3], double2 *const spec[3], int rows, int Nz, int Nzp, bool inverse, const double2 *tw, hipStream_t s);
bool zfft_g_supported(int Nz);   // pse_zfft.hip: NC = R0 x R1 x R2 (360, 270, 180, ...); launch_zfft calls launch_zfft_g at those sizes
void launch_zfft_g(double *const real[3], double2 *const spec[3], int rows, int Nz, int Nzp, bool inverse, const double2 *tw, hipStream_t s);
void launch_xfft_scale(double2 *X, double2 *Y, double2 *Z, DGrid G, DBox box, ScaleArgs a, const double2 *tw, hipStream_t s);

// Which kernel family a transform launcher takes, and its kz columns per workgroup (pse_debug_fft_path).  launch_xfft_scale, launch_yfft
// and launch_zfft switch on what these return, so the report cannot name another kernel than the one launched.  FFT_ROCFFT is never
// returned: it is what the handle reports for an axis whose launcher is not called (xfuse / own_y / own_z off).
enum { FFT_ROCFFT = 0,
       XFFT_LDS = 1, XFFT_REGS = 2, XFFT_MIXED_CT = 3, XFFT_MIXED_RT = 4,      // k_xfft_scale, k_xfft_scale_cols, k_xfft_scale_mixed with a compile-time / runtime plan
       YFFT_COLS_CT = 1, YFFT_COLS_RT = 2, YFFT_REGS = 3,                     // k_fft_cols with a compile-time / runtime plan, k_yfft_regs
       ZFFT_ROWS = 1, ZFFT_ROWS_G = 2 };                                      // k_zfft_rows (256, 512), k_zfft_rows_g (pse_zfft.hip)
struct FftChoice { int kernel, kb; };
FftChoice xfft_choice(const DGrid &G, const ScaleArgs &a);
FftChoice yfft_choice(const DGrid &G, int kb);
int zfft_choice(int Nz);

// slab ranks: the pack / unpack of the all-to-all blocks as a pass of its own (launch_yfft_slab folds it into the y transform)
void launch_slab_pack(double2 *cgrid, double2 *buf, int nxl, int Ny, int Nzh, int nyl, int unpack, hipStream_t s);

}  // namespace pse
