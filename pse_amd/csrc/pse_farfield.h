// Launch wrappers of the far-field kernels K2-K8 (defined in pse_farfield.hip).  All take the stream explicitly.
#pragma once
#include "pse_kernels.h"

namespace pse {

// scratch of the fast far-field path (rebuilt every call): particles binned by the 8^3 block of nodes their support
// origin lies in, and their records written in bin order
struct FarBins {
    int nbx, nby, nbz;          // bins per axis (set by the launchers from the grid)
    int *cnt, *off;             // [nbins], [nbins + 1]
    int *rank_s;                // [N] rank of a particle inside its bin (-1: not needed by this slab rank)
    void *tmp; size_t tmp_bytes;   // scan scratch
};
size_t bin_scan_temp_bytes(size_t nbins);
struct FarRec;                  // 64-byte bin-ordered particle record (pse_farfield.hip)
struct SpreadWork {
    FarBins fb;
    FarRec *rec_t;              // [N] bin order: origin, sorted index (bit 31: owned by another slab rank), offset, prefac * force
    int force_tz, force_nw;     // tuning switches of the handle (0: automatic): z depth of a spread block, waves per block
    int force_bz;               // ... bins along z per gather workgroup (PSE_GATHER_BZ=1|2)
    CellRanges need;            // a slab rank: rows outside hold no particle data (their support cannot reach the slab)
    const int *cell_off;
    int rows_local;             // 1: N counts the rows of ONE slab rank (owned-particle teams), not the particles of the suspension
};
// per-step constants of the separable Gaussian weights: step ratios r_t = exp(-c h^2 (2t+1)) (y with the (1 + xy^2) of the
// sheared lattice), ln K = -2 c xy hx hy, the tilt
constexpr int FAR_PMAX = 14;   // largest support of the block far field (error 1e-6 gives P = 13)
struct GaussConsts { double rx[FAR_PMAX - 1], ry[FAR_PMAX - 1], rz[FAR_PMAX - 1], lnk, s; };
size_t farfield_bins(const DGrid &G);
// true if the caller must zero the grids first (atomic fallback: P outside 4..8 or a grid smaller than two tiles)
bool spread_needs_zero(const DGrid &G);
// The far field of a step: (1) the pass that gathers the particles into cell order (launch_permute) ranks every particle inside
// its bin (FarBinArgs; the bin counts are zeroed by the caller before it); (2) launch_far_records: bin offsets + the 64-byte
// records in bin order; (3) launch_spread; ... (4) launch_gather, which reads the same records.
struct FarBinArgs { bool on; DGrid G; FarBins fb; };
FarBinArgs far_bin_args(const DGrid &G, const SpreadWork &w);
size_t far_bin_count(const DGrid &G);   // ints of fb.cnt to zero
hipError_t launch_far_records(const double4 *pos_s, const double4 *f_s, int N, DGrid G, DBox box, SpreadWork w, hipStream_t s);
hipError_t launch_spread(const double4 *pos_s, const double4 *f_s, int N, double *gx, double *gy, double *gz, DGrid G,
                   DBox box, SpreadWork w, hipStream_t s);
// the fast path reads the records written by launch_spread of the same step
hipError_t launch_gather(const double4 *pos_s, SpreadWork w, int N, const double *gx, const double *gy, const double *gz, DGrid G,
                   DBox box, double4 *u_s, hipStream_t s);

// which kernels launch_spread / launch_gather would launch for N particles (pse_debug_far_path): decided by the functions the launchers call
void far_path(const DGrid &G, const SpreadWork &w, int N, double xy, int out[6]);

}  // namespace pse
