// Launch wrappers of the analysis kernels (defined in pse_analysis.hip).  All take the stream explicitly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pse_forces.h"

namespace pse {

// pair-distance histogram (k_pair_hist; pse_pair_hist_create): the device arrays and the bins of one object.  types, type_s: as in
// PairTypedTables (type_s is written by every launch, k_type_mirror).  Every unordered pair of sorted rows with rmin <= r, r^2 < rmax^2,
// r > 0 that is not in `ex` adds 1 to counts[p nbins + b]: p the pair type p(a, b), b = min((int)((r - rmin) scale), nbins - 1),
// scale = nbins/(rmax - rmin).  counts (device, npt x nbins) is ADDED to with integer atomics: exact, whatever the order.
struct PairHist {
    const unsigned char *types;
    unsigned char *type_s;
    unsigned n;
    int ntypes, nbins;
    double rmin, rmax;
};
void launch_pair_hist(const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc, const PairHist &ph,
                      unsigned long long *counts, hipStream_t s, const PairExclusions *ex = nullptr);
// static structure factor (k_sf_partial, k_sf_finish; pse_structure_factor_create): the device arrays of one object.  types: n bytes
// as in PairTypedTables (a caller index >= n acts as type 0); segs: two int4 per segment of the mode plan (structure_factor_plan):
// (m0x, m0y, m0z, len), (dx, dy, dz, first); perm: nk, the caller's indices in the canonical order, uoff: nu + 1, where the u-th of the nu
// DISTINCT modes begins in perm (its value goes to every caller index there); rows: the workspace of sf_workspace(n_max, ntypes, nk)
// complex numbers, one row of nu per (span of `span` particles, type); span = sf_span(n_max, ntypes, nk),
// a multiple of the staged chunk, the smallest with which the workspace stays within 256 MB.  rho (ntypes x nk x 2, overwritten) and
// sums (npt x nk, added to) are the caller's device arrays in its order of the modes, either may be null.
struct StructureFactor {
    const unsigned char *types;
    unsigned n;
    int ntypes;
    const int4 *segs;
    int nseg, nlong;   // segments in all, and those of more than SF_SHORT modes, which come first
    const unsigned *perm, *uoff;
    int nu, nk;
    double2 *rows;
    int span;
};
int sf_span(unsigned n_max, int ntypes, int nk);
size_t sf_workspace(unsigned n_max, int ntypes, int nk);
void launch_structure_factor(const double4 *pos, const unsigned *group, int N, DBox box, const StructureFactor &sf, double *rho, double *sums,
                             hipStream_t s);
// displacement moments (k_msd_store, k_msd_partial, k_msd_finish; pse_msd_create): the device arrays of one object.  types: n bytes as
// in PairTypedTables (a caller index >= n acts as type 0); planes: norigins slots of three planes (x, y, z) of n_max doubles each,
// plane c of slot s at planes + (3 s + c) n_max, indexed by the caller-order particle index: a lane's loads are 8 bytes and, with an
// identity group, consecutive; part: the workspace, one row of MSD_MOMENTS doubles per (wave of 256 particles, listed pair, type).
// Lx, Ly, Lz: the box lengths, sLy = strain Ly (formed on the host).  A caller index >= n_max is skipped (nothing read, nothing written).
struct MsdOrigins {
    const unsigned char *types;
    unsigned n;
    int ntypes;
    double *planes;
    size_t n_max;
    double *part;
};
// the pairs of one pse_msd_accumulate, by value in the kernel arguments: slot[q] the origin, row[q] the row of sums
struct MsdPairs {
    int npairs;
    unsigned char slot[MSD_MAX_ORIGINS];
    int row[MSD_MAX_ORIGINS];
};
size_t msd_workspace(unsigned n_max, int ntypes);   // doubles: rows for MSD_MAX_ORIGINS listed pairs, whatever the number of slots
// out == null: r_u of the group members into `slot`; out != null: out[t] = (d.xyz, |d|^2) against `slot`, nothing stored
void launch_msd_store(const double4 *pos, const int3 *image, const unsigned *group, int N, double Lx, double Ly, double Lz, double sLy,
                      const MsdOrigins &mo, int slot, double4 *out, hipStream_t s);
void launch_msd_accumulate(const double4 *pos, const int3 *image, const unsigned *group, int N, double Lx, double Ly, double Lz, double sLy,
                           const MsdOrigins &mo, const MsdPairs &pairs, double *sums, hipStream_t s);
// cluster analysis (pse_clusters_label): the device arrays and the link distances of one object.  types, type_s: as in PairHist.
// rlink2: npt squares of the link distances (0: off), rl2_all the largest; parent, mintag, csize: n_max unsigned words each, the
// union-find over the sorted rows, rewritten by every call; status: the object's sticky word (a trip cap was reached).  Two sorted rows
// are linked when 0 < r^2 < rlink2[p] and the pair is not in `ex`; label and size are written by caller index (tag_s), stats (four
// words) is overwritten, hist (nhist words) is added to with integer atomics; each may be null.
struct ClusterLinks {
    const unsigned char *types;
    unsigned char *type_s;
    unsigned n;
    int ntypes;
    const double *rlink2;
    double rl2_all;
    unsigned *parent, *mintag, *csize, *status;
};
void launch_clusters(const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc, const ClusterLinks &cl,
                     unsigned *label, unsigned *size, unsigned long long *stats, unsigned long long *hist, unsigned nhist, hipStream_t s,
                     const PairExclusions *ex = nullptr);

}  // namespace pse
