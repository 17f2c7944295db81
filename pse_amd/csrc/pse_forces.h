// Launch wrappers of the force providers' kernels (defined in pse_forces.hip).  All take the stream explicitly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pse_device.h"

namespace pse {

// soft pair repulsion from the cell list, scattered to the caller's order (force provider).  out8 != null: the same
// pass + the pair observables U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, npairs over the rows j > i: one row of PAIR_VIRIAL_NOBS doubles
// per workgroup into `rows` (pair_virial_rows(N) doubles), added up in a fixed order into out8 (device) by a second, one-workgroup
// kernel; force may then be null (observables only).  out8 == null: forces only, no reduction (rows is not touched)
constexpr int PAIR_VIRIAL_NOBS = 8;
size_t pair_virial_rows(int n);
// pair exclusions of the two cell-list passes (pse_exclusions_create): the device copy of the rows of pse_host_exclusion_rows, a CSR
// over the first n caller-order indices, row t = entries[row_off[t] .. row_off[t + 1]) the partners excluded from t, ascending.
// ex != null: the pairs in it contribute nothing to forces or sums (k_pair_repulsion<OBS, true>, k_pair_table<OBS, true>); ex == null:
// the plain kernels
struct PairExclusions {
    const unsigned *row_off, *entries;
    unsigned n;
};
void launch_pair_repulsion(const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc,
                           double k, double sigma, int accumulate, double4 *force, double *rows, double *out8, hipStream_t s,
                           const PairExclusions *ex = nullptr);
// tabulated central pair potential from the cell list (k_pair_table): table = width x (V, F) on the device, 16-byte aligned, nodes
// r_e = rmin + e (rmax - rmin)/(width - 1), linear between them, staged in width * 16 bytes of LDS per workgroup.  out8 != null: the
// eight observables through `rows` as above; out8 == null: forces only, no reduction (rows is not touched)
void launch_pair_table(const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc, const double *table,
                       int width, double rmin, double rmax, int accumulate, double4 *force, double *rows, double *out8, hipStream_t s,
                       const PairExclusions *ex = nullptr);
// typed pair tables (k_pair_table_typed; pse_typed_table_create): the device arrays of one object.  types: n bytes, the type of
// caller-order particle t (a tag >= n acts as type 0); type_s: room for one byte per sorted row, written by every launch behind the
// sort (k_type_mirror); tables: total x (V, F), the pair types' tables one after another, 16-byte aligned, staged in total * 16 bytes
// of LDS; par: two 16-byte words per pair type, (rmin, rmax^2) and (scale, {base, width - 2} as two ints in one double's bits), an
// off pair type with rmax^2 = 0; rmax2_all: the largest rmax^2, the wave-uniform prefilter.  rows, out8, ex as for launch_pair_table
constexpr int PAIR_TYPED_MAX_PAIR_TYPES = pse::PAIR_TYPED_MAX_TYPES * (pse::PAIR_TYPED_MAX_TYPES + 1) / 2;
struct PairTypedTables {
    const unsigned char *types;
    unsigned char *type_s;
    const double *tables, *par;
    unsigned n;
    int ntypes, total;
    double rmax2_all;
};
// the type mirror of the typed cell-list passes (k_type_mirror): type_s[i] = types[tag_s[i]], 0 for a tag >= n
void launch_type_mirror(const unsigned *tag_s, int N, const unsigned char *types, unsigned n, unsigned char *type_s, hipStream_t s);
void launch_pair_table_typed(const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc,
                             const PairTypedTables &tt, int accumulate, double4 *force, double *rows, double *out8, hipStream_t s,
                             const PairExclusions *ex = nullptr);
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
// bonded forces (k_bond_forces): one row of (partner, type) entries per particle of the caller-order arrays, row i =
// entries[row_off[i] .. row_off[i + 1]), sorted (pse_host_bond_rows); par = ntypes <= BOND_MAX_TYPES parameter sets.  out8 != null: the
// eight observables through `rows` (pair_virial_rows(n) doubles) as above; out8 == null: forces only.  A FENE bond at r >= r0 does
// not act and adds one to *overstretched.
struct BondParam {   // 32 bytes, staged in LDS as two 16-byte words (the device array is a hipMalloc of its own: aligned)
    double k, r0;
    double ir02;     // 1 / r0^2 (FENE; 0 where r0 = 0)
    double kind;     // PSE_BOND_HARMONIC or PSE_BOND_FENE as a double
};
void launch_bond_forces(const double4 *pos, int n, const unsigned *row_off, const uint2 *entries, const BondParam *par, int ntypes, DBox box,
                        int accumulate, double4 *force, double *rows, double *out8, unsigned long long *overstretched, hipStream_t s);
// angle forces (k_angle_forces): one row of (i, j, k, type) entries per particle of the caller-order arrays, row p =
// entries[row_off[p] .. row_off[p + 1]), j the vertex, i < k, sorted (pse_host_angle_rows); par = ntypes <= ANGLE_MAX_TYPES parameter
// sets.  out8 != null: the eight observables through `rows` (pair_virial_rows(n) doubles) as above; out8 == null: forces only.
struct AngleParam {   // 32 bytes, staged in LDS as two 16-byte words (the device array is a hipMalloc of its own: aligned)
    double k, theta0;
    double cos0;     // cos(theta0)
    double kind;     // PSE_ANGLE_HARMONIC or PSE_ANGLE_COSINESQ as a double
};
void launch_angle_forces(const double4 *pos, int n, const int *row_off, const uint4 *entries, const AngleParam *par, int ntypes, DBox box,
                         int accumulate, double4 *force, double *rows, double *out8, hipStream_t s);
// dihedral forces (k_dihedral_forces): one row of (i, j, k, l) entries per particle of the caller-order arrays, row p =
// entries[row_off[p] .. row_off[p + 1]), i < l, sorted, and types[e] the type of entry e (the two sections pse_host_dihedral_rows
// writes: 16 + 4 bytes per entry); par = ntypes <= DIHEDRAL_MAX_TYPES parameter sets.  out8 != null: the eight observables through
// `rows` (pair_virial_rows(n) doubles) as above; out8 == null: forces only.
struct DihedralParam {   // 48 bytes, staged in LDS as three 16-byte words (the device array is a hipMalloc of its own: aligned)
    double p0, p1;   // harmonic: k/2, d cos(phi0);  OPLS: k1, k2
    double p2, p3;   // harmonic: d sin(phi0), 0;    OPLS: k3, k4
    double mult;     // harmonic: the multiplicity 1..6 as a double;  OPLS: 0, which is how the kernel tells the kinds apart
    double pad;
};
void launch_dihedral_forces(const double4 *pos, int n, const int *row_off, const uint4 *entries, const unsigned *types,
                            const DihedralParam *par, int ntypes, DBox box, int accumulate, double4 *force, double *rows, double *out8,
                            hipStream_t s);

}  // namespace pse
