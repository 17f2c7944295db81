// Launch wrappers of the force providers' kernels (defined in pse_forces.hip).  All take the stream explicitly.  The analyses'
// wrappers are in pse_analysis.h and pse_order.h, which include this header for PairExclusions and the type mirror.
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
