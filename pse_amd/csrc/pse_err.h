// Error state of the C-ABI (include/pse_amd.h: every entry point returns a status, the message is read with
// pse_last_error()).  Defined in pse_host_api.cpp, which holds everything of the C-ABI that needs no device -- so that the
// host-only entry points, the parameter rule and the tridiagonal solver can also be built for the CPU sanitizers
// (python -m pse_amd.build --asan).
#pragma once
#include <string>
#include <vector>

#include "../../include/pse_amd.h"
#include "pse_host.h"

namespace pse {

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));   // records the message, returns code
std::string &error_text();                                                          // thread-local
void fill_info(const Derived &d, pse_info *o);
// 0, or PSE_ERR_INVALID with a message: the spreading Gaussian of these parameters leaves the double range over its support on the
// coarsest of the three grid spacings (an override the reference's rule cannot produce) -- shared by pse_create, pse_set_box,
// pse_host_select_params and the sanitizer build's stand-in, so that all agree on which configurations are valid
int gaussian_fits(const Derived &d, double hx, double hy, double hz);
// 0, or PSE_ERR_INVALID with a message under the name `who`: what pse_host_lz_decide and pse_debug_lz_decide refuse alike -- a null
// array, n_dec outside [1, 40], a first decision without `first`, and per decision anything but 1 <= m_lo <= m_hi <= done_iters <=
// M_MAX, pending_beta in [0, m_hi], m_max <= M_MAX (the device entry point adds what its kernel is sized for)
int lz_decisions_validate(const char *who, const double *scal_host, int n_dec, const pse_debug_lz_decision *dec, const void *out);
// what the two entry points hand on and hand back: a decision of the C-ABI as the contract's, a state as the C-ABI's outcome (mirror aside)
LzDecide lz_decision(const pse_debug_lz_decision &d);
void lz_outcome(const LzState &st, pse_debug_lz_outcome *o);
// 0, or PSE_ERR_INVALID with a message: the argument checks of pse_pair_repulsion (virial = false) and pse_pair_repulsion_virial
// (virial = true) behind the null-handle check, with the handle's rcut, n_max and n_slabs -- shared by the device library and the
// sanitizer build's stand-in, in the order include/pse_amd.h promises
int pair_repulsion_validate(double rcut, unsigned n_max, int n_slabs, unsigned N, const void *pos, const void *force, bool virial,
                            const void *out8, double sigma);
// the same for pse_pair_table
int pair_table_validate(double rcut, unsigned n_max, int n_slabs, unsigned N, const void *pos, const void *force, const double *table, int width,
                        double rmin, double rmax, const void *out8);
// 0, or PSE_ERR_INVALID with a message naming the offending value: the argument checks of pse_bonds_create that need no device
// (include/pse_amd.h lists them) -- shared by the device library and the sanitizer build's stand-in
int bonds_validate(unsigned n_max, unsigned n, unsigned nbonds, const unsigned *pairs, const unsigned *types, int ntypes, const int *kind,
                   const double *k, const double *r0);
// the same for pse_angles_create
int angles_validate(unsigned n_max, unsigned n, unsigned nangles, const unsigned *triples, const unsigned *types, int ntypes,
                    const int *kind, const double *k, const double *theta0);
// the same for pse_dihedrals_create (params: ntypes x 4)
int dihedrals_validate(unsigned n_max, unsigned n, unsigned ndihedrals, const unsigned *quads, const unsigned *types, int ntypes,
                       const int *kind, const double *params);
// the same for pse_exclusions_create
int exclusions_validate(unsigned n_max, unsigned n, unsigned npairs, const unsigned *pairs);
// what pse_pair_table_excl and pse_pair_repulsion_excl (`who`) check behind the validators of the plain passes: an exclusion object,
// and one of this handle (ex_handle: the handle it was created on)
int pair_excl_validate(const char *who, const void *ex, const void *ex_handle, const void *h);
// the same for pse_typed_table_create behind its null-out and null-handle checks: the null arrays, n, the types, and -- through the
// checks of pse_host_typed_table_layout under the caller's name -- ntypes, the widths, the ranges and the sum of the widths; then
// rmax against rcut and the table entries
int typed_table_validate(double rcut, unsigned n_max, unsigned n, const unsigned *types, int ntypes, const int *width, const double *rmin,
                         const double *rmax, const double *tables);
// the argument checks of pse_pair_table_typed, in the order of pse_pair_table_excl: the object (t_handle: the handle it was created
// on, n_max and n_slabs that handle's), N, pos, force and out8, out8 on a slab rank; then an exclusion object, if one is given, of
// the same handle
int pair_typed_validate(const void *t, const void *t_handle, unsigned n_max, int n_slabs, unsigned N, const void *pos, const void *force,
                        const void *out8, const void *ex, const void *ex_handle);
// the argument checks of pse_pair_hist_create behind its null-out and null-handle checks, in the order include/pse_amd.h lists them
// (types may be null: one type), with the handle's rcut, n_max and n_slabs
int pair_hist_create_validate(double rcut, unsigned n_max, int n_slabs, unsigned n, const unsigned *types, int ntypes, int nbins, double rmin,
                              double rmax);
// the argument checks of pse_pair_hist_accumulate: the object (g_handle: the handle it was created on, n_max that handle's), N, pos,
// counts; then an exclusion object, if one is given, of the same handle
int pair_hist_validate(const void *g, const void *g_handle, unsigned n_max, unsigned N, const void *pos, const void *counts, const void *ex,
                       const void *ex_handle);
// the argument checks of pse_structure_factor_create behind its null-out and null-handle checks, in the order include/pse_amd.h lists
// them (types may be null: one type), with the handle's n_max
int structure_factor_create_validate(unsigned n_max, unsigned n, const unsigned *types, int ntypes, unsigned nk, const int *modes);
// the argument checks of pse_structure_factor_accumulate: the object (n_max its handle's), N, pos, rho and sums
int structure_factor_validate(const void *f, unsigned n_max, unsigned N, const void *pos, const void *rho, const void *sums);
// The plan of a mode list (nk x 3), a function of the mode SET: perm = the caller's indices in the canonical order (ascending mx,
// then my, then mz; equal modes by index); uoff (nu + 1) = where the u-th DISTINCT mode begins in perm -- a duplicate is computed once
// and written to every place that asked for it; and the segments that cover the nu distinct modes in that order: greedy arithmetic
// progressions m0 + t d, d the difference of a segment's first two modes (any integer vector), cut after SF_RUN modes and in front of (0, 0, 0), which is always a seed (rho = N_a exactly).  segs holds
// eight ints per segment: m0x, m0y, m0z, len, dx, dy, dz, first (the position of m0 among the distinct modes); the segments of more
// than SF_SHORT modes come first, the short ones behind them, each class in the canonical order.
void structure_factor_plan(unsigned nk, const int *modes, std::vector<unsigned> &perm, std::vector<unsigned> &uoff, std::vector<int> &segs);
// the argument checks of pse_msd_create behind its null-out and null-handle checks, in the order include/pse_amd.h lists them (types
// may be null: one type), with the handle's n_max
int msd_create_validate(unsigned n_max, unsigned n, const unsigned *types, int ntypes, int norigins);
// the argument checks that pse_msd_store and pse_msd_displacement (`who`) share: the object (norigins its own, n_max its handle's), the
// slot, N, pos, image, strain
int msd_slot_validate(const char *who, const void *m, int norigins, unsigned n_max, int slot, unsigned N, const void *pos, const void *image,
                      double strain);
// what pse_msd_displacement checks behind them: the slot was stored (stored: bit s = slot s holds positions), out
int msd_displacement_validate(unsigned long long stored, int slot, const void *out);
// the argument checks of pse_msd_accumulate
int msd_accumulate_validate(const void *m, int norigins, unsigned long long stored, unsigned n_max, unsigned N, const void *pos,
                            const void *image, double strain, int npairs, const int *slots, const int *rows, int nrows, const void *sums);
// the argument checks of pse_isf_create behind its null-out and null-handle checks: those of pse_structure_factor_create, in its
// order, with nk capped at ISF_MAX_MODES, then norigins
int isf_create_validate(unsigned n_max, unsigned n, const unsigned *types, int ntypes, unsigned nk, const int *modes, int norigins);
// the argument checks of pse_isf_sample, pse_isf_store and pse_isf_correlate, in the order include/pse_amd.h lists them (n_max: the
// handle's; norigins: the object's; sample_N: N of the sample in the current buffer, 0: none since create; slot_N[s]: N of the sample
// stored in slot s, 0: never stored).  A slot holds one sample whole, so the checks of a pair's slot -- in range, stored, the N of the
// current sample -- run over the list one after another, as those of pse_msd_accumulate do
int isf_sample_validate(const void *obj, unsigned n_max, unsigned N, const void *pos, const void *rho, const void *static_sums);
int isf_store_validate(const void *obj, int norigins, unsigned sample_N, int slot);
int isf_correlate_validate(const void *obj, int norigins, unsigned sample_N, const unsigned *slot_N, int npairs, const int *slots, const int *rows,
                           int nrows, const void *self, const void *coll);
// the argument checks of pse_clusters_create behind its null-out and null-handle checks, in the order include/pse_amd.h lists them
// (types may be null: one type), with the handle's rcut and n_max
int clusters_create_validate(double rcut, unsigned n_max, unsigned n, const unsigned *types, int ntypes, const double *rlink);
// the argument checks of pse_clusters_label: the object (g_handle: the handle it was created on, n_max and n_slabs that handle's;
// known_status: the last word pse_clusters_status returned), N, pos, the outputs, an exclusion object of the same handle, the slab rank
int clusters_label_validate(const void *g, const void *g_handle, unsigned n_max, int n_slabs, unsigned known_status, unsigned N, const void *pos,
                            const void *label, const void *size, const void *stats, const void *hist, unsigned nhist, const void *ex,
                            const void *ex_handle);
// the same for pse_clusters_span: those checks in that order, the all-null refusal over all eight outputs, then the alignment of
// rg2 and pstats
int clusters_span_validate(const void *g, const void *g_handle, unsigned n_max, int n_slabs, unsigned known_status, unsigned N, const void *pos,
                           const void *label, const void *size, const void *stats, const void *hist, unsigned nhist, const void *span,
                           const void *image, const void *rg2, const void *pstats, const void *ex, const void *ex_handle);
// the argument checks of pse_bond_order_create behind its null-out and null-handle checks, in the order include/pse_amd.h lists them
// (types may be null: one type), with the handle's rcut and n_max
int bond_order_create_validate(double rcut, unsigned n_max, unsigned n, const unsigned *types, int ntypes, const double *rnb, int nl,
                               const int *degrees);
// the argument checks of pse_bond_order_compute: the object (b_handle: the handle it was created on, n_max and n_slabs that handle's,
// nl its number of degrees), N, pos, the outputs, the solid degree and its threshold, an exclusion object of the same handle, the slab rank
int bond_order_compute_validate(const void *b, const void *b_handle, int nl, unsigned n_max, int n_slabs, unsigned N, const void *pos,
                                const void *nnb, const void *q, const void *qbar, int solid_degree, double threshold, const void *nconn,
                                const void *stats, const void *ex, const void *ex_handle);
// the argument checks of pse_bond_order_histogram: the object (nl and ntypes its own, n_max its handle's), N, values, the column, the bins, counts
int bond_order_histogram_validate(const void *b, int nl, int ntypes, unsigned n_max, const void *values, int column, unsigned N, int nbins,
                                  double lo, double hi, const void *counts);
// The layout of pse_host_molecule_rows (include/pse_amd.h documents every array) as host vectors: mol_of (n), members, parent and depth
// (one per member, molecule after molecule in breadth-first order; parent: the position in its molecule), mol_off (nmol + 1), ends
// (2 nmol positions, 0xffffffff: none), nring (nmol), tile_mol (ntiles + 1), tile_rounds (ntiles).
struct MoleculeLayout {
    std::vector<int> mol_of;
    std::vector<unsigned> members, parent, depth, mol_off, ends, nring, tile_mol, tile_rounds;
    unsigned nmol = 0, ntiles = 0;
};
// 0 and the layout, or PSE_ERR_INVALID with a message under the name `who`: the refusals of pse_host_molecule_rows behind its null arrays
int molecule_layout(const char *who, unsigned n, unsigned nbonds, const unsigned *pairs, MoleculeLayout &L);
// what pse_molecules_create and pse_molecule_pairs_create (`who`) refuse alike behind their null-out and null-handle checks, up to and
// including the molecule types, with the handle's n_max; the layout is built on the way and returned
int molecule_topology_validate(const char *who, unsigned n_max, unsigned n, unsigned nbonds, const unsigned *pairs, const unsigned *mol_types,
                               int ntypes, MoleculeLayout &L);
// the argument checks of pse_molecules_create behind its null-out and null-handle checks, in the order include/pse_amd.h lists them,
// with the handle's n_max; the layout is built on the way (its refusals stand between those of nbonds and of ntypes) and returned
int molecules_create_validate(unsigned n_max, unsigned n, unsigned nbonds, const unsigned *pairs, const unsigned *mol_types, int ntypes, int nbins,
                              double rg_max, double ree_max, MoleculeLayout &L);
// the argument checks of pse_molecules_compute (nbins: the object's) and of pse_molecules_count
int molecules_compute_validate(const void *m, int nbins, const void *pos, const void *rows, const void *unfolded, const void *sums,
                               const void *sample, const void *hist);
int molecules_count_validate(const void *m, const void *nmol, const void *nlinear, const void *nmol_type);
// what pse_molecules_count writes (each output may be null): the molecules, and per type the linear ones and all of them
void molecules_counts(const MoleculeLayout &L, const unsigned *mol_types, int ntypes, unsigned *nmol, unsigned *nlinear, unsigned *nmol_type);
// pse_host_chain_order on a layout: rank (one per member slot)
void chain_order(const MoleculeLayout &L, std::vector<unsigned> &rank);
// the argument checks of pse_molecule_pairs_create behind its null-out and null-handle checks: molecule_topology_validate, then ns
int molecule_pairs_create_validate(unsigned n_max, unsigned n, unsigned nbonds, const unsigned *pairs, const unsigned *mol_types, int ntypes, int ns,
                                   MoleculeLayout &L);
// the argument checks of pse_molecule_pairs_compute and of pse_molecule_pairs_counts
int molecule_pairs_compute_validate(const void *p, const void *pos, const void *inv_rh, const void *curves, const void *sums, const void *sample);
int molecule_pairs_counts_validate(const void *p, const void *nmol, const void *nmol_type, const void *terms);
// terms (ntypes x ns x MOLPAIR_COLS): the summands behind every entry of the curves, max(m - s, 0) for D and max(m - 1 - s, 0) for C over
// the linear molecules of a type
void molecule_pairs_terms(const MoleculeLayout &L, const unsigned *mol_types, int ntypes, int ns, unsigned long long *terms);
// the linear molecules of a layout in ascending molecule number: their molecule numbers and sizes, and per type how many there are
void chain_modes_linear(const MoleculeLayout &L, const unsigned *mol_types, int ntypes, std::vector<unsigned> &lin_mol,
                        std::vector<unsigned> &lin_size, std::vector<unsigned> &nlin_type);
// the argument checks of pse_chain_modes_create behind its null-out and null-handle checks, in the order include/pse_amd.h lists them:
// molecule_topology_validate, nmodes, norigins, a linear molecule, the size list against the layout, the weights
int chain_modes_create_validate(unsigned n_max, unsigned n, unsigned nbonds, const unsigned *pairs, const unsigned *mol_types, int ntypes,
                                int nmodes, int nsizes, const unsigned *sizes, const double *weights, int norigins, MoleculeLayout &L);
// the argument checks of pse_chain_modes_counts, pse_chain_modes_compute, pse_chain_modes_store and pse_chain_modes_correlate
// (norigins: the object's; computed: a compute has run since create; stored: bit s = slot s holds a buffer)
int chain_modes_counts_validate(const void *obj, const void *nmol, const void *nlin, const void *nlin_type, const void *lin_mol,
                                const void *lin_size);
int chain_modes_compute_validate(const void *obj, const void *pos, const void *modes, const void *sums, const void *sample);
int chain_modes_store_validate(const void *obj, int norigins, bool computed, int slot);
int chain_modes_correlate_validate(const void *obj, int norigins, bool computed, unsigned long long stored, int npairs, const int *slots,
                                   const int *rows, int nrows, const void *corr);

}  // namespace pse
