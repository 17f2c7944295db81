// Device entry points of include/pse_amd.h for the CPU SANITIZER build only (python -m pse_amd.build --asan; never part of
// libpse_amd.so): GPU AddressSanitizer is not available on the MI355X pool, so the host-side code -- the parameter rule and the
// real-space table builder (pse_params.cpp), the tridiagonal solver, and the C++ host classes (csrc/host/) -- is
// exercised under -fsanitize=address,undefined against this stand-in.  The calls the host classes make (pse_create,
// pse_destroy, pse_set_box, pse_get_info, pse_step, pse_set_lanczos_operator) and the force entry points that the CPU tests call through
// ctypes (pse_pair_repulsion, pse_pair_repulsion_virial, pse_pair_table, their _excl forms, pse_bonds_*, pse_angles_*,
// pse_dihedrals_*, pse_exclusions_*, pse_typed_table_*, pse_pair_table_typed, pse_pair_hist_*, pse_structure_factor_*, pse_msd_*, pse_clusters_*, pse_bond_order_*, pse_molecules_*, pse_molecule_pairs_*, pse_chain_modes_*, pse_isf_*) keep a small host object that runs the REAL parameter
// rule and table builder; every entry point that would need a device returns PSE_ERR_HIP.  No test takes a number from here.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "pse_err.h"

using namespace pse;

struct Topology;
struct pse_handle {
    pse_params par;
    Derived d;
    pse_info info;
    std::vector<double> coef;
    int n_intervals = 0;
    unsigned long long steps = 0;
    int lz_op = PSE_LANCZOS_RECORDS16;
    std::vector<Topology *> topologies;
};
struct Topology {   // the REAL rows (pse_host_bond_rows, pse_host_angle_rows, pse_host_dihedral_rows, pse_host_exclusion_rows), kept on the host
    pse_handle *h;
    std::vector<int> row_off;
    std::vector<unsigned> entries;
    Topology(pse_handle *h, size_t noff, size_t nent) : h(h), row_off(noff), entries(nent) {}
    virtual ~Topology() {}
};
struct pse_bonds : Topology { using Topology::Topology; };
struct pse_angles : Topology { using Topology::Topology; };
struct pse_dihedrals : Topology { using Topology::Topology; };
struct pse_exclusions : Topology { using Topology::Topology; };
struct pse_typed_table : Topology { using Topology::Topology; };   // row_off: the REAL layout (pse_host_typed_table_layout), entries: the types
struct pse_pair_hist : Topology { using Topology::Topology; };     // entries: the types (zeros where none were given)
struct pse_structure_factor : Topology { using Topology::Topology; };   // row_off: the REAL plan (structure_factor_plan), entries: its permutation
struct pse_msd : Topology { using Topology::Topology; int norigins = 0; unsigned long long stored = 0ull; };   // the slots' bookkeeping alone
struct pse_clusters : Topology { using Topology::Topology; };      // entries: the types (zeros where none were given); the status word is always 0
struct pse_bond_order : Topology { using Topology::Topology; int ntypes = 1; };   // entries: the types; row_off: the degrees
struct pse_molecules : Topology {   // the REAL layout (molecule_layout) and the molecule types
    using Topology::Topology;
    MoleculeLayout L;
    std::vector<unsigned> types;
    int ntypes = 1, nbins = 0;
};
struct pse_molecule_pairs : Topology {   // the REAL layout and the molecule types
    using Topology::Topology;
    MoleculeLayout L;
    std::vector<unsigned> types;
    int ntypes = 1, ns = 1;
};
struct pse_chain_modes : Topology {   // the REAL layout and the molecule types; the slots' bookkeeping
    using Topology::Topology;
    MoleculeLayout L;
    std::vector<unsigned> types;
    int ntypes = 1, norigins = 0;
    bool computed = false;
    unsigned long long stored = 0ull;
};
struct pse_isf : Topology {   // row_off: the REAL plan (structure_factor_plan), entries: its permutation; the buffers' bookkeeping
    using Topology::Topology;
    int norigins = 0;
    unsigned sample_N = 0u, slot_N[ISF_MAX_ORIGINS] = {};
};
struct pse_team { int unused; };

// keeps t on its handle unless the row builder refused the list (rows_rc != 0)
template <class T>
static int topology_adopt(T *t, int rows_rc, T **out) {
    if (rows_rc) { delete t; return rows_rc; }
    t->h->topologies.push_back(t);
    *out = t;
    return 0;
}
static int topology_destroy(Topology *t) {
    if (!t) return 0;
    std::vector<Topology *> &l = t->h->topologies;
    l.erase(std::remove(l.begin(), l.end(), t), l.end());
    delete t;
    return 0;
}
static int no_device(const char *what) { return fail(PSE_ERR_HIP, "%s: sanitizer build, there is no device behind this library", what); }

extern "C" {

int pse_create(const pse_params *p, pse_handle **out) {
    if (!p || !out) return fail(PSE_ERR_INVALID, "null argument");
    *out = nullptr;
    if (p->n_max == 0) return fail(PSE_ERR_INVALID, "n_max must be positive");
    if (!(std::fabs(p->xy) <= 0.5 * (1.0 + 1e-9))) return fail(PSE_ERR_INVALID, "tilt xy = %g outside [-0.5, 0.5]", p->xy);
    pse_handle *h = new pse_handle();
    h->par = *p;
    std::string e = select_params(Box{p->Lx, p->Ly, p->Lz, p->xy}, p->xi, p->error, p->max_strain, p->Nx, p->Ny, p->Nz, p->P, p->rcut, h->d);
    if (!e.empty()) { delete h; return fail(PSE_ERR_INVALID, "%s", e.c_str()); }
    if (int rc = gaussian_fits(h->d, h->d.hx, h->d.hy, h->d.hz)) { delete h; return rc; }
    build_realspace_table(h->d.xi, h->d.rcut, h->coef, h->n_intervals);
    fill_info(h->d, &h->info);
    *out = h;
    return 0;
}
int pse_destroy(pse_handle *h) {
    if (h) for (Topology *t : h->topologies) delete t;
    delete h;
    return 0;
}
int pse_set_box(pse_handle *h, double Lx, double Ly, double Lz, double xy) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    if (!(Lx > 0 && Ly > 0 && Lz > 0)) return fail(PSE_ERR_INVALID, "box lengths must be positive");
    if (!(std::fabs(xy) <= 0.5 * (1.0 + 1e-9))) return fail(PSE_ERR_INVALID, "tilt xy = %g outside [-0.5, 0.5]", xy);
    if (int rc = gaussian_fits(h->d, Lx / h->d.Nx, Ly / h->d.Ny, Lz / h->d.Nz)) return rc;
    h->par.Lx = Lx; h->par.Ly = Ly; h->par.Lz = Lz; h->par.xy = xy;
    h->info.hx = Lx / h->d.Nx; h->info.hy = Ly / h->d.Ny; h->info.hz = Lz / h->d.Nz;
    return 0;
}
int pse_get_info(pse_handle *h, pse_info *info) {
    if (!h || !info) return fail(PSE_ERR_INVALID, "null argument");
    *info = h->info;
    return 0;
}
int pse_step(pse_handle *h, pse_double4 *, pse_double4 *, pse_double3 *, pse_int3 *, const pse_double4 *, const unsigned int *,
             unsigned int N, double kT, double dt, unsigned int, double, int *lanczos_m) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    if (N == 0 || N > h->par.n_max) return fail(PSE_ERR_INVALID, "N = %u outside (0, n_max = %u]", N, h->par.n_max);
    if (kT < 0 || !(dt > 0)) return fail(PSE_ERR_INVALID, "need kT >= 0 and dt > 0");
    ++h->steps;
    if (lanczos_m && *lanczos_m < 2) *lanczos_m = 2;
    return 0;   // nothing is integrated: the arrays are device pointers and there is no device
}
// (pos, force, table and out8 are device pointers and there is no device: nothing is read or written)
int pse_pair_repulsion(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *, unsigned N, double, double sigma, int) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    return pair_repulsion_validate(h->d.rcut, h->par.n_max, h->par.n_slabs, N, pos, force, false, nullptr, sigma);
}
int pse_pair_repulsion_virial(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *, unsigned N, double, double sigma, int,
                              double *out8) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    return pair_repulsion_validate(h->d.rcut, h->par.n_max, h->par.n_slabs, N, pos, force, true, out8, sigma);
}
int pse_pair_table(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *, unsigned N, const double *table, int width,
                   double rmin, double rmax, int, double *out8) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    return pair_table_validate(h->d.rcut, h->par.n_max, h->par.n_slabs, N, pos, force, table, width, rmin, rmax, out8);
}
int pse_exclusions_create(pse_handle *h, unsigned n, unsigned npairs, const unsigned *pairs_host, pse_exclusions **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_exclusions_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_exclusions_create: null handle");
    if (int rc = exclusions_validate(h->par.n_max, n, npairs, pairs_host)) return rc;
    pse_exclusions *ex = new pse_exclusions(h, (size_t)n + 1, (size_t)npairs * 2);
    return topology_adopt(ex, pse_host_exclusion_rows(n, npairs, pairs_host, ex->row_off.data(), ex->entries.data()), out);
}
int pse_exclusions_destroy(pse_exclusions *ex) { return topology_destroy(ex); }
int pse_pair_repulsion_excl(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *, unsigned N, double, double sigma, int,
                            double *out8, const pse_exclusions *ex) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    if (int rc = pair_repulsion_validate(h->d.rcut, h->par.n_max, h->par.n_slabs, N, pos, force, out8 != nullptr, out8, sigma)) return rc;
    return pair_excl_validate("pse_pair_repulsion_excl", ex, ex ? ex->h : nullptr, h);
}
int pse_pair_table_excl(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *, unsigned N, const double *table, int width,
                        double rmin, double rmax, int, double *out8, const pse_exclusions *ex) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    if (int rc = pair_table_validate(h->d.rcut, h->par.n_max, h->par.n_slabs, N, pos, force, table, width, rmin, rmax, out8)) return rc;
    return pair_excl_validate("pse_pair_table_excl", ex, ex ? ex->h : nullptr, h);
}
int pse_typed_table_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, const int *width_host, const double *rmin_host,
                           const double *rmax_host, const double *tables_host, pse_typed_table **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_typed_table_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_typed_table_create: null handle");
    if (int rc = typed_table_validate(h->d.rcut, h->par.n_max, n, types_host, ntypes, width_host, rmin_host, rmax_host, tables_host)) return rc;
    const int npt = ntypes * (ntypes + 1) / 2;
    pse_typed_table *t = new pse_typed_table(h, (size_t)npt, (size_t)n);
    std::vector<double> scale(npt), rmax2(npt);
    int total = 0;
    std::copy(types_host, types_host + n, t->entries.begin());
    return topology_adopt(t, pse_host_typed_table_layout(ntypes, width_host, rmin_host, rmax_host, t->row_off.data(), scale.data(), rmax2.data(), &total),
                          out);
}
int pse_typed_table_destroy(pse_typed_table *t) { return topology_destroy(t); }
int pse_pair_table_typed(pse_typed_table *t, const pse_double4 *pos, pse_double4 *force, const unsigned *, unsigned N, int, double *out8,
                         const pse_exclusions *ex) {
    pse_handle *h = t ? t->h : nullptr;
    return pair_typed_validate(t, h, h ? h->par.n_max : 0u, h ? h->par.n_slabs : 1, N, pos, force, out8, ex, ex ? ex->h : nullptr);
}
int pse_pair_hist_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, int nbins, double rmin, double rmax, pse_pair_hist **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_pair_hist_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_pair_hist_create: null handle");
    if (int rc = pair_hist_create_validate(h->d.rcut, h->par.n_max, h->par.n_slabs, n, types_host, ntypes, nbins, rmin, rmax)) return rc;
    pse_pair_hist *g = new pse_pair_hist(h, 0, (size_t)n);
    if (types_host) std::copy(types_host, types_host + n, g->entries.begin());
    return topology_adopt(g, 0, out);
}
int pse_pair_hist_destroy(pse_pair_hist *g) { return topology_destroy(g); }
int pse_pair_hist_accumulate(pse_pair_hist *g, const pse_double4 *pos, const unsigned *, unsigned N, unsigned long long *counts,
                             const pse_exclusions *ex) {
    pse_handle *h = g ? g->h : nullptr;   // (pos and counts are device pointers and there is no device: nothing is read or written)
    return pair_hist_validate(g, h, h ? h->par.n_max : 0u, N, pos, counts, ex, ex ? ex->h : nullptr);
}
int pse_structure_factor_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, unsigned nk, const int *modes_host,
                                pse_structure_factor **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_structure_factor_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_structure_factor_create: null handle");
    if (int rc = structure_factor_create_validate(h->par.n_max, n, types_host, ntypes, nk, modes_host)) return rc;
    pse_structure_factor *f = new pse_structure_factor(h, 0, 0);
    std::vector<unsigned> uoff;
    structure_factor_plan(nk, modes_host, f->entries, uoff, f->row_off);
    return topology_adopt(f, 0, out);
}
int pse_structure_factor_destroy(pse_structure_factor *f) { return topology_destroy(f); }
int pse_structure_factor_accumulate(pse_structure_factor *f, const pse_double4 *pos, const unsigned *, unsigned N, double *rho, double *sums) {
    pse_handle *h = f ? f->h : nullptr;   // (pos, rho and sums are device pointers and there is no device: nothing is read or written)
    return structure_factor_validate(f, h ? h->par.n_max : 0u, N, pos, rho, sums);
}
int pse_msd_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, int norigins, pse_msd **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_msd_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_msd_create: null handle");
    if (int rc = msd_create_validate(h->par.n_max, n, types_host, ntypes, norigins)) return rc;
    pse_msd *m = new pse_msd(h, 0, 0);
    m->norigins = norigins;
    return topology_adopt(m, 0, out);
}
int pse_msd_destroy(pse_msd *m) { return topology_destroy(m); }
// (pos, image, sums and out are device pointers and there is no device: nothing is read or written; a store marks its slot)
int pse_msd_store(pse_msd *m, int slot, const pse_double4 *pos, const pse_int3 *image, const unsigned *, unsigned N, double strain) {
    if (int rc = msd_slot_validate("pse_msd_store", m, m ? m->norigins : 0, m ? m->h->par.n_max : 0u, slot, N, pos, image, strain)) return rc;
    m->stored |= 1ull << slot;
    return 0;
}
int pse_msd_displacement(pse_msd *m, int slot, const pse_double4 *pos, const pse_int3 *image, const unsigned *, unsigned N, double strain,
                         pse_double4 *out) {
    if (int rc = msd_slot_validate("pse_msd_displacement", m, m ? m->norigins : 0, m ? m->h->par.n_max : 0u, slot, N, pos, image, strain)) return rc;
    return msd_displacement_validate(m->stored, slot, out);
}
int pse_msd_accumulate(pse_msd *m, const pse_double4 *pos, const pse_int3 *image, const unsigned *, unsigned N, double strain, int npairs,
                       const int *slots_host, const int *rows_host, int nrows, double *sums) {
    return msd_accumulate_validate(m, m ? m->norigins : 0, m ? m->stored : 0ull, m ? m->h->par.n_max : 0u, N, pos, image, strain, npairs,
                                   slots_host, rows_host, nrows, sums);
}
int pse_clusters_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, const double *rlink_host, pse_clusters **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_clusters_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_clusters_create: null handle");
    if (int rc = clusters_create_validate(h->d.rcut, h->par.n_max, n, types_host, ntypes, rlink_host)) return rc;
    pse_clusters *g = new pse_clusters(h, 0, (size_t)n);
    if (types_host) std::copy(types_host, types_host + n, g->entries.begin());
    return topology_adopt(g, 0, out);
}
int pse_clusters_destroy(pse_clusters *g) { return topology_destroy(g); }
int pse_clusters_label(pse_clusters *g, const pse_double4 *pos, const unsigned *, unsigned N, unsigned *label, unsigned *size,
                       unsigned long long *stats, unsigned long long *hist, unsigned nhist, const pse_exclusions *ex) {
    pse_handle *h = g ? g->h : nullptr;   // (the arrays are device pointers and there is no device: nothing is read or written)
    return clusters_label_validate(g, h, h ? h->par.n_max : 0u, h ? h->par.n_slabs : 1, 0u, N, pos, label, size, stats, hist, nhist, ex,
                                   ex ? ex->h : nullptr);
}
int pse_clusters_span(pse_clusters *g, const pse_double4 *pos, const unsigned *, unsigned N, unsigned *label, unsigned *size,
                      unsigned long long *stats, unsigned long long *hist, unsigned nhist, unsigned *span, int *image, double *rg2,
                      unsigned long long *pstats, const pse_exclusions *ex) {
    pse_handle *h = g ? g->h : nullptr;   // (as pse_clusters_label: nothing is read or written)
    return clusters_span_validate(g, h, h ? h->par.n_max : 0u, h ? h->par.n_slabs : 1, 0u, N, pos, label, size, stats, hist, nhist, span, image,
                                  rg2, pstats, ex, ex ? ex->h : nullptr);
}
int pse_clusters_status(pse_clusters *g, unsigned *status) {
    if (!g) return fail(PSE_ERR_INVALID, "pse_clusters_status: null cluster object");
    if (!status) return fail(PSE_ERR_INVALID, "pse_clusters_status: null status");
    *status = 0u;   // (nothing ever ran)
    return 0;
}
int pse_bond_order_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, const double *rnb_host, int nl, const int *degrees_host,
                          pse_bond_order **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_bond_order_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_bond_order_create: null handle");
    if (int rc = bond_order_create_validate(h->d.rcut, h->par.n_max, n, types_host, ntypes, rnb_host, nl, degrees_host)) return rc;
    pse_bond_order *b = new pse_bond_order(h, (size_t)nl, (size_t)n);
    b->ntypes = ntypes;
    std::copy(degrees_host, degrees_host + nl, b->row_off.begin());
    if (types_host) std::copy(types_host, types_host + n, b->entries.begin());
    return topology_adopt(b, 0, out);
}
int pse_bond_order_destroy(pse_bond_order *b) { return topology_destroy(b); }
// (the arrays are device pointers and there is no device: nothing is read or written)
int pse_bond_order_compute(pse_bond_order *b, const pse_double4 *pos, const unsigned *, unsigned N, unsigned *nnb, double *q, double *qbar,
                           int solid_degree, double threshold, unsigned, unsigned *nconn, unsigned long long *stats, const pse_exclusions *ex) {
    pse_handle *h = b ? b->h : nullptr;
    return bond_order_compute_validate(b, h, b ? (int)b->row_off.size() : 0, h ? h->par.n_max : 0u, h ? h->par.n_slabs : 1, N, pos, nnb, q, qbar,
                                       solid_degree, threshold, nconn, stats, ex, ex ? ex->h : nullptr);
}
int pse_bond_order_histogram(pse_bond_order *b, const double *values, int column, const unsigned *, unsigned N, int nbins, double lo, double hi,
                             unsigned long long *counts) {
    return bond_order_histogram_validate(b, b ? (int)b->row_off.size() : 0, b ? b->ntypes : 1, b ? b->h->par.n_max : 0u, values, column, N, nbins,
                                         lo, hi, counts);
}
int pse_molecules_create(pse_handle *h, unsigned n, unsigned nbonds, const unsigned *pairs_host, const unsigned *mol_types_host, int ntypes, int nbins,
                         double rg_max, double ree_max, pse_molecules **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_molecules_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_molecules_create: null handle");
    pse_molecules *m = new pse_molecules(h, 0, 0);
    m->ntypes = ntypes; m->nbins = nbins;
    const int rc = molecules_create_validate(h->par.n_max, n, nbonds, pairs_host, mol_types_host, ntypes, nbins, rg_max, ree_max, m->L);
    if (!rc && mol_types_host) m->types.assign(mol_types_host, mol_types_host + m->L.nmol);
    return topology_adopt(m, rc, out);
}
int pse_molecules_destroy(pse_molecules *m) { return topology_destroy(m); }
int pse_molecules_count(pse_molecules *m, unsigned *nmol, unsigned *nlinear, unsigned *nmol_type) {
    if (int rc = molecules_count_validate(m, nmol, nlinear, nmol_type)) return rc;
    molecules_counts(m->L, m->types.empty() ? nullptr : m->types.data(), m->ntypes, nmol, nlinear, nmol_type);
    return 0;
}
// (the arrays are device pointers and there is no device: nothing is read or written)
int pse_molecules_compute(pse_molecules *m, const pse_double4 *pos, double *rows, pse_double4 *unfolded, double *sums, double *sample,
                          unsigned long long *hist) {
    return molecules_compute_validate(m, m ? m->nbins : 0, pos, rows, unfolded, sums, sample, hist);
}
int pse_molecule_pairs_create(pse_handle *h, unsigned n, unsigned nbonds, const unsigned *pairs_host, const unsigned *mol_types_host, int ntypes,
                              int ns, pse_molecule_pairs **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_molecule_pairs_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_molecule_pairs_create: null handle");
    pse_molecule_pairs *p = new pse_molecule_pairs(h, 0, 0);
    p->ntypes = ntypes; p->ns = ns;
    const int rc = molecule_pairs_create_validate(h->par.n_max, n, nbonds, pairs_host, mol_types_host, ntypes, ns, p->L);
    if (!rc && mol_types_host) p->types.assign(mol_types_host, mol_types_host + p->L.nmol);
    return topology_adopt(p, rc, out);
}
int pse_molecule_pairs_destroy(pse_molecule_pairs *p) { return topology_destroy(p); }
int pse_molecule_pairs_counts(pse_molecule_pairs *p, unsigned *nmol, unsigned *nmol_type, unsigned long long *terms) {
    if (int rc = molecule_pairs_counts_validate(p, nmol, nmol_type, terms)) return rc;
    const unsigned *types = p->types.empty() ? nullptr : p->types.data();
    molecules_counts(p->L, types, p->ntypes, nmol, nullptr, nmol_type);
    if (terms) molecule_pairs_terms(p->L, types, p->ntypes, p->ns, terms);
    return 0;
}
// (the arrays are device pointers and there is no device: nothing is read or written)
int pse_molecule_pairs_compute(pse_molecule_pairs *p, const pse_double4 *pos, double *inv_rh, double *curves, double *sums, double *sample) {
    return molecule_pairs_compute_validate(p, pos, inv_rh, curves, sums, sample);
}
int pse_chain_modes_create(pse_handle *h, unsigned n, unsigned nbonds, const unsigned *pairs_host, const unsigned *mol_types_host, int ntypes,
                           int nmodes, int nsizes, const unsigned *sizes_host, const double *weights_host, int norigins, pse_chain_modes **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_chain_modes_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_chain_modes_create: null handle");
    pse_chain_modes *m = new pse_chain_modes(h, 0, 0);
    m->ntypes = ntypes; m->norigins = norigins;
    const int rc = chain_modes_create_validate(h->par.n_max, n, nbonds, pairs_host, mol_types_host, ntypes, nmodes, nsizes, sizes_host, weights_host,
                                               norigins, m->L);
    if (!rc && mol_types_host) m->types.assign(mol_types_host, mol_types_host + m->L.nmol);
    return topology_adopt(m, rc, out);
}
int pse_chain_modes_destroy(pse_chain_modes *obj) { return topology_destroy(obj); }
int pse_chain_modes_counts(pse_chain_modes *obj, unsigned *nmol, unsigned *nlin, unsigned *nlin_type, unsigned *lin_mol, unsigned *lin_size) {
    if (int rc = chain_modes_counts_validate(obj, nmol, nlin, nlin_type, lin_mol, lin_size)) return rc;
    std::vector<unsigned> mol, size, per_type;
    chain_modes_linear(obj->L, obj->types.empty() ? nullptr : obj->types.data(), obj->ntypes, mol, size, per_type);
    if (nmol) *nmol = obj->L.nmol;
    if (nlin) *nlin = (unsigned)mol.size();
    if (nlin_type) std::copy(per_type.begin(), per_type.end(), nlin_type);
    if (lin_mol) std::copy(mol.begin(), mol.end(), lin_mol);
    if (lin_size) std::copy(size.begin(), size.end(), lin_size);
    return 0;
}
// (the arrays are device pointers and there is no device: nothing is read or written; a compute and a store mark the bookkeeping)
int pse_chain_modes_compute(pse_chain_modes *obj, const pse_double4 *pos, double *modes, double *sums, double *sample) {
    if (int rc = chain_modes_compute_validate(obj, pos, modes, sums, sample)) return rc;
    obj->computed = true;
    return 0;
}
int pse_chain_modes_store(pse_chain_modes *obj, int slot) {
    if (int rc = chain_modes_store_validate(obj, obj ? obj->norigins : 0, obj ? obj->computed : false, slot)) return rc;
    obj->stored |= 1ull << slot;
    return 0;
}
int pse_chain_modes_correlate(pse_chain_modes *obj, int npairs, const int *slots_host, const int *rows_host, int nrows, double *corr) {
    return chain_modes_correlate_validate(obj, obj ? obj->norigins : 0, obj ? obj->computed : false, obj ? obj->stored : 0ull, npairs, slots_host,
                                          rows_host, nrows, corr);
}
int pse_isf_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, unsigned nk, const int *modes_host, int norigins,
                   pse_isf **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_isf_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_isf_create: null handle");
    if (int rc = isf_create_validate(h->par.n_max, n, types_host, ntypes, nk, modes_host, norigins)) return rc;
    pse_isf *f = new pse_isf(h, 0, 0);
    f->norigins = norigins;
    std::vector<unsigned> uoff;
    structure_factor_plan(nk, modes_host, f->entries, uoff, f->row_off);
    return topology_adopt(f, 0, out);
}
int pse_isf_destroy(pse_isf *f) { return topology_destroy(f); }
// (the arrays are device pointers and there is no device: nothing is read or written; a sample and a store mark the bookkeeping)
int pse_isf_sample(pse_isf *f, const pse_double4 *pos, const unsigned *, unsigned N, double *rho, double *static_sums) {
    if (int rc = isf_sample_validate(f, f ? f->h->par.n_max : 0u, N, pos, rho, static_sums)) return rc;
    f->sample_N = N;
    return 0;
}
int pse_isf_store(pse_isf *f, int slot) {
    if (int rc = isf_store_validate(f, f ? f->norigins : 0, f ? f->sample_N : 0u, slot)) return rc;
    f->slot_N[slot] = f->sample_N;
    return 0;
}
int pse_isf_correlate(pse_isf *f, int npairs, const int *slots_host, const int *rows_host, int nrows, double *self, double *coll) {
    return isf_correlate_validate(f, f ? f->norigins : 0, f ? f->sample_N : 0u, f ? f->slot_N : nullptr, npairs, slots_host, rows_host, nrows,
                                  self, coll);
}
int pse_bonds_create(pse_handle *h, unsigned n, unsigned nbonds, const unsigned *pairs_host, const unsigned *types_host, int ntypes,
                     const int *kind_host, const double *k_host, const double *r0_host, pse_bonds **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_bonds_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_bonds_create: null handle");
    if (int rc = bonds_validate(h->par.n_max, n, nbonds, pairs_host, types_host, ntypes, kind_host, k_host, r0_host)) return rc;
    pse_bonds *b = new pse_bonds(h, (size_t)n + 1, (size_t)nbonds * 4);
    return topology_adopt(b, pse_host_bond_rows(n, nbonds, pairs_host, types_host, b->row_off.data(), b->entries.data()), out);
}
int pse_bonds_destroy(pse_bonds *b) { return topology_destroy(b); }
int pse_bond_forces(pse_bonds *b, const pse_double4 *pos, pse_double4 *force, int, double *out8) {
    if (!b) return fail(PSE_ERR_INVALID, "pse_bond_forces: null bond object");
    if (!pos) return fail(PSE_ERR_INVALID, "pse_bond_forces: null pos");
    if (!force && !out8) return fail(PSE_ERR_INVALID, "pse_bond_forces: force and out8 are both null: nothing to compute");
    return 0;   // pos, force and out8 are device pointers and there is no device: nothing is read or written
}
int pse_bonds_overstretched(pse_bonds *b, unsigned long long *count) {
    if (!b || !count) return fail(PSE_ERR_INVALID, "pse_bonds_overstretched: null argument");
    *count = 0;
    return 0;
}
int pse_angles_create(pse_handle *h, unsigned n, unsigned nangles, const unsigned *triples_host, const unsigned *types_host, int ntypes,
                      const int *kind_host, const double *k_host, const double *theta0_host, pse_angles **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_angles_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_angles_create: null handle");
    if (int rc = angles_validate(h->par.n_max, n, nangles, triples_host, types_host, ntypes, kind_host, k_host, theta0_host)) return rc;
    pse_angles *a = new pse_angles(h, (size_t)n + 1, (size_t)nangles * 12);
    return topology_adopt(a, pse_host_angle_rows(n, nangles, triples_host, types_host, a->row_off.data(), a->entries.data()), out);
}
int pse_angles_destroy(pse_angles *a) { return topology_destroy(a); }
int pse_angle_forces(pse_angles *a, const pse_double4 *pos, pse_double4 *force, int, double *out8) {
    if (!a) return fail(PSE_ERR_INVALID, "pse_angle_forces: null angle object");
    if (!pos) return fail(PSE_ERR_INVALID, "pse_angle_forces: null pos");
    if (!force && !out8) return fail(PSE_ERR_INVALID, "pse_angle_forces: force and out8 are both null: nothing to compute");
    return 0;   // pos, force and out8 are device pointers and there is no device: nothing is read or written
}
int pse_dihedrals_create(pse_handle *h, unsigned n, unsigned ndihedrals, const unsigned *quads_host, const unsigned *types_host, int ntypes,
                         const int *kind_host, const double *params_host, pse_dihedrals **out) {
    if (!out) return fail(PSE_ERR_INVALID, "pse_dihedrals_create: null out");
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "pse_dihedrals_create: null handle");
    if (int rc = dihedrals_validate(h->par.n_max, n, ndihedrals, quads_host, types_host, ntypes, kind_host, params_host)) return rc;
    pse_dihedrals *d = new pse_dihedrals(h, (size_t)n + 1, (size_t)ndihedrals * 20);
    return topology_adopt(d, pse_host_dihedral_rows(n, ndihedrals, quads_host, types_host, d->row_off.data(), d->entries.data()), out);
}
int pse_dihedrals_destroy(pse_dihedrals *d) { return topology_destroy(d); }
int pse_dihedral_forces(pse_dihedrals *d, const pse_double4 *pos, pse_double4 *force, int, double *out8) {
    if (!d) return fail(PSE_ERR_INVALID, "pse_dihedral_forces: null dihedral object");
    if (!pos) return fail(PSE_ERR_INVALID, "pse_dihedral_forces: null pos");
    if (!force && !out8) return fail(PSE_ERR_INVALID, "pse_dihedral_forces: force and out8 are both null: nothing to compute");
    return 0;   // pos, force and out8 are device pointers and there is no device: nothing is read or written
}

int pse_set_stream(pse_handle *, void *) { return no_device("pse_set_stream"); }
int pse_set_timing(pse_handle *, int) { return no_device("pse_set_timing"); }
int pse_set_async(pse_handle *, int) { return no_device("pse_set_async"); }
int pse_set_timestep_offset(pse_handle *, const unsigned int *) { return no_device("pse_set_timestep_offset"); }
int pse_debug_last_gate(pse_handle *, int *) { return no_device("pse_debug_last_gate"); }
int pse_set_neighbor_skin(pse_handle *, double) { return no_device("pse_set_neighbor_skin"); }
int pse_neighbor_stats(pse_handle *, double *, unsigned long long *, unsigned long long *) { return no_device("pse_neighbor_stats"); }
int pse_mobility(pse_handle *, const pse_double4 *, const pse_double4 *, pse_double4 *, const unsigned int *, unsigned int, int) { return no_device("pse_mobility"); }
int pse_brownian_velocity(pse_handle *, const pse_double4 *, const pse_double4 *, pse_double4 *, const unsigned int *, unsigned int, double,
                          double, unsigned int, int *) { return no_device("pse_brownian_velocity"); }
int pse_sqrt_mreal(pse_handle *, const pse_double4 *, const pse_double4 *, pse_double4 *, const unsigned int *, unsigned int, double, int *) { return no_device("pse_sqrt_mreal"); }
int pse_random_psi(pse_handle *, pse_double4 *, const unsigned int *, unsigned int, unsigned int) { return no_device("pse_random_psi"); }
int pse_eval_realspace(pse_handle *, const double *, int, double *, double *) { return no_device("pse_eval_realspace"); }
int pse_debug_copy_grid(pse_handle *, int, double *) { return no_device("pse_debug_copy_grid"); }
int pse_debug_spread(pse_handle *, const pse_double4 *, const pse_double4 *, const unsigned int *, unsigned int) { return no_device("pse_debug_spread"); }
int pse_debug_gather(pse_handle *, const pse_double4 *, const double *, const unsigned int *, unsigned int, pse_double4 *) { return no_device("pse_debug_gather"); }
int pse_debug_far_path(pse_handle *, unsigned int, int *) { return no_device("pse_debug_far_path"); }
int pse_debug_wave_grid(pse_handle *, const double *, double, double, int, double, double, unsigned int, int, double *) { return no_device("pse_debug_wave_grid"); }
int pse_debug_fft_path(pse_handle *, int *) { return no_device("pse_debug_fft_path"); }
int pse_debug_kvector(pse_handle *, int, const int *, double *) { return no_device("pse_debug_kvector"); }
int pse_debug_grid_placement(pse_handle *, int *, float *, float *) { return no_device("pse_debug_grid_placement"); }
int pse_debug_vq_roundtrip(int, const double *, double *) { return no_device("pse_debug_vq_roundtrip"); }
int pse_debug_lz_decide(const double *, int, const pse_debug_lz_decision *, double, pse_debug_lz_outcome *) { return no_device("pse_debug_lz_decide"); }
int pse_debug_lz_decide_supported(int) { return 0; }   // (a yes / no answer, not a status: without a device no size is)
int pse_debug_matvec_ms(pse_handle *, int, float *) { return no_device("pse_debug_matvec_ms"); }
int pse_set_lanczos_extra(pse_handle *, int) { return no_device("pse_set_lanczos_extra"); }
// the operator choice is host state (the fp64 plane would be allocated on the device: the stub only records the choice)
int pse_set_lanczos_operator(pse_handle *h, int op) {
    if (!h) return fail(PSE_ERR_INVALID, "pse_set_lanczos_operator: null handle");
    if (op != PSE_LANCZOS_RECORDS16 && op != PSE_LANCZOS_FP64) return fail(PSE_ERR_INVALID, "pse_set_lanczos_operator: %d is not an operator", op);
    h->lz_op = op;
    return 0;
}
int pse_get_lanczos_operator(pse_handle *h, int *op) {
    if (!h || !op) return fail(PSE_ERR_INVALID, "pse_get_lanczos_operator: null argument");
    *op = h->lz_op;
    return 0;
}
int pse_brownian_velocity_part(pse_handle *, const pse_double4 *, const pse_double4 *, pse_double4 *, const unsigned int *, unsigned int, double,
                               double, unsigned int, int, int *) { return no_device("pse_brownian_velocity_part"); }
int pse_integrate(pse_handle *, pse_double4 *, const pse_double4 *, pse_double3 *, pse_int3 *, const pse_double4 *, const unsigned int *, unsigned int,
                  double, double) { return no_device("pse_integrate"); }
int pse_team_redistribute_local(pse_team *, pse_double4 *const *, pse_double4 *const *, pse_double3 *const *, pse_int3 *const *, pse_double4 *const *,
                                unsigned int *const *, unsigned int *const *) { return no_device("pse_team_redistribute_local"); }
int pse_team_set_lanczos_extra(pse_team *, int) { return no_device("pse_team_set_lanczos_extra"); }
int pse_team_unique_id(void *) { return no_device("pse_team_unique_id"); }
int pse_team_create(pse_handle **, int, const void *, pse_team **) { return no_device("pse_team_create"); }
int pse_team_create_transport(pse_handle *, const pse_transport *, pse_team **) { return no_device("pse_team_create_transport"); }
int pse_team_destroy(pse_team *) { return 0; }
int pse_team_debug_solo(pse_team *, int) { return no_device("pse_team_debug_solo"); }
int pse_team_step_local(pse_team *, pse_double4 *const *, pse_double4 *const *, pse_double3 *const *, pse_int3 *const *, const pse_double4 *const *,
                        unsigned int *const *, unsigned int *const *, double, double, unsigned int, double, int, int *) { return no_device("pse_team_step_local"); }
int pse_local_layout(pse_handle *, int *, int *, int *, int *, int *) { return no_device("pse_local_layout"); }
int pse_team_local_status(pse_team *, int *) { return no_device("pse_team_local_status"); }
int pse_team_set_diag(pse_team *, int) { return no_device("pse_team_set_diag"); }
int pse_team_get_diag(pse_team *, pse_team_diag *) { return no_device("pse_team_get_diag"); }
int pse_team_mobility(pse_team *, const pse_double4 *const *, const pse_double4 *const *, pse_double4 *const *, const unsigned int *, unsigned int, int) { return no_device("pse_team_mobility"); }
int pse_team_brownian_velocity(pse_team *, const pse_double4 *const *, const pse_double4 *const *, pse_double4 *const *, const unsigned int *,
                               unsigned int, double, double, unsigned int, int *) { return no_device("pse_team_brownian_velocity"); }
int pse_team_step(pse_team *, pse_double4 *const *, pse_double4 *const *, pse_double3 *const *, pse_int3 *const *, const pse_double4 *const *,
                  const unsigned int *, unsigned int, double, double, unsigned int, double, int *) { return no_device("pse_team_step"); }

}  // extern "C"
