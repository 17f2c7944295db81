// The device objects of the C-ABI (include/pse_amd.h) and the passes that take them: the pair passes on the cell list (repulsion, table,
// typed table, histogram, clusters, bond order), the bonded passes (bonds, angles, dihedrals), pair exclusions, structure factors, displacement
// moments, chain conformations, chain statistics, chain normal modes and intermediate scattering functions.  Host code only: every kernel is behind a launch wrapper of pse_forces.h, pse_analysis.h, pse_percolation.h, pse_order.h, pse_molecules.h, pse_molpairs.h, pse_molmodes.h or pse_scatter.h, the objects own their arrays through DeviceObject
// (pse_handle.h), and every argument check is a validator of pse_host_api.cpp (pse_err.h), shared with the sanitizer build's stand-in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pse_handle.h"
#include "pse_forces.h"
#include "pse_analysis.h"
#include "pse_percolation.h"
#include "pse_order.h"
#include "pse_molecules.h"
#include "pse_molpairs.h"
#include "pse_molmodes.h"
#include "pse_scatter.h"

// A bonded topology on the device (include/pse_amd.h): the rows of pse_host_bond_rows, pse_host_angle_rows or pse_host_dihedral_rows, the per-type parameters
// and, for bonds, the counter of overstretched FENE bonds.
struct Topology : DeviceObject {
    unsigned n = 0, count = 0;              // particles; bonds, angles or dihedrals
    int ntypes = 0;
    int *row_off = nullptr;                 // n + 1 (bonds and exclusions read them as unsigned, angles and dihedrals as int)
    unsigned *entries = nullptr;            // bonds: 2 count x uint2 (partner, type); angles: 3 count x uint4 (i, j, k, type), j the vertex, i < k;
                                            // dihedrals: 4 count x uint4 (i, j, k, l), i < l, then 4 count x unsigned types
    void *par = nullptr;                    // ntypes x BondParam, AngleParam or DihedralParam
    unsigned long long *over = nullptr;     // bonds: FENE bonds seen at r >= r0 since creation
};
struct pse_bonds : Topology {};
struct pse_angles : Topology {};
struct pse_dihedrals : Topology {};
struct pse_exclusions : Topology {};   // entries: the partners, one unsigned each (pse_host_exclusion_rows); no parameters
// The other objects hold the struct that their launches take (pse_forces.h, pse_analysis.h and pse_order.h, which document the arrays), filled once at creation, and
// the host-only words that the entry points keep about them.
struct pse_typed_table : DeviceObject { PairTypedTables tt{}; };
struct pse_pair_hist : DeviceObject { PairHist ph{}; };
struct pse_clusters : DeviceObject {
    ClusterLinks cl{};
    ClusterSpan sp{};                       // the scratch of pse_clusters_span, placed by its first call (word == null: not yet)
    unsigned known_status = 0u;             // the last word pse_clusters_status read
};
struct pse_bond_order : DeviceObject { BondOrder bo{}; };
struct pse_structure_factor : DeviceObject { StructureFactor sf{}; };
struct pse_molecules : DeviceObject {
    Molecules mo{};
    std::vector<unsigned> nlinear, nmol_type;   // per type, for pse_molecules_count
};
struct pse_molecule_pairs : DeviceObject {
    MolPairs mp{};
    std::vector<unsigned> nmol_type;            // per type, for pse_molecule_pairs_counts
    std::vector<unsigned long long> terms;      // ntypes x ns x MOLPAIR_COLS
};
struct pse_chain_modes : DeviceObject {
    MolModes mm{};
    int norigins = 0;
    bool computed = false;                      // a pse_chain_modes_compute has been queued since create
    unsigned long long stored = 0ull;           // bit s = slot s holds a buffer
    std::vector<unsigned> lin_mol, lin_size, nlin_type;   // for pse_chain_modes_counts
};
struct pse_msd : DeviceObject {
    MsdOrigins mo{};
    int norigins = 0;
    unsigned long long stored = 0ull;       // bit s = slot s holds positions
};
struct pse_isf : DeviceObject {
    Scatter sc{};
    int norigins = 0;
    unsigned sample_N = 0u;                     // N of the sample in the current buffer (0: no pse_isf_sample since create)
    const unsigned *group = nullptr;            // ... and its group
    unsigned slot_N[ISF_MAX_ORIGINS] = {};      // N of the sample stored in a slot (0: never stored)
};

// ---- what every pse_*_create shares (`who`: its name) --------------------------------------------------------------------------------
// In front of the validator: a null `out` and a null handle, refused in that order.
template <class T>
static int create_begin(const char *who, pse_handle *h, T **out) {
    if (!out) return fail(PSE_ERR_INVALID, "%s: null out", who);
    *out = nullptr;
    if (!h) return fail(PSE_ERR_INVALID, "%s: null handle", who);
    return 0;
}
// Behind the put()s of the new object `t`, `e` what the last of them returned (the first failure, if there was one): the object goes
// again, with whatever it had placed, or it is adopted by the handle and handed out.
template <class T>
static int create_end(const char *who, pse_handle *h, T *t, hipError_t e, T **out) {
    // a hipMemset may return before the memory is zero, and it ran on the null stream, which a non-blocking h->stream (pse_set_stream)
    // does not wait for: the object's first pass must not overtake it
    if (e == hipSuccess && t->zeroed) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        const size_t bytes = t->bytes;
        delete t;
        return fail(PSE_ERR_HIP, "%s: placing %zu bytes on the device failed: %s", who, bytes, hipGetErrorString(e));
    }
    h->topologies.push_back(t);
    *out = t;
    return 0;
}
// The types of n particles as the device holds them, one byte each; types_host null: one type.
static std::vector<unsigned char> type_bytes(const unsigned *types_host, unsigned n) {
    std::vector<unsigned char> types(n, (unsigned char)0);
    if (types_host) for (unsigned i = 0; i < n; ++i) types[i] = (unsigned char)types_host[i];
    return types;
}
static int object_destroy(DeviceObject *t) {
    if (!t) return 0;
    pse_handle *h = t->h;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));   // a queued pass may still read the rows
    h->topologies.erase(std::remove(h->topologies.begin(), h->topologies.end(), t), h->topologies.end());
    delete t;
    return 0;
}

// What the six passes over the cell list share behind their validators: the device, the sort with the cell list, and the rows of an
// optional exclusion object as the launches take them (rows == null: a plain pass).
struct CellPass {
    PairExclusions er{};
    const PairExclusions *rows = nullptr;
    int begin(pse_handle *h, const pse_double4 *pos, const unsigned *group, unsigned N, const pse_exclusions *ex) {
        HIPCHK(hipSetDevice(h->device));
        TRY(prepare(h, (const double4 *)pos, nullptr, group, (int)N, false, true, PrepExtra{false, 0}, true));
        if (ex) { er = PairExclusions{(const unsigned *)ex->row_off, ex->entries, ex->n}; rows = &er; }
        return 0;
    }
};

// pse_pair_repulsion and pse_pair_repulsion_virial (include/pse_amd.h): the force pass, and the same pass with the pair observables of
// the repulsion -- energy, virial and pair count in eight device doubles.  Queue-only: nothing is read back, out8 is written by the stream.
// `excl`: the name of the entry point that takes an exclusion object `ex`, checked behind the plain pass's own arguments; null: a plain pass.
static int pair_repulsion(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *group, unsigned N, double k, double sigma,
                          int accumulate, bool virial, double *out8, const char *excl = nullptr, const pse_exclusions *ex = nullptr) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    TRY(pair_repulsion_validate(h->d.rcut, (unsigned)h->n_max, h->n_slabs, N, pos, force, virial, out8, sigma));
    if (excl) TRY(pair_excl_validate(excl, ex, ex ? ex->h : nullptr, h));
    CellPass cp;
    TRY(cp.begin(h, pos, group, N, ex));
    launch_pair_repulsion(h->pos_s, h->tag_s, (int)N, h->cell_off, h->dbox, h->nc, k, sigma, accumulate, (double4 *)force, h->pv_rows, out8,
                          h->stream, cp.rows);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int pse_pair_repulsion(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *group, unsigned N,
                                  double k, double sigma, int accumulate) {
    return pair_repulsion(h, pos, force, group, N, k, sigma, accumulate, false, nullptr);
}
extern "C" int pse_pair_repulsion_virial(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *group, unsigned N,
                                         double k, double sigma, int accumulate, double *out8) {
    return pair_repulsion(h, pos, force, group, N, k, sigma, accumulate, true, out8);
}
extern "C" int pse_pair_repulsion_excl(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *group, unsigned N,
                                       double k, double sigma, int accumulate, double *out8, const pse_exclusions *ex) {
    return pair_repulsion(h, pos, force, group, N, k, sigma, accumulate, out8 != nullptr, out8, "pse_pair_repulsion_excl", ex);
}

// Tabulated pair potential on the same cell list (include/pse_amd.h), with or without the eight observables.  Queue-only wherever
// pse_pair_repulsion is; the table is read by the stream.
static int pair_table(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *group, unsigned N, const double *table,
                      int width, double rmin, double rmax, int accumulate, double *out8, const char *excl, const pse_exclusions *ex) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    TRY(pair_table_validate(h->d.rcut, (unsigned)h->n_max, h->n_slabs, N, pos, force, table, width, rmin, rmax, out8));
    if (excl) TRY(pair_excl_validate(excl, ex, ex ? ex->h : nullptr, h));
    CellPass cp;
    TRY(cp.begin(h, pos, group, N, ex));
    launch_pair_table(h->pos_s, h->tag_s, (int)N, h->cell_off, h->dbox, h->nc, table, width, rmin, rmax, accumulate, (double4 *)force,
                      h->pv_rows, out8, h->stream, cp.rows);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int pse_pair_table(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *group, unsigned N,
                              const double *table, int width, double rmin, double rmax, int accumulate, double *out8) {
    return pair_table(h, pos, force, group, N, table, width, rmin, rmax, accumulate, out8, nullptr, nullptr);
}
extern "C" int pse_pair_table_excl(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *group, unsigned N,
                                   const double *table, int width, double rmin, double rmax, int accumulate, double *out8,
                                   const pse_exclusions *ex) {
    return pair_table(h, pos, force, group, N, table, width, rmin, rmax, accumulate, out8, "pse_pair_table_excl", ex);
}

// ---- bonded forces, angle forces, dihedral forces and pair exclusions (include/pse_amd.h) ------------------------------------------
// The device copy of a topology: the host rows `off` and `ent`, the ntypes parameter sets `par` (none: pair exclusions) and, with
// `counter`, a zeroed counter.
template <class T, class Param>
static int topology_create(const char *who, pse_handle *h, unsigned n, unsigned count, const std::vector<int> &off,
                           const std::vector<unsigned> &ent, const std::vector<Param> &par, bool counter, T **out) {
    T *t = new T();
    t->h = h; t->n = n; t->count = count; t->ntypes = (int)par.size();
    Param *dpar = nullptr;
    hipError_t e = t->put(&t->row_off, off.data(), off.size());
    e = t->put(&t->entries, ent.data(), ent.size());
    if (!par.empty()) e = t->put(&dpar, par.data(), par.size());
    if (counter) e = t->put(&t->over, nullptr, 1, true);
    t->par = dpar;
    return create_end(who, h, t, e, out);
}

extern "C" int pse_bonds_create(pse_handle *h, unsigned n, unsigned nbonds, const unsigned *pairs_host, const unsigned *types_host, int ntypes,
                                const int *kind_host, const double *k_host, const double *r0_host, pse_bonds **out) {
    TRY(create_begin("pse_bonds_create", h, out));
    TRY(bonds_validate((unsigned)h->n_max, n, nbonds, pairs_host, types_host, ntypes, kind_host, k_host, r0_host));
    HIPCHK(hipSetDevice(h->device));
    std::vector<int> off((size_t)n + 1);
    std::vector<unsigned> ent((size_t)nbonds * 4);
    TRY(pse_host_bond_rows(n, nbonds, pairs_host, types_host, off.data(), ent.data()));
    std::vector<BondParam> par((size_t)ntypes);
    for (int t = 0; t < ntypes; ++t)
        par[t] = BondParam{k_host[t], r0_host[t], r0_host[t] > 0.0 ? 1.0 / (r0_host[t] * r0_host[t]) : 0.0, (double)kind_host[t]};
    return topology_create("pse_bonds_create", h, n, nbonds, off, ent, par, true, out);
}
extern "C" int pse_bonds_destroy(pse_bonds *b) { return object_destroy(b); }

// Queue-only: no prepare(), no sort, nothing of the cell list or the kept neighbour list is touched.
extern "C" int pse_bond_forces(pse_bonds *b, const pse_double4 *pos, pse_double4 *force, int accumulate, double *out8) {
    if (!b) return fail(PSE_ERR_INVALID, "pse_bond_forces: null bond object");
    if (!pos) return fail(PSE_ERR_INVALID, "pse_bond_forces: null pos");
    if (!force && !out8) return fail(PSE_ERR_INVALID, "pse_bond_forces: force and out8 are both null: nothing to compute");
    pse_handle *h = b->h;
    HIPCHK(hipSetDevice(h->device));
    launch_bond_forces((const double4 *)pos, (int)b->n, (const unsigned *)b->row_off, (const uint2 *)b->entries, (const BondParam *)b->par,
                       b->ntypes, h->dbox, accumulate, (double4 *)force, h->pv_rows, out8, b->over, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int pse_bonds_overstretched(pse_bonds *b, unsigned long long *count) {
    if (!b || !count) return fail(PSE_ERR_INVALID, "pse_bonds_overstretched: null argument");
    pse_handle *h = b->h;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(count, b->over, sizeof *count, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int pse_angles_create(pse_handle *h, unsigned n, unsigned nangles, const unsigned *triples_host, const unsigned *types_host,
                                 int ntypes, const int *kind_host, const double *k_host, const double *theta0_host, pse_angles **out) {
    TRY(create_begin("pse_angles_create", h, out));
    TRY(angles_validate((unsigned)h->n_max, n, nangles, triples_host, types_host, ntypes, kind_host, k_host, theta0_host));
    HIPCHK(hipSetDevice(h->device));
    std::vector<int> off((size_t)n + 1);
    std::vector<unsigned> ent((size_t)nangles * 12);
    TRY(pse_host_angle_rows(n, nangles, triples_host, types_host, off.data(), ent.data()));
    std::vector<AngleParam> par((size_t)ntypes);
    for (int t = 0; t < ntypes; ++t) par[t] = AngleParam{k_host[t], theta0_host[t], std::cos(theta0_host[t]), (double)kind_host[t]};
    return topology_create("pse_angles_create", h, n, nangles, off, ent, par, false, out);
}
extern "C" int pse_angles_destroy(pse_angles *a) { return object_destroy(a); }

// Queue-only: no prepare(), no sort, nothing of the cell list or the kept neighbour list is touched.
extern "C" int pse_angle_forces(pse_angles *a, const pse_double4 *pos, pse_double4 *force, int accumulate, double *out8) {
    if (!a) return fail(PSE_ERR_INVALID, "pse_angle_forces: null angle object");
    if (!pos) return fail(PSE_ERR_INVALID, "pse_angle_forces: null pos");
    if (!force && !out8) return fail(PSE_ERR_INVALID, "pse_angle_forces: force and out8 are both null: nothing to compute");
    pse_handle *h = a->h;
    HIPCHK(hipSetDevice(h->device));
    launch_angle_forces((const double4 *)pos, (int)a->n, a->row_off, (const uint4 *)a->entries, (const AngleParam *)a->par,
                        a->ntypes, h->dbox, accumulate, (double4 *)force, h->pv_rows, out8, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int pse_dihedrals_create(pse_handle *h, unsigned n, unsigned ndihedrals, const unsigned *quads_host, const unsigned *types_host,
                                    int ntypes, const int *kind_host, const double *params_host, pse_dihedrals **out) {
    TRY(create_begin("pse_dihedrals_create", h, out));
    TRY(dihedrals_validate((unsigned)h->n_max, n, ndihedrals, quads_host, types_host, ntypes, kind_host, params_host));
    HIPCHK(hipSetDevice(h->device));
    std::vector<int> off((size_t)n + 1);
    std::vector<unsigned> ent((size_t)ndihedrals * 20);
    TRY(pse_host_dihedral_rows(n, ndihedrals, quads_host, types_host, off.data(), ent.data()));
    std::vector<DihedralParam> par((size_t)ntypes);
    for (int t = 0; t < ntypes; ++t) {
        const double *p = params_host + 4 * (size_t)t;
        // (d = +-1: the products with it are exact; mult >= 1 marks the harmonic kind, 0 the OPLS kind)
        if (kind_host[t] == PSE_DIHEDRAL_HARMONIC) par[t] = DihedralParam{0.5 * p[0], p[1] * std::cos(p[3]), p[1] * std::sin(p[3]), 0.0, p[2], 0.0};
        else par[t] = DihedralParam{p[0], p[1], p[2], p[3], 0.0, 0.0};
    }
    return topology_create("pse_dihedrals_create", h, n, ndihedrals, off, ent, par, false, out);
}
extern "C" int pse_dihedrals_destroy(pse_dihedrals *d) { return object_destroy(d); }

// Queue-only: no prepare(), no sort, nothing of the cell list or the kept neighbour list is touched.
extern "C" int pse_dihedral_forces(pse_dihedrals *d, const pse_double4 *pos, pse_double4 *force, int accumulate, double *out8) {
    if (!d) return fail(PSE_ERR_INVALID, "pse_dihedral_forces: null dihedral object");
    if (!pos) return fail(PSE_ERR_INVALID, "pse_dihedral_forces: null pos");
    if (!force && !out8) return fail(PSE_ERR_INVALID, "pse_dihedral_forces: force and out8 are both null: nothing to compute");
    pse_handle *h = d->h;
    HIPCHK(hipSetDevice(h->device));
    launch_dihedral_forces((const double4 *)pos, (int)d->n, d->row_off, (const uint4 *)d->entries, d->entries + 16 * (size_t)d->count,
                           (const DihedralParam *)d->par, d->ntypes, h->dbox, accumulate, (double4 *)force, h->pv_rows, out8, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// Pair exclusions (include/pse_amd.h): the rows of pse_host_exclusion_rows on the device, read by the _excl pair passes.
extern "C" int pse_exclusions_create(pse_handle *h, unsigned n, unsigned npairs, const unsigned *pairs_host, pse_exclusions **out) {
    TRY(create_begin("pse_exclusions_create", h, out));
    TRY(exclusions_validate((unsigned)h->n_max, n, npairs, pairs_host));
    HIPCHK(hipSetDevice(h->device));
    std::vector<int> off((size_t)n + 1);
    std::vector<unsigned> ent((size_t)npairs * 2);
    TRY(pse_host_exclusion_rows(n, npairs, pairs_host, off.data(), ent.data()));
    ent.resize((size_t)(unsigned)off[n]);   // duplicates are gone
    return topology_create("pse_exclusions_create", h, n, (unsigned)off[n] / 2, off, ent, std::vector<char>(), false, out);
}
extern "C" int pse_exclusions_destroy(pse_exclusions *ex) { return object_destroy(ex); }

// Typed pair tables (include/pse_amd.h): the types, the concatenated tables and the per-pair-type words on the device, and the pass.
extern "C" int pse_typed_table_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, const int *width_host,
                                      const double *rmin_host, const double *rmax_host, const double *tables_host, pse_typed_table **out) {
    const char *who = "pse_typed_table_create";
    TRY(create_begin(who, h, out));
    TRY(typed_table_validate(h->d.rcut, (unsigned)h->n_max, n, types_host, ntypes, width_host, rmin_host, rmax_host, tables_host));
    HIPCHK(hipSetDevice(h->device));
    const int npt = ntypes * (ntypes + 1) / 2;
    std::vector<int> base(npt);
    std::vector<double> scale(npt), rmax2(npt);
    int total = 0;
    TRY(pse_host_typed_table_layout(ntypes, width_host, rmin_host, rmax_host, base.data(), scale.data(), rmax2.data(), &total));
    pse_typed_table *t = new pse_typed_table();
    t->h = h;
    PairTypedTables &tt = t->tt;
    tt.n = n; tt.ntypes = ntypes; tt.total = total;
    std::vector<double> par((size_t)4 * npt);   // (rmin, rmax2), (scale, {base, width - 2}): an off pair type is all zeros
    for (int p = 0; p < npt; ++p) {
        if (width_host[p] == 0) continue;
        const long long bw = (long long)(unsigned)base[p] | ((long long)(width_host[p] - 2) << 32);
        par[4 * p] = rmin_host[p]; par[4 * p + 1] = rmax2[p]; par[4 * p + 2] = scale[p];
        memcpy(&par[4 * p + 3], &bw, sizeof bw);
        tt.rmax2_all = std::max(tt.rmax2_all, rmax2[p]);
    }
    hipError_t e = t->put(&tt.types, type_bytes(types_host, n).data(), n);
    e = t->put(&tt.type_s, nullptr, (size_t)h->n_max);
    e = t->put(&tt.tables, tables_host, (size_t)total * 2);
    e = t->put(&tt.par, par.data(), par.size());
    return create_end(who, h, t, e, out);
}
extern "C" int pse_typed_table_destroy(pse_typed_table *t) { return object_destroy(t); }
extern "C" int pse_pair_table_typed(pse_typed_table *t, const pse_double4 *pos, pse_double4 *force, const unsigned *group, unsigned N,
                                    int accumulate, double *out8, const pse_exclusions *ex) {
    pse_handle *h = t ? t->h : nullptr;
    TRY(pair_typed_validate(t, h, h ? (unsigned)h->n_max : 0u, h ? h->n_slabs : 1, N, pos, force, out8, ex, ex ? ex->h : nullptr));
    CellPass cp;
    TRY(cp.begin(h, pos, group, N, ex));
    launch_pair_table_typed(h->pos_s, h->tag_s, (int)N, h->cell_off, h->dbox, h->nc, t->tt, accumulate, (double4 *)force, h->pv_rows, out8,
                            h->stream, cp.rows);
    HIPCHK(hipGetLastError());
    return 0;
}

// Pair-distance histograms (include/pse_amd.h): the types on the device, and the pass.  Queue-only: the sort, the type mirror, the
// pass; nothing is read back, the counters are added to by the stream.
extern "C" int pse_pair_hist_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, int nbins, double rmin, double rmax,
                                    pse_pair_hist **out) {
    const char *who = "pse_pair_hist_create";
    TRY(create_begin(who, h, out));
    TRY(pair_hist_create_validate(h->d.rcut, (unsigned)h->n_max, h->n_slabs, n, types_host, ntypes, nbins, rmin, rmax));
    HIPCHK(hipSetDevice(h->device));
    pse_pair_hist *g = new pse_pair_hist();
    g->h = h;
    g->ph.n = n; g->ph.ntypes = ntypes; g->ph.nbins = nbins; g->ph.rmin = rmin; g->ph.rmax = rmax;
    hipError_t e = g->put(&g->ph.types, type_bytes(types_host, n).data(), n);
    e = g->put(&g->ph.type_s, nullptr, (size_t)h->n_max);
    return create_end(who, h, g, e, out);
}
extern "C" int pse_pair_hist_destroy(pse_pair_hist *g) { return object_destroy(g); }
extern "C" int pse_pair_hist_accumulate(pse_pair_hist *g, const pse_double4 *pos, const unsigned *group, unsigned N, unsigned long long *counts,
                                        const pse_exclusions *ex) {
    pse_handle *h = g ? g->h : nullptr;
    TRY(pair_hist_validate(g, h, h ? (unsigned)h->n_max : 0u, N, pos, counts, ex, ex ? ex->h : nullptr));
    CellPass cp;
    TRY(cp.begin(h, pos, group, N, ex));
    launch_pair_hist(h->pos_s, h->tag_s, (int)N, h->cell_off, h->dbox, h->nc, g->ph, counts, h->stream, cp.rows);
    HIPCHK(hipGetLastError());
    return 0;
}

// Static structure factors (include/pse_amd.h): the types, the plan of the modes and the workspace on the device, and the pass.
// Queue-only: no prepare(), no sort, nothing of the cell list or the kept neighbour list is touched; nothing is read back.
extern "C" int pse_structure_factor_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, unsigned nk, const int *modes_host,
                                           pse_structure_factor **out) {
    const char *who = "pse_structure_factor_create";
    TRY(create_begin(who, h, out));
    TRY(structure_factor_create_validate((unsigned)h->n_max, n, types_host, ntypes, nk, modes_host));
    HIPCHK(hipSetDevice(h->device));
    std::vector<unsigned> perm, uoff;
    std::vector<int> segs;
    structure_factor_plan(nk, modes_host, perm, uoff, segs);
    pse_structure_factor *f = new pse_structure_factor();
    f->h = h;
    StructureFactor &sf = f->sf;
    sf.n = n; sf.ntypes = ntypes; sf.nk = (int)nk;
    sf.nseg = (int)(segs.size() / 8);
    for (size_t g = 0; g < segs.size(); g += 8) sf.nlong += segs[g + 3] > SF_SHORT;
    sf.nu = (int)uoff.size() - 1; sf.span = sf_span((unsigned)h->n_max, ntypes, (int)nk);
    hipError_t e = f->put(&sf.types, type_bytes(types_host, n).data(), n);
    e = f->put(&sf.segs, (const int4 *)segs.data(), segs.size() / 4);
    e = f->put(&sf.perm, perm.data(), perm.size());
    e = f->put(&sf.uoff, uoff.data(), uoff.size());
    e = f->put(&sf.rows, nullptr, sf_workspace((unsigned)h->n_max, ntypes, (int)nk));
    return create_end(who, h, f, e, out);
}
extern "C" int pse_structure_factor_destroy(pse_structure_factor *f) { return object_destroy(f); }
extern "C" int pse_structure_factor_accumulate(pse_structure_factor *f, const pse_double4 *pos, const unsigned *group, unsigned N, double *rho,
                                               double *sums) {
    pse_handle *h = f ? f->h : nullptr;
    TRY(structure_factor_validate(f, h ? (unsigned)h->n_max : 0u, N, pos, rho, sums));
    HIPCHK(hipSetDevice(h->device));
    launch_structure_factor((const double4 *)pos, group, (int)N, h->dbox, f->sf, rho, sums, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// Displacement moments (include/pse_amd.h): the types, the slots of unwrapped positions and the workspace on the device, and the
// three passes.  Queue-only: no prepare(), no sort, nothing of the cell list or the kept neighbour list is touched; nothing is read back.
extern "C" int pse_msd_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, int norigins, pse_msd **out) {
    const char *who = "pse_msd_create";
    TRY(create_begin(who, h, out));
    TRY(msd_create_validate((unsigned)h->n_max, n, types_host, ntypes, norigins));
    HIPCHK(hipSetDevice(h->device));
    pse_msd *m = new pse_msd();
    m->h = h;
    m->norigins = norigins;
    m->mo.n = n; m->mo.ntypes = ntypes; m->mo.n_max = (size_t)h->n_max;
    hipError_t e = m->put(&m->mo.types, type_bytes(types_host, n).data(), n);
    e = m->put(&m->mo.planes, nullptr, (size_t)norigins * 3 * m->mo.n_max, true);
    e = m->put(&m->mo.part, nullptr, msd_workspace((unsigned)h->n_max, ntypes));
    return create_end(who, h, m, e, out);
}
extern "C" int pse_msd_destroy(pse_msd *m) { return object_destroy(m); }
extern "C" int pse_msd_store(pse_msd *m, int slot, const pse_double4 *pos, const pse_int3 *image, const unsigned *group, unsigned N, double strain) {
    pse_handle *h = m ? m->h : nullptr;
    TRY(msd_slot_validate("pse_msd_store", m, m ? m->norigins : 0, h ? (unsigned)h->n_max : 0u, slot, N, pos, image, strain));
    HIPCHK(hipSetDevice(h->device));
    launch_msd_store((const double4 *)pos, (const int3 *)image, group, (int)N, h->dbox.Lx, h->dbox.Ly, h->dbox.Lz, strain * h->dbox.Ly,
                     m->mo, slot, nullptr, h->stream);
    HIPCHK(hipGetLastError());
    m->stored |= 1ull << slot;
    return 0;
}
extern "C" int pse_msd_displacement(pse_msd *m, int slot, const pse_double4 *pos, const pse_int3 *image, const unsigned *group, unsigned N,
                                    double strain, pse_double4 *out) {
    pse_handle *h = m ? m->h : nullptr;
    TRY(msd_slot_validate("pse_msd_displacement", m, m ? m->norigins : 0, h ? (unsigned)h->n_max : 0u, slot, N, pos, image, strain));
    TRY(msd_displacement_validate(m->stored, slot, out));
    HIPCHK(hipSetDevice(h->device));
    launch_msd_store((const double4 *)pos, (const int3 *)image, group, (int)N, h->dbox.Lx, h->dbox.Ly, h->dbox.Lz, strain * h->dbox.Ly,
                     m->mo, slot, (double4 *)out, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int pse_msd_accumulate(pse_msd *m, const pse_double4 *pos, const pse_int3 *image, const unsigned *group, unsigned N, double strain,
                                  int npairs, const int *slots_host, const int *rows_host, int nrows, double *sums) {
    pse_handle *h = m ? m->h : nullptr;
    TRY(msd_accumulate_validate(m, m ? m->norigins : 0, m ? m->stored : 0ull, h ? (unsigned)h->n_max : 0u, N, pos, image, strain, npairs,
                                slots_host, rows_host, nrows, sums));
    HIPCHK(hipSetDevice(h->device));
    MsdPairs pairs{};
    pairs.npairs = npairs;
    for (int q = 0; q < npairs; ++q) { pairs.slot[q] = (unsigned char)slots_host[q]; pairs.row[q] = rows_host[q]; }
    launch_msd_accumulate((const double4 *)pos, (const int3 *)image, group, (int)N, h->dbox.Lx, h->dbox.Ly, h->dbox.Lz, strain * h->dbox.Ly,
                          m->mo, pairs, sums, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// Intermediate scattering functions (include/pse_amd.h): the types, the plan of the modes and the workspace of the structure-factor
// pass, the current buffer, the origin slots and the workspace of the self pass -- everything is placed here --, and the passes.
// Queue-only: no prepare(), no sort, nothing of the cell list or the kept neighbour list is touched; nothing is read back.
extern "C" int pse_isf_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, unsigned nk, const int *modes_host, int norigins,
                              pse_isf **out) {
    const char *who = "pse_isf_create";
    TRY(create_begin(who, h, out));
    TRY(isf_create_validate((unsigned)h->n_max, n, types_host, ntypes, nk, modes_host, norigins));
    HIPCHK(hipSetDevice(h->device));
    std::vector<unsigned> perm, uoff;
    std::vector<int> segs;
    structure_factor_plan(nk, modes_host, perm, uoff, segs);
    pse_isf *f = new pse_isf();
    f->h = h;
    f->norigins = norigins;
    Scatter &sc = f->sc;
    StructureFactor &sf = sc.sf;
    sf.n = n; sf.ntypes = ntypes; sf.nk = (int)nk;
    sf.nseg = (int)(segs.size() / 8);
    for (size_t g = 0; g < segs.size(); g += 8) sf.nlong += segs[g + 3] > SF_SHORT;
    sf.nu = (int)uoff.size() - 1; sf.span = sf_span((unsigned)h->n_max, ntypes, (int)nk);
    sc.n_max = (size_t)h->n_max; sc.buf = 3 * sc.n_max + 2 * (size_t)ntypes * nk;
    sc.span = isf_span((unsigned)h->n_max, ntypes, (int)nk);
    hipError_t e = f->put(&sf.types, type_bytes(types_host, n).data(), n);
    e = f->put(&sf.segs, (const int4 *)segs.data(), segs.size() / 4);
    e = f->put(&sf.perm, perm.data(), perm.size());
    e = f->put(&sf.uoff, uoff.data(), uoff.size());
    e = f->put(&sf.rows, nullptr, sf_workspace((unsigned)h->n_max, ntypes, (int)nk));
    e = f->put(&sc.cur, nullptr, sc.buf, true);
    e = f->put(&sc.slots, nullptr, sc.buf * (size_t)norigins, true);
    e = f->put(&sc.part, nullptr, isf_workspace((unsigned)h->n_max, ntypes, (int)nk));
    return create_end(who, h, f, e, out);
}
extern "C" int pse_isf_destroy(pse_isf *f) { return object_destroy(f); }
extern "C" int pse_isf_sample(pse_isf *f, const pse_double4 *pos, const unsigned *group, unsigned N, double *rho, double *static_sums) {
    pse_handle *h = f ? f->h : nullptr;
    TRY(isf_sample_validate(f, h ? (unsigned)h->n_max : 0u, N, pos, rho, static_sums));
    HIPCHK(hipSetDevice(h->device));
    launch_isf_sample((const double4 *)pos, group, (int)N, h->dbox, f->sc, static_sums, h->stream);
    HIPCHK(hipGetLastError());
    f->sample_N = N; f->group = group;
    if (rho)
        HIPCHK(hipMemcpyAsync(rho, f->sc.cur + 3 * f->sc.n_max, (f->sc.buf - 3 * f->sc.n_max) * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return 0;
}
extern "C" int pse_isf_store(pse_isf *f, int slot) {
    TRY(isf_store_validate(f, f ? f->norigins : 0, f ? f->sample_N : 0u, slot));
    pse_handle *h = f->h;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(f->sc.slots + (size_t)slot * f->sc.buf, f->sc.cur, f->sc.buf * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    f->slot_N[slot] = f->sample_N;
    return 0;
}
extern "C" int pse_isf_correlate(pse_isf *f, int npairs, const int *slots_host, const int *rows_host, int nrows, double *self, double *coll) {
    TRY(isf_correlate_validate(f, f ? f->norigins : 0, f ? f->sample_N : 0u, f ? f->slot_N : nullptr, npairs, slots_host, rows_host, nrows, self,
                               coll));
    pse_handle *h = f->h;
    HIPCHK(hipSetDevice(h->device));
    ScatterPairs pairs{};
    pairs.npairs = npairs;
    for (int q = 0; q < npairs; ++q) { pairs.slot[q] = (unsigned char)slots_host[q]; pairs.row[q] = rows_host[q]; }
    if (self) launch_isf_self(f->sc, f->group, (int)f->sample_N, pairs, self, h->stream);
    if (coll) launch_isf_coll(f->sc, pairs, coll, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// Cluster analysis (include/pse_amd.h): the types and the link distances on the device, and the pass.  Queue-only: the sort, the type
// mirror and the four kernels of the union-find; nothing is read back.
extern "C" int pse_clusters_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, const double *rlink_host,
                                   pse_clusters **out) {
    const char *who = "pse_clusters_create";
    TRY(create_begin(who, h, out));
    TRY(clusters_create_validate(h->d.rcut, (unsigned)h->n_max, n, types_host, ntypes, rlink_host));
    HIPCHK(hipSetDevice(h->device));
    std::vector<double> rl2((size_t)(ntypes * (ntypes + 1) / 2));
    pse_clusters *g = new pse_clusters();
    g->h = h;
    ClusterLinks &cl = g->cl;
    cl.n = n; cl.ntypes = ntypes;
    for (size_t p = 0; p < rl2.size(); ++p) { rl2[p] = rlink_host[p] * rlink_host[p]; cl.rl2_all = std::max(cl.rl2_all, rl2[p]); }
    const size_t nm = (size_t)h->n_max;
    hipError_t e = g->put(&cl.types, type_bytes(types_host, n).data(), n);
    e = g->put(&cl.type_s, nullptr, nm);
    e = g->put(&cl.rlink2, rl2.data(), rl2.size());
    e = g->put(&cl.parent, nullptr, 3 * nm + 1, true);   // one array: parent, mintag, csize (n_max each), then the status word
    if (e == hipSuccess) { cl.mintag = cl.parent + nm; cl.csize = cl.parent + 2 * nm; cl.status = cl.parent + 3 * nm; }
    return create_end(who, h, g, e, out);
}
extern "C" int pse_clusters_destroy(pse_clusters *g) { return object_destroy(g); }
extern "C" int pse_clusters_label(pse_clusters *g, const pse_double4 *pos, const unsigned *group, unsigned N, unsigned *label, unsigned *size,
                                  unsigned long long *stats, unsigned long long *hist, unsigned nhist, const pse_exclusions *ex) {
    pse_handle *h = g ? g->h : nullptr;
    TRY(clusters_label_validate(g, h, h ? (unsigned)h->n_max : 0u, h ? h->n_slabs : 1, g ? g->known_status : 0u, N, pos, label, size, stats, hist,
                                nhist, ex, ex ? ex->h : nullptr));
    CellPass cp;
    TRY(cp.begin(h, pos, group, N, ex));
    launch_clusters(h->pos_s, h->tag_s, (int)N, h->cell_off, h->dbox, h->nc, g->cl, label, size, stats, hist, nhist, h->stream, cp.rows);
    HIPCHK(hipGetLastError());
    return 0;
}
// The same pass with the image offsets (pse_percolation.h).  The first call on an object places the scratch: 68 bytes per particle of
// n_max, written by k_span_init before anything reads it.  Queue-only from then on (a capture needs one call before it, as it needs
// the sort's buffers).
extern "C" int pse_clusters_span(pse_clusters *g, const pse_double4 *pos, const unsigned *group, unsigned N, unsigned *label, unsigned *size,
                                 unsigned long long *stats, unsigned long long *hist, unsigned nhist, unsigned *span, int *image, double *rg2,
                                 unsigned long long *pstats, const pse_exclusions *ex) {
    pse_handle *h = g ? g->h : nullptr;
    TRY(clusters_span_validate(g, h, h ? (unsigned)h->n_max : 0u, h ? h->n_slabs : 1, g ? g->known_status : 0u, N, pos, label, size, stats, hist,
                               nhist, span, image, rg2, pstats, ex, ex ? ex->h : nullptr));
    CellPass cp;
    TRY(cp.begin(h, pos, group, N, ex));
    if (!g->sp.word) {
        const size_t nm = (size_t)h->n_max;
        unsigned long long *words = nullptr;
        hipError_t e = g->put(&words, nullptr, 7 * nm);   // one array: word, minkey (n_max each), sums (5 n_max)
        e = g->put(&g->sp.flag, nullptr, nm);
        if (e != hipSuccess) return fail(PSE_ERR_HIP, "pse_clusters_span: placing the scratch of %zu particles on the device failed: %s", nm,
                                         hipGetErrorString(e));
        g->sp.word = words; g->sp.minkey = words + nm; g->sp.sums = words + 2 * nm;
    }
    launch_clusters_span((const double4 *)pos, h->pos_s, h->tag_s, (int)N, h->cell_off, h->dbox, h->nc, g->cl, g->sp, label, size, stats, hist,
                         nhist, span, image, rg2, pstats, h->stream, cp.rows);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int pse_clusters_status(pse_clusters *g, unsigned *status) {
    if (!g) return fail(PSE_ERR_INVALID, "pse_clusters_status: null cluster object");
    if (!status) return fail(PSE_ERR_INVALID, "pse_clusters_status: null status");
    pse_handle *h = g->h;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(&g->known_status, g->cl.status, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *status = g->known_status;
    return 0;
}

// Bond-orientational order (include/pse_amd.h): the types, the neighbour distances and the workspace of the c_lm rows on the device,
// and the two passes.  Queue-only: the sort, the type mirror, one launch per degree and pass; nothing is read back.
extern "C" int pse_bond_order_create(pse_handle *h, unsigned n, const unsigned *types_host, int ntypes, const double *rnb_host, int nl,
                                     const int *degrees_host, pse_bond_order **out) {
    const char *who = "pse_bond_order_create";
    TRY(create_begin(who, h, out));
    TRY(bond_order_create_validate(h->d.rcut, (unsigned)h->n_max, n, types_host, ntypes, rnb_host, nl, degrees_host));
    HIPCHK(hipSetDevice(h->device));
    std::vector<double> rn2((size_t)(ntypes * (ntypes + 1) / 2));
    pse_bond_order *b = new pse_bond_order();
    b->h = h;
    BondOrder &bo = b->bo;
    bo.n = n; bo.ntypes = ntypes; bo.nl = nl;
    for (size_t p = 0; p < rn2.size(); ++p) { rn2[p] = rnb_host[p] * rnb_host[p]; bo.r2_all = std::max(bo.r2_all, rn2[p]); }
    for (int d = 0; d < nl; ++d) { bo.degree[d] = degrees_host[d]; bo.off[d] = bo.stride; bo.stride += degrees_host[d] + 1; }
    const size_t nm = (size_t)h->n_max;
    hipError_t e = b->put(&bo.types, type_bytes(types_host, n).data(), n);
    e = b->put(&bo.type_s, nullptr, nm);
    e = b->put(&bo.rnb2, rn2.data(), rn2.size());
    e = b->put(&bo.clm, nullptr, nm * (size_t)bo.stride);
    e = b->put(&bo.ql_s, nullptr, nm * (size_t)nl);
    return create_end(who, h, b, e, out);
}
extern "C" int pse_bond_order_destroy(pse_bond_order *b) { return object_destroy(b); }
extern "C" int pse_bond_order_compute(pse_bond_order *b, const pse_double4 *pos, const unsigned *group, unsigned N, unsigned *nnb, double *q,
                                      double *qbar, int solid_degree, double threshold, unsigned min_conn, unsigned *nconn,
                                      unsigned long long *stats, const pse_exclusions *ex) {
    pse_handle *h = b ? b->h : nullptr;
    TRY(bond_order_compute_validate(b, h, b ? b->bo.nl : 0, h ? (unsigned)h->n_max : 0u, h ? h->n_slabs : 1, N, pos, nnb, q, qbar, solid_degree,
                                    threshold, nconn, stats, ex, ex ? ex->h : nullptr));
    CellPass cp;
    TRY(cp.begin(h, pos, group, N, ex));
    launch_bond_order(h->pos_s, h->tag_s, (int)N, h->cell_off, h->dbox, h->nc, b->bo, nnb, q, qbar, solid_degree, threshold, min_conn, nconn,
                      stats, h->stream, cp.rows);
    HIPCHK(hipGetLastError());
    return 0;
}
// Queue-only: no prepare(), no sort, nothing of the cell list or the kept neighbour list is touched.
extern "C" int pse_bond_order_histogram(pse_bond_order *b, const double *values, int column, const unsigned *group, unsigned N, int nbins,
                                        double lo, double hi, unsigned long long *counts) {
    pse_handle *h = b ? b->h : nullptr;
    TRY(bond_order_histogram_validate(b, b ? b->bo.nl : 0, b ? b->bo.ntypes : 1, h ? (unsigned)h->n_max : 0u, values, column, N, nbins, lo, hi,
                                      counts));
    HIPCHK(hipSetDevice(h->device));
    launch_bond_order_hist(values, b->bo.nl, column, group, (int)N, (unsigned)h->n_max, b->bo, nbins, lo, hi, counts, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// Chain conformations (include/pse_amd.h): the layout of pse_host_molecule_rows, packed as the kernel reads it (pse_molecules.h), and
// the workspace on the device, and the pass.  Queue-only: no prepare(), no sort, nothing of the cell list or the kept neighbour list is
// touched; nothing is read back.
extern "C" int pse_molecules_create(pse_handle *h, unsigned n, unsigned nbonds, const unsigned *pairs_host, const unsigned *mol_types_host,
                                    int ntypes, int nbins, double rg_max, double ree_max, pse_molecules **out) {
    const char *who = "pse_molecules_create";
    TRY(create_begin(who, h, out));
    MoleculeLayout L;
    TRY(molecules_create_validate((unsigned)h->n_max, n, nbonds, pairs_host, mol_types_host, ntypes, nbins, rg_max, ree_max, L));
    HIPCHK(hipSetDevice(h->device));
    const size_t nmem = L.members.size();
    std::vector<unsigned> word(nmem), mol(nmem), info(L.nmol), tile_slot(L.ntiles + 1), tile_word(L.ntiles);
    auto lg_ceil = [](unsigned v) { unsigned r = 0; while ((1u << r) < v) ++r; return r; };
    for (unsigned t = 0; t < L.ntiles; ++t) {
        const unsigned first = L.mol_off[L.tile_mol[t]];
        unsigned largest = 0;
        tile_slot[t] = first;
        for (unsigned q = L.tile_mol[t]; q < L.tile_mol[t + 1]; ++q) {
            const unsigned o = L.mol_off[q], m = L.mol_off[q + 1] - o;
            largest = std::max(largest, m);
            for (unsigned p = 0; p < m; ++p) {
                word[o + p] = (o - first + L.parent[o + p]) | (p << 10) | ((m - 1u) << 20);
                mol[o + p] = q;
            }
            const bool linear = L.ends[2 * (size_t)q] != 0xffffffffu;
            info[q] = (linear ? L.ends[2 * (size_t)q] | (L.ends[2 * (size_t)q + 1] << 10) | (1u << 24) : 0u) |
                      ((mol_types_host ? mol_types_host[q] : 0u) << 20);
        }
        tile_word[t] = L.tile_rounds[t] | (lg_ceil(largest) << 8) | (lg_ceil(L.tile_mol[t + 1] - L.tile_mol[t]) << 16);
    }
    tile_slot[L.ntiles] = (unsigned)nmem;
    pse_molecules *m = new pse_molecules();
    m->h = h;
    m->nlinear.resize((size_t)ntypes); m->nmol_type.resize((size_t)ntypes);
    molecules_counts(L, mol_types_host, ntypes, nullptr, m->nlinear.data(), m->nmol_type.data());
    Molecules &mo = m->mo;
    mo.nmol = L.nmol; mo.ntiles = L.ntiles; mo.ntypes = ntypes; mo.nbins = nbins;
    mo.f_rg = nbins > 0 ? (double)nbins / rg_max : 0.0;
    mo.f_ree = nbins > 0 ? (double)nbins / ree_max : 0.0;
    hipError_t e = m->put(&mo.member, L.members.data(), nmem);
    e = m->put(&mo.word, word.data(), nmem);
    e = m->put(&mo.mol, mol.data(), nmem);
    e = m->put(&mo.info, info.data(), info.size());
    e = m->put(&mo.tile_slot, tile_slot.data(), tile_slot.size());
    e = m->put(&mo.tile_mol, L.tile_mol.data(), L.tile_mol.size());
    e = m->put(&mo.tile_word, tile_word.data(), tile_word.size());
    e = m->put(&mo.part, nullptr, (size_t)L.ntiles * ntypes * MOL_COLS);
    return create_end(who, h, m, e, out);
}
extern "C" int pse_molecules_destroy(pse_molecules *m) { return object_destroy(m); }
extern "C" int pse_molecules_count(pse_molecules *m, unsigned *nmol, unsigned *nlinear, unsigned *nmol_type) {
    TRY(molecules_count_validate(m, nmol, nlinear, nmol_type));
    if (nmol) *nmol = m->mo.nmol;
    if (nlinear) std::copy(m->nlinear.begin(), m->nlinear.end(), nlinear);
    if (nmol_type) std::copy(m->nmol_type.begin(), m->nmol_type.end(), nmol_type);
    return 0;
}
extern "C" int pse_molecules_compute(pse_molecules *m, const pse_double4 *pos, double *rows, pse_double4 *unfolded, double *sums, double *sample,
                                     unsigned long long *hist) {
    TRY(molecules_compute_validate(m, m ? m->mo.nbins : 0, pos, rows, unfolded, sums, sample, hist));
    pse_handle *h = m->h;
    HIPCHK(hipSetDevice(h->device));
    launch_molecules((const double4 *)pos, h->dbox, m->mo, rows, (double4 *)unfolded, sums, sample, hist, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// Chain statistics (include/pse_amd.h): its own layout of pse_host_molecule_rows with the ranks of pse_host_chain_order, packed as the
// kernel reads it (pse_molpairs.h), the two workspaces of per-tile partial sums, and the pass.  Queue-only, as pse_molecules_compute.
extern "C" int pse_molecule_pairs_create(pse_handle *h, unsigned n, unsigned nbonds, const unsigned *pairs_host, const unsigned *mol_types_host,
                                         int ntypes, int ns, pse_molecule_pairs **out) {
    const char *who = "pse_molecule_pairs_create";
    TRY(create_begin(who, h, out));
    MoleculeLayout L;
    TRY(molecule_pairs_create_validate((unsigned)h->n_max, n, nbonds, pairs_host, mol_types_host, ntypes, ns, L));
    HIPCHK(hipSetDevice(h->device));
    const size_t nmem = L.members.size();
    std::vector<unsigned> rank, word(nmem), mol_word(L.nmol), tile_slot(L.ntiles + 1), tile_word(L.ntiles);
    chain_order(L, rank);
    auto lg_ceil = [](unsigned v) { unsigned r = 0; while ((1u << r) < v) ++r; return r; };
    for (unsigned t = 0; t < L.ntiles; ++t) {
        const unsigned first = L.mol_off[L.tile_mol[t]];
        unsigned largest = 0;
        tile_slot[t] = first;
        for (unsigned q = L.tile_mol[t]; q < L.tile_mol[t + 1]; ++q) {
            const unsigned o = L.mol_off[q], m = L.mol_off[q + 1] - o;
            largest = std::max(largest, m);
            for (unsigned p = 0; p < m; ++p) {
                word[o + p] = (o - first + L.parent[o + p]) | (p << 10) | ((m - 1u) << 20);
                rank[o + p] |= (q - L.tile_mol[t]) << 10;
            }
            const bool linear = L.ends[2 * (size_t)q] != 0xffffffffu;
            mol_word[q] = (o - first) | ((m - 1u) << 10) | ((mol_types_host ? mol_types_host[q] : 0u) << 20) | (linear ? 1u << 24 : 0u);
        }
        tile_word[t] = L.tile_rounds[t] | (lg_ceil(largest) << 8);
    }
    tile_slot[L.ntiles] = (unsigned)nmem;
    pse_molecule_pairs *m = new pse_molecule_pairs();
    m->h = h;
    m->nmol_type.resize((size_t)ntypes);
    molecules_counts(L, mol_types_host, ntypes, nullptr, nullptr, m->nmol_type.data());
    m->terms.resize((size_t)ntypes * ns * MOLPAIR_COLS);
    molecule_pairs_terms(L, mol_types_host, ntypes, ns, m->terms.data());
    MolPairs &mp = m->mp;
    mp.nmol = L.nmol; mp.ntiles = L.ntiles; mp.ntypes = ntypes; mp.ns = ns;
    hipError_t e = m->put(&mp.member, L.members.data(), nmem);
    e = m->put(&mp.word, word.data(), nmem);
    e = m->put(&mp.rank, rank.data(), nmem);
    e = m->put(&mp.mol_word, mol_word.data(), mol_word.size());
    e = m->put(&mp.tile_slot, tile_slot.data(), tile_slot.size());
    e = m->put(&mp.tile_mol, L.tile_mol.data(), L.tile_mol.size());
    e = m->put(&mp.tile_word, tile_word.data(), tile_word.size());
    e = m->put(&mp.part_curves, nullptr, (size_t)L.ntiles * ntypes * ns * MOLPAIR_COLS);
    e = m->put(&mp.part_sums, nullptr, (size_t)L.ntiles * ntypes * MOLPAIR_SUMS);
    return create_end(who, h, m, e, out);
}
extern "C" int pse_molecule_pairs_destroy(pse_molecule_pairs *p) { return object_destroy(p); }
extern "C" int pse_molecule_pairs_counts(pse_molecule_pairs *p, unsigned *nmol, unsigned *nmol_type, unsigned long long *terms) {
    TRY(molecule_pairs_counts_validate(p, nmol, nmol_type, terms));
    if (nmol) *nmol = p->mp.nmol;
    if (nmol_type) std::copy(p->nmol_type.begin(), p->nmol_type.end(), nmol_type);
    if (terms) std::copy(p->terms.begin(), p->terms.end(), terms);
    return 0;
}
extern "C" int pse_molecule_pairs_compute(pse_molecule_pairs *p, const pse_double4 *pos, double *inv_rh, double *curves, double *sums,
                                          double *sample) {
    TRY(molecule_pairs_compute_validate(p, pos, inv_rh, curves, sums, sample));
    pse_handle *h = p->h;
    HIPCHK(hipSetDevice(h->device));
    launch_molecule_pairs((const double4 *)pos, h->dbox, p->mp, inv_rh, curves, sums, sample, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

// Chain normal modes (include/pse_amd.h): its own layout of pse_host_molecule_rows with the ranks of pse_host_chain_order, packed as the
// kernels read it (pse_molmodes.h), the transposed weight tables, the current buffer, the origin slots and the two workspaces of
// partial sums -- everything is placed here --, and the passes.  Queue-only, as pse_molecules_compute.
extern "C" int pse_chain_modes_create(pse_handle *h, unsigned n, unsigned nbonds, const unsigned *pairs_host, const unsigned *mol_types_host,
                                      int ntypes, int nmodes, int nsizes, const unsigned *sizes_host, const double *weights_host, int norigins,
                                      pse_chain_modes **out) {
    const char *who = "pse_chain_modes_create";
    TRY(create_begin(who, h, out));
    MoleculeLayout L;
    TRY(chain_modes_create_validate((unsigned)h->n_max, n, nbonds, pairs_host, mol_types_host, ntypes, nmodes, nsizes, sizes_host, weights_host,
                                    norigins, L));
    HIPCHK(hipSetDevice(h->device));
    const size_t nmem = L.members.size();
    const int K = nmodes;
    // the tables transposed (entry q K + k of a size's block is w_{k,q}), and where the block of every size begins
    std::vector<size_t> table_off((size_t)nsizes + 1, 0);
    for (int s = 0; s < nsizes; ++s) table_off[s + 1] = table_off[s] + (size_t)K * sizes_host[s];
    std::vector<double> wt(table_off[nsizes]);
    for (int s = 0; s < nsizes; ++s)
        for (int k = 0; k < K; ++k)
            for (unsigned q = 0; q < sizes_host[s]; ++q) wt[table_off[s] + (size_t)q * K + k] = weights_host[table_off[s] + (size_t)k * sizes_host[s] + q];
    std::vector<unsigned> rank, word(nmem), mol_word(L.nmol), mol_chunk(L.nmol, 0u), mol_lin(L.nmol, 0xffffffffu), mol_wt(L.nmol, 0u),
        tile_slot(L.ntiles + 1), tile_word(L.ntiles);
    chain_order(L, rank);
    pse_chain_modes *m = new pse_chain_modes();
    m->h = h;
    m->norigins = norigins;
    chain_modes_linear(L, mol_types_host, ntypes, m->lin_mol, m->lin_size, m->nlin_type);
    const size_t nlin = m->lin_mol.size();
    std::vector<unsigned char> lin_type(nlin);
    auto lg_ceil = [](unsigned v) { unsigned r = 0; while ((1u << r) < v) ++r; return r; };
    unsigned jl = 0;
    for (unsigned t = 0; t < L.ntiles; ++t) {
        const unsigned first = L.mol_off[L.tile_mol[t]];
        unsigned largest = 0, chunks = 0;
        tile_slot[t] = first;
        for (unsigned q = L.tile_mol[t]; q < L.tile_mol[t + 1]; ++q) {
            const unsigned o = L.mol_off[q], sz = L.mol_off[q + 1] - o, type = mol_types_host ? mol_types_host[q] : 0u;
            largest = std::max(largest, sz);
            for (unsigned p = 0; p < sz; ++p) {
                word[o + p] = (o - first + L.parent[o + p]) | (p << 10) | ((sz - 1u) << 20);
                rank[o + p] |= (q - L.tile_mol[t]) << 10;
            }
            const bool linear = L.ends[2 * (size_t)q] != 0xffffffffu;
            mol_word[q] = (o - first) | ((sz - 1u) << 10) | (type << 20) | (linear ? 1u << 24 : 0u);
            if (!linear) continue;
            mol_chunk[q] = chunks;
            chunks += (sz + MODE_CHUNK - 1u) / MODE_CHUNK;
            mol_lin[q] = jl;
            lin_type[jl++] = (unsigned char)type;
            mol_wt[q] = (unsigned)table_off[std::lower_bound(sizes_host, sizes_host + nsizes, sz) - sizes_host];
        }
        tile_word[t] = L.tile_rounds[t] | (lg_ceil(largest) << 8) | (chunks << 16);
    }
    tile_slot[L.ntiles] = (unsigned)nmem;
    MolModes &mm = m->mm;
    mm.nmol = L.nmol; mm.ntiles = L.ntiles; mm.nlin = (unsigned)nlin; mm.nblocks = (unsigned)((nlin + MODE_BLOCK - 1) / MODE_BLOCK);
    mm.ntypes = ntypes; mm.K = K;
    const size_t buf = (size_t)3 * K * nlin;
    hipError_t e = m->put(&mm.member, L.members.data(), nmem);
    e = m->put(&mm.word, word.data(), nmem);
    e = m->put(&mm.rank, rank.data(), nmem);
    e = m->put(&mm.mol_word, mol_word.data(), mol_word.size());
    e = m->put(&mm.mol_chunk, mol_chunk.data(), mol_chunk.size());
    e = m->put(&mm.mol_lin, mol_lin.data(), mol_lin.size());
    e = m->put(&mm.mol_wt, mol_wt.data(), mol_wt.size());
    e = m->put(&mm.tile_slot, tile_slot.data(), tile_slot.size());
    e = m->put(&mm.tile_mol, L.tile_mol.data(), L.tile_mol.size());
    e = m->put(&mm.tile_word, tile_word.data(), tile_word.size());
    e = m->put(&mm.lin_type, lin_type.data(), nlin);
    e = m->put(&mm.weights, wt.data(), wt.size());
    e = m->put(&mm.cur, nullptr, buf, true);
    if (norigins > 0) {
        e = m->put(&mm.slots, nullptr, buf * (size_t)norigins, true);
        e = m->put(&mm.part_corr, nullptr, (size_t)mm.nblocks * MODE_MAX_PAIRS * ntypes * K * CHAIN_MODES_CORR);
    }
    e = m->put(&mm.part_static, nullptr, (size_t)L.ntiles * ntypes * K * CHAIN_MODES_STATIC);
    return create_end(who, h, m, e, out);
}
extern "C" int pse_chain_modes_destroy(pse_chain_modes *obj) { return object_destroy(obj); }
extern "C" int pse_chain_modes_counts(pse_chain_modes *obj, unsigned *nmol, unsigned *nlin, unsigned *nlin_type, unsigned *lin_mol, unsigned *lin_size) {
    TRY(chain_modes_counts_validate(obj, nmol, nlin, nlin_type, lin_mol, lin_size));
    if (nmol) *nmol = obj->mm.nmol;
    if (nlin) *nlin = obj->mm.nlin;
    if (nlin_type) std::copy(obj->nlin_type.begin(), obj->nlin_type.end(), nlin_type);
    if (lin_mol) std::copy(obj->lin_mol.begin(), obj->lin_mol.end(), lin_mol);
    if (lin_size) std::copy(obj->lin_size.begin(), obj->lin_size.end(), lin_size);
    return 0;
}
extern "C" int pse_chain_modes_compute(pse_chain_modes *obj, const pse_double4 *pos, double *modes, double *sums, double *sample) {
    TRY(chain_modes_compute_validate(obj, pos, modes, sums, sample));
    pse_handle *h = obj->h;
    HIPCHK(hipSetDevice(h->device));
    launch_chain_modes((const double4 *)pos, h->dbox, obj->mm, modes, sums, sample, h->stream);
    HIPCHK(hipGetLastError());
    obj->computed = true;
    return 0;
}
extern "C" int pse_chain_modes_store(pse_chain_modes *obj, int slot) {
    TRY(chain_modes_store_validate(obj, obj ? obj->norigins : 0, obj ? obj->computed : false, slot));
    pse_handle *h = obj->h;
    HIPCHK(hipSetDevice(h->device));
    const size_t buf = (size_t)3 * obj->mm.K * obj->mm.nlin;
    HIPCHK(hipMemcpyAsync(obj->mm.slots + (size_t)slot * buf, obj->mm.cur, buf * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    obj->stored |= 1ull << slot;
    return 0;
}
extern "C" int pse_chain_modes_correlate(pse_chain_modes *obj, int npairs, const int *slots_host, const int *rows_host, int nrows, double *corr) {
    TRY(chain_modes_correlate_validate(obj, obj ? obj->norigins : 0, obj ? obj->computed : false, obj ? obj->stored : 0ull, npairs, slots_host,
                                       rows_host, nrows, corr));
    pse_handle *h = obj->h;
    HIPCHK(hipSetDevice(h->device));
    ModePairs pairs{};
    pairs.npairs = npairs;
    for (int q = 0; q < npairs; ++q) { pairs.slot[q] = (unsigned char)slots_host[q]; pairs.row[q] = rows_host[q]; }
    launch_chain_modes_correlate(obj->mm, pairs, corr, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}
