// The part of the C-ABI (include/pse_amd.h) that never touches a device: the error text, the parameter rule of
// Stokes::setParams without a handle (PSEv1/Stokes.cc:129-236,319), the Lanczos tridiagonal square root
// (LAPACKE_spteqr + the host loops at PSEv1/Brownian.cu:540-582) and the host-checked drivers' decision on given
// coefficients (lz_decide_host).  Plain C++: linked into libpse_amd.so, and -- with
// pse_params.cpp and a stub of the device entry points -- into the sanitizer build that the CPU tests run against.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pse_err.h"
#include "pse_cluster_word.h"

namespace pse {

std::string &error_text() {
    static thread_local std::string text;
    return text;
}

int fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    error_text() = buf;
    return code;
}

void fill_info(const Derived &d, pse_info *o) {
    memset(o, 0, sizeof *o);
    o->Nx = d.Nx; o->Ny = d.Ny; o->Nz = d.Nz; o->P = d.P;
    o->rcut = d.rcut; o->xi = d.xi; o->eta = d.eta; o->gaussm = d.gaussm; o->lambda = d.lambda;
    o->self_mobility = d.self; o->hx = d.hx; o->hy = d.hy; o->hz = d.hz;
}

// The spreading Gaussian exp(-c r^2), c = 2 xi^2 / eta, has its width from the SMALLEST grid spacing (the reference's rule makes the
// three spacings equal up to the rounding of the grid sizes, PSEv1/Stokes.cc:147-214); spread and gather build its P values per axis
// by a product recurrence whose factors reach exp(c h^2 P) and whose values fall to exp(-c h^2 P^2 / 4).  A grid or box override whose
// coarsest spacing puts those outside the double range would turn into NaN velocities: refused.
int gaussian_fits(const Derived &d, double hx, double hy, double hz) {
    const double c = 2.0 * d.xi * d.xi / d.eta, hmax = std::max(hx, std::max(hy, hz));
    const double worst = c * hmax * hmax * std::max((double)d.P, 0.25 * d.P * d.P);
    if (!(worst < 700.0))
        return fail(PSE_ERR_INVALID, "grid spacings (%g, %g, %g) too unequal for the spreading Gaussian of P = %d points, eta = %g: "
                    "exp(+-%.0f) over its support on the coarsest axis", hx, hy, hz, d.P, d.eta, worst);
    return 0;
}

int lz_decisions_validate(const char *who, const double *scal_host, int n_dec, const pse_debug_lz_decision *dec, const void *out) {
    if (!scal_host || !dec || !out) return fail(PSE_ERR_INVALID, "%s: null argument", who);
    if (n_dec < 1 || n_dec > 40) return fail(PSE_ERR_INVALID, "%s: %d decisions outside [1, 40]", who, n_dec);
    if (!dec[0].first) return fail(PSE_ERR_INVALID, "%s: the first decision must reset the state (first = 1)", who);
    for (int k = 0; k < n_dec; ++k) {
        const pse_debug_lz_decision &d = dec[k];
        if (d.m_lo < 1 || d.m_lo > d.m_hi) return fail(PSE_ERR_INVALID, "%s: decision %d: m_lo = %d outside [1, m_hi = %d]", who, k, d.m_lo, d.m_hi);
        if (d.done_iters < d.m_hi || d.done_iters > M_MAX)
            return fail(PSE_ERR_INVALID, "%s: decision %d: done_iters = %d outside [m_hi, %d]", who, k, d.done_iters, M_MAX);
        if (d.pending_beta < 0 || d.pending_beta > d.m_hi)
            return fail(PSE_ERR_INVALID, "%s: decision %d: pending_beta = %d outside [0, m_hi]", who, k, d.pending_beta);
        if (d.m_max > M_MAX) return fail(PSE_ERR_INVALID, "%s: decision %d: m_max = %d above %d", who, k, d.m_max, M_MAX);
    }
    return 0;
}

LzDecide lz_decision(const pse_debug_lz_decision &d) {
    LzDecide a{};
    a.m_lo = d.m_lo; a.m_hi = d.m_hi; a.done_iters = d.done_iters; a.have_last_beta = d.have_last_beta; a.pending_beta = d.pending_beta;
    a.first = d.first; a.last = d.last; a.normalised = d.normalised; a.m_max = d.m_max; a.tol = d.tol;
    return a;
}

void lz_outcome(const LzState &st, pse_debug_lz_outcome *o) {
    o->done = st.done; o->m_final = st.m_final; o->checked = st.checked; o->status = st.status; o->stepnorm = st.stepnorm;
    std::copy(st.t_prev, st.t_prev + 104, o->t_prev);
    std::copy(st.coef, st.coef + 104, o->coef);
}

static int count_in_range(unsigned n_max, unsigned N) {
    if (N == 0 || N > n_max) return fail(PSE_ERR_INVALID, "N = %u outside (0, n_max = %u]", N, n_max);
    return 0;
}

int pair_repulsion_validate(double rcut, unsigned n_max, int n_slabs, unsigned N, const void *pos, const void *force, bool virial,
                            const void *out8, double sigma) {
    if (int rc = count_in_range(n_max, N)) return rc;
    if (!pos || (!virial && !force)) return fail(PSE_ERR_INVALID, "null array");
    if (virial && !out8) return fail(PSE_ERR_INVALID, "null out8: the observables need eight device doubles");
    if (virial && n_slabs > 1)
        return fail(PSE_ERR_INVALID, "pse_pair_repulsion_virial: this handle is a slab rank (n_slabs = %d): it orders only its own cells, the sums "
                                     "would be partial", n_slabs);
    if (!(sigma > 0.0) || sigma > rcut)
        return fail(PSE_ERR_INVALID, "repulsion range %.4f outside (0, rcut = %.4f]: the cell list is built for the hydrodynamic cutoff", sigma, rcut);
    return 0;
}

int pair_table_validate(double rcut, unsigned n_max, int n_slabs, unsigned N, const void *pos, const void *force, const double *table, int width,
                        double rmin, double rmax, const void *out8) {
    if (int rc = count_in_range(n_max, N)) return rc;
    if (!pos) return fail(PSE_ERR_INVALID, "pse_pair_table: null pos");
    if (!table) return fail(PSE_ERR_INVALID, "pse_pair_table: null table");
    if (((uintptr_t)table & 15u) != 0) return fail(PSE_ERR_INVALID, "pse_pair_table: the table is not 16-byte aligned (it is read as (V, F) entries)");
    if (!force && !out8) return fail(PSE_ERR_INVALID, "pse_pair_table: force and out8 are both null: nothing to compute");
    if (width < 2 || width > PAIR_TABLE_MAX_WIDTH)
        return fail(PSE_ERR_INVALID, "pse_pair_table: table width %d outside [2, %d] (the table is staged in 32 KB of LDS)", width, PAIR_TABLE_MAX_WIDTH);
    if (!std::isfinite(rmin) || !std::isfinite(rmax)) return fail(PSE_ERR_INVALID, "pse_pair_table: rmin = %g, rmax = %g must be finite", rmin, rmax);
    if (rmin < 0.0) return fail(PSE_ERR_INVALID, "pse_pair_table: rmin = %g is negative", rmin);
    if (!(rmax > rmin)) return fail(PSE_ERR_INVALID, "pse_pair_table: rmax = %g must exceed rmin = %g", rmax, rmin);
    if (rmax > rcut)
        return fail(PSE_ERR_INVALID, "pse_pair_table: table range rmax = %.4f beyond rcut = %.4f: the cell list is built for the hydrodynamic cutoff",
                    rmax, rcut);
    if (out8 && n_slabs > 1)
        return fail(PSE_ERR_INVALID, "pse_pair_table: this handle is a slab rank (n_slabs = %d): it orders only its own cells, the sums would be "
                                     "partial (out8 must be null here)", n_slabs);
    return 0;
}

int bonds_validate(unsigned n_max, unsigned n, unsigned nbonds, const unsigned *pairs, const unsigned *types, int ntypes, const int *kind,
                   const double *k, const double *r0) {
    if (!pairs) return fail(PSE_ERR_INVALID, "pse_bonds_create: null pairs_host");
    if (!kind || !k || !r0) return fail(PSE_ERR_INVALID, "pse_bonds_create: null parameter array (kind_host, k_host, r0_host)");
    if (n == 0 || n > n_max) return fail(PSE_ERR_INVALID, "pse_bonds_create: n = %u outside (0, n_max = %u]", n, n_max);
    if (nbonds == 0 || nbonds > (1u << 30)) return fail(PSE_ERR_INVALID, "pse_bonds_create: nbonds = %u outside (0, 2^30]", nbonds);
    if (ntypes < 1 || ntypes > BOND_MAX_TYPES) return fail(PSE_ERR_INVALID, "pse_bonds_create: ntypes = %d outside [1, %d]", ntypes, BOND_MAX_TYPES);
    for (int t = 0; t < ntypes; ++t) {
        if (kind[t] != PSE_BOND_HARMONIC && kind[t] != PSE_BOND_FENE)
            return fail(PSE_ERR_INVALID, "pse_bonds_create: type %d has kind %d, neither PSE_BOND_HARMONIC nor PSE_BOND_FENE", t, kind[t]);
        if (!std::isfinite(k[t]) || !std::isfinite(r0[t]))
            return fail(PSE_ERR_INVALID, "pse_bonds_create: type %d has k = %g, r0 = %g: both must be finite", t, k[t], r0[t]);
        if (r0[t] < 0.0) return fail(PSE_ERR_INVALID, "pse_bonds_create: type %d has r0 = %g < 0", t, r0[t]);
        if (kind[t] == PSE_BOND_FENE && !(r0[t] > 0.0)) return fail(PSE_ERR_INVALID, "pse_bonds_create: FENE type %d needs r0 > 0, not %g", t, r0[t]);
    }
    for (unsigned b = 0; b < nbonds; ++b) {
        const unsigned i = pairs[2 * (size_t)b], j = pairs[2 * (size_t)b + 1];
        if (i >= n || j >= n) return fail(PSE_ERR_INVALID, "pse_bonds_create: bond %u = (%u, %u) has an endpoint >= n = %u", b, i, j, n);
        if (i == j) return fail(PSE_ERR_INVALID, "pse_bonds_create: bond %u joins particle %u to itself", b, i);
        if (types && types[b] >= (unsigned)ntypes) return fail(PSE_ERR_INVALID, "pse_bonds_create: bond %u has type %u >= ntypes = %d", b, types[b], ntypes);
    }
    return 0;
}

int angles_validate(unsigned n_max, unsigned n, unsigned nangles, const unsigned *triples, const unsigned *types, int ntypes,
                    const int *kind, const double *k, const double *theta0) {
    if (!triples) return fail(PSE_ERR_INVALID, "pse_angles_create: null triples_host");
    if (!kind || !k || !theta0) return fail(PSE_ERR_INVALID, "pse_angles_create: null parameter array (kind_host, k_host, theta0_host)");
    if (n == 0 || n > n_max) return fail(PSE_ERR_INVALID, "pse_angles_create: n = %u outside (0, n_max = %u]", n, n_max);
    if (nangles == 0 || nangles > (1u << 28)) return fail(PSE_ERR_INVALID, "pse_angles_create: nangles = %u outside (0, 2^28]", nangles);
    if (ntypes < 1 || ntypes > ANGLE_MAX_TYPES) return fail(PSE_ERR_INVALID, "pse_angles_create: ntypes = %d outside [1, %d]", ntypes, ANGLE_MAX_TYPES);
    const double pi = 3.14159265358979323846;
    for (int t = 0; t < ntypes; ++t) {
        if (kind[t] != PSE_ANGLE_HARMONIC && kind[t] != PSE_ANGLE_COSINESQ)
            return fail(PSE_ERR_INVALID, "pse_angles_create: type %d has kind %d, neither PSE_ANGLE_HARMONIC nor PSE_ANGLE_COSINESQ", t, kind[t]);
        if (!std::isfinite(k[t]) || !std::isfinite(theta0[t]))
            return fail(PSE_ERR_INVALID, "pse_angles_create: type %d has k = %g, theta0 = %g: both must be finite", t, k[t], theta0[t]);
        if (theta0[t] < 0.0 || theta0[t] > pi) return fail(PSE_ERR_INVALID, "pse_angles_create: type %d has theta0 = %g outside [0, pi]", t, theta0[t]);
    }
    for (unsigned a = 0; a < nangles; ++a) {
        const unsigned i = triples[3 * (size_t)a], j = triples[3 * (size_t)a + 1], l = triples[3 * (size_t)a + 2];
        if (i >= n || j >= n || l >= n)
            return fail(PSE_ERR_INVALID, "pse_angles_create: angle %u = (%u, %u, %u) has an index >= n = %u", a, i, j, l, n);
        if (i == j || j == l || i == l)
            return fail(PSE_ERR_INVALID, "pse_angles_create: angle %u = (%u, %u, %u) has two equal members", a, i, j, l);
        if (types && types[a] >= (unsigned)ntypes) return fail(PSE_ERR_INVALID, "pse_angles_create: angle %u has type %u >= ntypes = %d", a, types[a], ntypes);
    }
    return 0;
}

int dihedrals_validate(unsigned n_max, unsigned n, unsigned ndihedrals, const unsigned *quads, const unsigned *types, int ntypes,
                       const int *kind, const double *params) {
    if (!quads) return fail(PSE_ERR_INVALID, "pse_dihedrals_create: null quads_host");
    if (!kind || !params) return fail(PSE_ERR_INVALID, "pse_dihedrals_create: null parameter array (kind_host, params_host)");
    if (n == 0 || n > n_max) return fail(PSE_ERR_INVALID, "pse_dihedrals_create: n = %u outside (0, n_max = %u]", n, n_max);
    if (ndihedrals == 0 || ndihedrals > (1u << 28))
        return fail(PSE_ERR_INVALID, "pse_dihedrals_create: ndihedrals = %u outside (0, 2^28]", ndihedrals);
    if (ntypes < 1 || ntypes > DIHEDRAL_MAX_TYPES)
        return fail(PSE_ERR_INVALID, "pse_dihedrals_create: ntypes = %d outside [1, %d]", ntypes, DIHEDRAL_MAX_TYPES);
    for (int t = 0; t < ntypes; ++t) {
        const double *p = params + 4 * (size_t)t;
        if (kind[t] != PSE_DIHEDRAL_HARMONIC && kind[t] != PSE_DIHEDRAL_OPLS)
            return fail(PSE_ERR_INVALID, "pse_dihedrals_create: type %d has kind %d, neither PSE_DIHEDRAL_HARMONIC nor PSE_DIHEDRAL_OPLS", t, kind[t]);
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]) || !std::isfinite(p[3]))
            return fail(PSE_ERR_INVALID, "pse_dihedrals_create: type %d has params = (%g, %g, %g, %g): all four must be finite", t, p[0], p[1], p[2], p[3]);
        if (kind[t] == PSE_DIHEDRAL_HARMONIC) {
            if (p[1] != -1.0 && p[1] != 1.0) return fail(PSE_ERR_INVALID, "pse_dihedrals_create: harmonic type %d has d = %g, neither -1 nor +1", t, p[1]);
            if (p[2] != std::floor(p[2]) || p[2] < 1.0 || p[2] > 6.0)
                return fail(PSE_ERR_INVALID, "pse_dihedrals_create: harmonic type %d has mult = %g, not an integer in [1, 6]", t, p[2]);
        }
    }
    for (unsigned a = 0; a < ndihedrals; ++a) {
        const unsigned *q = quads + 4 * (size_t)a;
        if (q[0] >= n || q[1] >= n || q[2] >= n || q[3] >= n)
            return fail(PSE_ERR_INVALID, "pse_dihedrals_create: dihedral %u = (%u, %u, %u, %u) has an index >= n = %u", a, q[0], q[1], q[2], q[3], n);
        if (q[0] == q[1] || q[0] == q[2] || q[0] == q[3] || q[1] == q[2] || q[1] == q[3] || q[2] == q[3])
            return fail(PSE_ERR_INVALID, "pse_dihedrals_create: dihedral %u = (%u, %u, %u, %u) has two equal members", a, q[0], q[1], q[2], q[3]);
        if (types && types[a] >= (unsigned)ntypes)
            return fail(PSE_ERR_INVALID, "pse_dihedrals_create: dihedral %u has type %u >= ntypes = %d", a, types[a], ntypes);
    }
    return 0;
}

int exclusions_validate(unsigned n_max, unsigned n, unsigned npairs, const unsigned *pairs) {
    if (!pairs) return fail(PSE_ERR_INVALID, "pse_exclusions_create: null pairs_host");
    if (n == 0 || n > n_max) return fail(PSE_ERR_INVALID, "pse_exclusions_create: n = %u outside (0, n_max = %u]", n, n_max);
    if (npairs == 0 || npairs > (1u << 30)) return fail(PSE_ERR_INVALID, "pse_exclusions_create: npairs = %u outside (0, 2^30]", npairs);
    for (unsigned b = 0; b < npairs; ++b) {
        const unsigned i = pairs[2 * (size_t)b], j = pairs[2 * (size_t)b + 1];
        if (i >= n || j >= n) return fail(PSE_ERR_INVALID, "pse_exclusions_create: pair %u = (%u, %u) has an index >= n = %u", b, i, j, n);
        if (i == j) return fail(PSE_ERR_INVALID, "pse_exclusions_create: pair %u excludes particle %u from itself", b, i);
    }
    return 0;
}

int pair_excl_validate(const char *who, const void *ex, const void *ex_handle, const void *h) {
    if (!ex) return fail(PSE_ERR_INVALID, "%s: null exclusion object", who);
    if (ex_handle != h) return fail(PSE_ERR_INVALID, "%s: the exclusion object was created on another handle", who);
    return 0;
}

// What the create validators of the typed objects (typed tables, histograms, structure factors, displacement origins, clusters) share,
// under the name `who` of the entry point: n and, with `with_ntypes`, ntypes ...
static int sizes_in_range(const char *who, unsigned n_max, unsigned n, int ntypes, bool with_ntypes = true) {
    if (n == 0 || n > n_max) return fail(PSE_ERR_INVALID, "%s: n = %u outside (0, n_max = %u]", who, n, n_max);
    if (with_ntypes && (ntypes < 1 || ntypes > PAIR_TYPED_MAX_TYPES))
        return fail(PSE_ERR_INVALID, "%s: ntypes = %d outside [1, %d]", who, ntypes, PAIR_TYPED_MAX_TYPES);
    return 0;
}
// ... and the type of every particle (types null: one type, nothing to check)
static int types_in_range(const char *who, unsigned n, const unsigned *types, int ntypes) {
    if (types)
        for (unsigned i = 0; i < n; ++i)
            if (types[i] >= (unsigned)ntypes) return fail(PSE_ERR_INVALID, "%s: particle %u has type %u >= ntypes = %d", who, i, types[i], ntypes);
    return 0;
}

// What pse_host_typed_table_layout computes and refuses, under the name `who` of the entry point that asks.
static int typed_layout(const char *who, int ntypes, const int *width, const double *rmin, const double *rmax, int *base, double *scale,
                        double *rmax2, int *total) {
    if (!width || !rmin || !rmax) return fail(PSE_ERR_INVALID, "%s: null array (width, rmin, rmax)", who);
    if (ntypes < 1 || ntypes > PAIR_TYPED_MAX_TYPES) return fail(PSE_ERR_INVALID, "%s: ntypes = %d outside [1, %d]", who, ntypes, PAIR_TYPED_MAX_TYPES);
    const int npt = ntypes * (ntypes + 1) / 2;
    long long sum = 0;
    for (int p = 0; p < npt; ++p) {
        if (width[p] < 0 || width[p] == 1 || width[p] > PAIR_TABLE_MAX_WIDTH)
            return fail(PSE_ERR_INVALID, "%s: pair type %d has width %d, neither 0 (off) nor in [2, %d]", who, p, width[p], PAIR_TABLE_MAX_WIDTH);
        sum += width[p];
        if (width[p] == 0) continue;
        if (!std::isfinite(rmin[p]) || !std::isfinite(rmax[p]))
            return fail(PSE_ERR_INVALID, "%s: pair type %d: rmin = %g, rmax = %g must be finite", who, p, rmin[p], rmax[p]);
        if (rmin[p] < 0.0) return fail(PSE_ERR_INVALID, "%s: pair type %d: rmin = %g is negative", who, p, rmin[p]);
        if (!(rmax[p] > rmin[p])) return fail(PSE_ERR_INVALID, "%s: pair type %d: rmax = %g must exceed rmin = %g", who, p, rmax[p], rmin[p]);
    }
    if (sum == 0) return fail(PSE_ERR_INVALID, "%s: all widths are zero: every pair type is off", who);
    if (sum > PAIR_TYPED_MAX_ENTRIES)
        return fail(PSE_ERR_INVALID, "%s: the widths sum to %lld entries, more than %d (the tables are staged together in 56 KB of LDS)", who, sum,
                    PAIR_TYPED_MAX_ENTRIES);
    int at = 0;
    for (int p = 0; p < npt; ++p) {
        const bool on = width[p] != 0;
        if (base) base[p] = at;
        if (scale) scale[p] = on ? (double)(width[p] - 1) / (rmax[p] - rmin[p]) : 0.0;
        if (rmax2) rmax2[p] = on ? rmax[p] * rmax[p] : 0.0;
        at += width[p];
    }
    if (total) *total = at;
    return 0;
}

int typed_table_validate(double rcut, unsigned n_max, unsigned n, const unsigned *types, int ntypes, const int *width, const double *rmin,
                         const double *rmax, const double *tables) {
    const char *who = "pse_typed_table_create";
    if (!types) return fail(PSE_ERR_INVALID, "%s: null types_host", who);
    if (!tables) return fail(PSE_ERR_INVALID, "%s: null tables_host", who);
    if (int rc = sizes_in_range(who, n_max, n, ntypes, false)) return rc;   // (ntypes: behind the null arrays, in typed_layout)
    int total = 0;
    if (int rc = typed_layout(who, ntypes, width, rmin, rmax, nullptr, nullptr, nullptr, &total)) return rc;
    if (int rc = types_in_range(who, n, types, ntypes)) return rc;
    for (int p = 0; p < ntypes * (ntypes + 1) / 2; ++p)
        if (width[p] != 0 && rmax[p] > rcut)
            return fail(PSE_ERR_INVALID, "%s: pair type %d: table range rmax = %.4f beyond rcut = %.4f: the cell list is built for the hydrodynamic "
                                         "cutoff", who, p, rmax[p], rcut);
    for (int e = 0; e < 2 * total; ++e)
        if (!std::isfinite(tables[e])) return fail(PSE_ERR_INVALID, "%s: table entry %d (%s) = %g is not finite", who, e / 2, e % 2 ? "F" : "V", tables[e]);
    return 0;
}

int pair_typed_validate(const void *t, const void *t_handle, unsigned n_max, int n_slabs, unsigned N, const void *pos, const void *force,
                        const void *out8, const void *ex, const void *ex_handle) {
    if (!t) return fail(PSE_ERR_INVALID, "pse_pair_table_typed: null typed table");
    if (int rc = count_in_range(n_max, N)) return rc;
    if (!pos) return fail(PSE_ERR_INVALID, "pse_pair_table_typed: null pos");
    if (!force && !out8) return fail(PSE_ERR_INVALID, "pse_pair_table_typed: force and out8 are both null: nothing to compute");
    if (out8 && n_slabs > 1)
        return fail(PSE_ERR_INVALID, "pse_pair_table_typed: this handle is a slab rank (n_slabs = %d): it orders only its own cells, the sums would "
                                     "be partial (out8 must be null here)", n_slabs);
    if (ex) return pair_excl_validate("pse_pair_table_typed", ex, ex_handle, t_handle);
    return 0;
}

int pair_hist_create_validate(double rcut, unsigned n_max, int n_slabs, unsigned n, const unsigned *types, int ntypes, int nbins, double rmin,
                              double rmax) {
    const char *who = "pse_pair_hist_create";
    if (int rc = sizes_in_range(who, n_max, n, ntypes)) return rc;
    if (nbins < 1) return fail(PSE_ERR_INVALID, "%s: nbins = %d, need at least one bin", who, nbins);
    const long long npt = ntypes * (ntypes + 1) / 2;
    if (npt * nbins > PAIR_HIST_MAX_COUNTERS)
        return fail(PSE_ERR_INVALID, "%s: %lld pair types x %d bins = %lld counters, more than %d (the counters are kept in 32 KB of LDS)", who, npt,
                    nbins, npt * nbins, PAIR_HIST_MAX_COUNTERS);
    if (!std::isfinite(rmin) || !std::isfinite(rmax)) return fail(PSE_ERR_INVALID, "%s: rmin = %g, rmax = %g must be finite", who, rmin, rmax);
    if (rmin < 0.0) return fail(PSE_ERR_INVALID, "%s: rmin = %g is negative", who, rmin);
    if (!(rmax > rmin)) return fail(PSE_ERR_INVALID, "%s: rmax = %g must exceed rmin = %g", who, rmax, rmin);
    if (rmax > rcut)
        return fail(PSE_ERR_INVALID, "%s: histogram range rmax = %.4f beyond rcut = %.4f: the cell list is built for the hydrodynamic cutoff", who,
                    rmax, rcut);
    if (n_slabs > 1)
        return fail(PSE_ERR_INVALID, "%s: this handle is a slab rank (n_slabs = %d): it orders only its own cells, the counts would be partial", who,
                    n_slabs);
    if (int rc = types_in_range(who, n, types, ntypes)) return rc;
    return 0;
}

int pair_hist_validate(const void *g, const void *g_handle, unsigned n_max, unsigned N, const void *pos, const void *counts, const void *ex,
                       const void *ex_handle) {
    const char *who = "pse_pair_hist_accumulate";
    if (!g) return fail(PSE_ERR_INVALID, "%s: null histogram object", who);
    if (N == 0 || N > n_max) return fail(PSE_ERR_INVALID, "%s: N = %u outside (0, n_max = %u]", who, N, n_max);
    if (!pos) return fail(PSE_ERR_INVALID, "%s: null pos", who);
    if (!counts) return fail(PSE_ERR_INVALID, "%s: null counts", who);
    if (((uintptr_t)counts & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: counts is not 8-byte aligned (64-bit counters)", who);
    if (ex) return pair_excl_validate(who, ex, ex_handle, g_handle);
    return 0;
}

// what pse_structure_factor_create and pse_isf_create (`who`) refuse alike: the sizes, nk against the cap of the object, the modes, the types
static int mode_list_validate(const char *who, unsigned n_max, unsigned n, const unsigned *types, int ntypes, unsigned nk, int nk_max,
                              const int *modes) {
    if (int rc = sizes_in_range(who, n_max, n, ntypes)) return rc;
    if (nk == 0 || nk > (unsigned)nk_max) return fail(PSE_ERR_INVALID, "%s: nk = %u outside [1, %d]", who, nk, nk_max);
    if (!modes) return fail(PSE_ERR_INVALID, "%s: null modes_host", who);
    for (unsigned q = 0; q < nk; ++q)
        for (int c = 0; c < 3; ++c)
            if (modes[3 * (size_t)q + c] > SF_MAX_INDEX || modes[3 * (size_t)q + c] < -SF_MAX_INDEX)
                return fail(PSE_ERR_INVALID, "%s: mode %u has the index m%c = %d beyond +-%d", who, q, "xyz"[c], modes[3 * (size_t)q + c], SF_MAX_INDEX);
    if (int rc = types_in_range(who, n, types, ntypes)) return rc;
    return 0;
}

int structure_factor_create_validate(unsigned n_max, unsigned n, const unsigned *types, int ntypes, unsigned nk, const int *modes) {
    return mode_list_validate("pse_structure_factor_create", n_max, n, types, ntypes, nk, SF_MAX_MODES, modes);
}

int structure_factor_validate(const void *f, unsigned n_max, unsigned N, const void *pos, const void *rho, const void *sums) {
    const char *who = "pse_structure_factor_accumulate";
    if (!f) return fail(PSE_ERR_INVALID, "%s: null structure-factor object", who);
    if (N == 0 || N > n_max) return fail(PSE_ERR_INVALID, "%s: N = %u outside (0, n_max = %u]", who, N, n_max);
    if (!pos) return fail(PSE_ERR_INVALID, "%s: null pos", who);
    if (!rho && !sums) return fail(PSE_ERR_INVALID, "%s: rho and sums are both null: nothing to compute", who);
    if (((uintptr_t)rho & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: rho = %p is not 8-byte aligned (doubles)", who, rho);
    if (((uintptr_t)sums & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: sums = %p is not 8-byte aligned (doubles)", who, sums);
    return 0;
}

int msd_create_validate(unsigned n_max, unsigned n, const unsigned *types, int ntypes, int norigins) {
    const char *who = "pse_msd_create";
    if (int rc = sizes_in_range(who, n_max, n, ntypes)) return rc;
    if (norigins < 1 || norigins > MSD_MAX_ORIGINS) return fail(PSE_ERR_INVALID, "%s: norigins = %d outside [1, %d]", who, norigins, MSD_MAX_ORIGINS);
    if (int rc = types_in_range(who, n, types, ntypes)) return rc;
    return 0;
}

int msd_slot_validate(const char *who, const void *m, int norigins, unsigned n_max, int slot, unsigned N, const void *pos, const void *image,
                      double strain) {
    if (!m) return fail(PSE_ERR_INVALID, "%s: null displacement object", who);
    if (slot < 0 || slot >= norigins) return fail(PSE_ERR_INVALID, "%s: slot = %d outside [0, norigins = %d)", who, slot, norigins);
    if (N == 0 || N > n_max) return fail(PSE_ERR_INVALID, "%s: N = %u outside (0, n_max = %u]", who, N, n_max);
    if (!pos) return fail(PSE_ERR_INVALID, "%s: null pos", who);
    if (!image) return fail(PSE_ERR_INVALID, "%s: null image", who);
    if (!std::isfinite(strain)) return fail(PSE_ERR_INVALID, "%s: strain = %g is not finite", who, strain);
    return 0;
}

int msd_displacement_validate(unsigned long long stored, int slot, const void *out) {
    const char *who = "pse_msd_displacement";
    if (!((stored >> slot) & 1ull)) return fail(PSE_ERR_INVALID, "%s: slot %d was never stored", who, slot);
    if (!out) return fail(PSE_ERR_INVALID, "%s: null out", who);
    if (((uintptr_t)out & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: out = %p is not 8-byte aligned (doubles)", who, out);
    return 0;
}

int msd_accumulate_validate(const void *m, int norigins, unsigned long long stored, unsigned n_max, unsigned N, const void *pos,
                            const void *image, double strain, int npairs, const int *slots, const int *rows, int nrows, const void *sums) {
    const char *who = "pse_msd_accumulate";
    if (!m) return fail(PSE_ERR_INVALID, "%s: null displacement object", who);
    if (N == 0 || N > n_max) return fail(PSE_ERR_INVALID, "%s: N = %u outside (0, n_max = %u]", who, N, n_max);
    if (!pos) return fail(PSE_ERR_INVALID, "%s: null pos", who);
    if (!image) return fail(PSE_ERR_INVALID, "%s: null image", who);
    if (!std::isfinite(strain)) return fail(PSE_ERR_INVALID, "%s: strain = %g is not finite", who, strain);
    if (npairs < 1 || npairs > MSD_MAX_ORIGINS) return fail(PSE_ERR_INVALID, "%s: npairs = %d outside [1, %d]", who, npairs, MSD_MAX_ORIGINS);
    if (!slots) return fail(PSE_ERR_INVALID, "%s: null slots_host", who);
    if (!rows) return fail(PSE_ERR_INVALID, "%s: null rows_host", who);
    if (nrows < 1) return fail(PSE_ERR_INVALID, "%s: nrows = %d, need at least one row", who, nrows);
    for (int q = 0; q < npairs; ++q)
        if (slots[q] < 0 || slots[q] >= norigins)
            return fail(PSE_ERR_INVALID, "%s: pair %d names the slot %d outside [0, norigins = %d)", who, q, slots[q], norigins);
    for (int q = 0; q < npairs; ++q)
        if (!((stored >> slots[q]) & 1ull)) return fail(PSE_ERR_INVALID, "%s: pair %d names the slot %d, which was never stored", who, q, slots[q]);
    for (int q = 0; q < npairs; ++q)
        if (rows[q] < 0 || rows[q] >= nrows) return fail(PSE_ERR_INVALID, "%s: pair %d names the row %d outside [0, nrows = %d)", who, q, rows[q], nrows);
    for (int q = 0; q < npairs; ++q)
        for (int p = 0; p < q; ++p)
            if (rows[p] == rows[q]) return fail(PSE_ERR_INVALID, "%s: pairs %d and %d both name the row %d", who, p, q, rows[q]);
    if (!sums) return fail(PSE_ERR_INVALID, "%s: null sums", who);
    if (((uintptr_t)sums & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: sums = %p is not 8-byte aligned (doubles)", who, sums);
    return 0;
}

int isf_create_validate(unsigned n_max, unsigned n, const unsigned *types, int ntypes, unsigned nk, const int *modes, int norigins) {
    const char *who = "pse_isf_create";
    if (int rc = mode_list_validate(who, n_max, n, types, ntypes, nk, ISF_MAX_MODES, modes)) return rc;
    if (norigins < 1 || norigins > ISF_MAX_ORIGINS) return fail(PSE_ERR_INVALID, "%s: norigins = %d outside [1, %d]", who, norigins, ISF_MAX_ORIGINS);
    return 0;
}

int isf_sample_validate(const void *obj, unsigned n_max, unsigned N, const void *pos, const void *rho, const void *static_sums) {
    const char *who = "pse_isf_sample";
    if (!obj) return fail(PSE_ERR_INVALID, "%s: null scattering object", who);
    if (N == 0 || N > n_max) return fail(PSE_ERR_INVALID, "%s: N = %u outside (0, n_max = %u]", who, N, n_max);
    if (!pos) return fail(PSE_ERR_INVALID, "%s: null pos", who);
    if (((uintptr_t)rho & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: rho = %p is not 8-byte aligned (doubles)", who, rho);
    if (((uintptr_t)static_sums & 7u) != 0)
        return fail(PSE_ERR_INVALID, "%s: static_sums = %p is not 8-byte aligned (doubles)", who, static_sums);
    return 0;
}

int isf_store_validate(const void *obj, int norigins, unsigned sample_N, int slot) {
    const char *who = "pse_isf_store";
    if (!obj) return fail(PSE_ERR_INVALID, "%s: null scattering object", who);
    if (slot < 0 || slot >= norigins) return fail(PSE_ERR_INVALID, "%s: slot = %d outside [0, norigins = %d)", who, slot, norigins);
    if (!sample_N) return fail(PSE_ERR_INVALID, "%s: no pse_isf_sample since create: the current buffer holds nothing", who);
    return 0;
}

int isf_correlate_validate(const void *obj, int norigins, unsigned sample_N, const unsigned *slot_N, int npairs, const int *slots, const int *rows,
                           int nrows, const void *self, const void *coll) {
    const char *who = "pse_isf_correlate";
    if (!obj) return fail(PSE_ERR_INVALID, "%s: null scattering object", who);
    if (!sample_N) return fail(PSE_ERR_INVALID, "%s: no pse_isf_sample since create: the current buffer holds nothing", who);
    if (npairs < 1 || npairs > ISF_MAX_ORIGINS) return fail(PSE_ERR_INVALID, "%s: npairs = %d outside [1, %d]", who, npairs, ISF_MAX_ORIGINS);
    if (!slots) return fail(PSE_ERR_INVALID, "%s: null slots_host", who);
    if (!rows) return fail(PSE_ERR_INVALID, "%s: null rows_host", who);
    if (nrows < 1) return fail(PSE_ERR_INVALID, "%s: nrows = %d, need at least one row", who, nrows);
    for (int q = 0; q < npairs; ++q)
        if (slots[q] < 0 || slots[q] >= norigins)
            return fail(PSE_ERR_INVALID, "%s: pair %d names the slot %d outside [0, norigins = %d)", who, q, slots[q], norigins);
    for (int q = 0; q < npairs; ++q)
        if (!slot_N[slots[q]]) return fail(PSE_ERR_INVALID, "%s: pair %d names the slot %d, which was never stored", who, q, slots[q]);
    for (int q = 0; q < npairs; ++q)
        if (slot_N[slots[q]] != sample_N)
            return fail(PSE_ERR_INVALID, "%s: pair %d names the slot %d, stored with N = %u: the current sample has N = %u", who, q, slots[q],
                        slot_N[slots[q]], sample_N);
    for (int q = 0; q < npairs; ++q)
        if (rows[q] < 0 || rows[q] >= nrows) return fail(PSE_ERR_INVALID, "%s: pair %d names the row %d outside [0, nrows = %d)", who, q, rows[q], nrows);
    for (int q = 0; q < npairs; ++q)
        for (int p = 0; p < q; ++p)
            if (rows[p] == rows[q]) return fail(PSE_ERR_INVALID, "%s: pairs %d and %d both name the row %d", who, p, q, rows[q]);
    if (!self && !coll) return fail(PSE_ERR_INVALID, "%s: self and coll are both null: nothing to compute", who);
    if (((uintptr_t)self & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: self = %p is not 8-byte aligned (doubles)", who, self);
    if (((uintptr_t)coll & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: coll = %p is not 8-byte aligned (doubles)", who, coll);
    return 0;
}

int clusters_create_validate(double rcut, unsigned n_max, unsigned n, const unsigned *types, int ntypes, const double *rlink) {
    const char *who = "pse_clusters_create";
    if (int rc = sizes_in_range(who, n_max, n, ntypes)) return rc;
    if (!rlink) return fail(PSE_ERR_INVALID, "%s: null rlink_host", who);
    const int npt = ntypes * (ntypes + 1) / 2;
    bool on = false;
    for (int p = 0; p < npt; ++p) {
        if (!std::isfinite(rlink[p])) return fail(PSE_ERR_INVALID, "%s: pair type %d has rlink = %g, which is not finite", who, p, rlink[p]);
        if (rlink[p] < 0.0) return fail(PSE_ERR_INVALID, "%s: pair type %d has rlink = %g, which is negative (0 switches a pair type off)", who, p, rlink[p]);
        if (rlink[p] > rcut)
            return fail(PSE_ERR_INVALID, "%s: pair type %d has rlink = %.4f beyond rcut = %.4f: the cell list is built for the hydrodynamic cutoff", who,
                        p, rlink[p], rcut);
        on = on || rlink[p] > 0.0;
    }
    if (!on) return fail(PSE_ERR_INVALID, "%s: every pair type is off (rlink = 0): nothing could be linked", who);
    if (int rc = types_in_range(who, n, types, ntypes)) return rc;
    return 0;
}

int clusters_label_validate(const void *g, const void *g_handle, unsigned n_max, int n_slabs, unsigned known_status, unsigned N, const void *pos,
                            const void *label, const void *size, const void *stats, const void *hist, unsigned nhist, const void *ex,
                            const void *ex_handle) {
    const char *who = "pse_clusters_label";
    if (!g) return fail(PSE_ERR_INVALID, "%s: null cluster object", who);
    if (N == 0 || N > n_max) return fail(PSE_ERR_INVALID, "%s: N = %u outside (0, n_max = %u]", who, N, n_max);
    if (!pos) return fail(PSE_ERR_INVALID, "%s: null pos", who);
    if (!label && !size && !stats && !hist) return fail(PSE_ERR_INVALID, "%s: label, size, stats and hist are all null: nothing to write", who);
    if (((uintptr_t)stats & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: stats is not 8-byte aligned (64-bit words)", who);
    if (((uintptr_t)hist & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: hist is not 8-byte aligned (64-bit words)", who);
    if (hist && nhist == 0) return fail(PSE_ERR_INVALID, "%s: hist given with nhist = 0, need at least one word", who);
    if (ex) if (int rc = pair_excl_validate(who, ex, ex_handle, g_handle)) return rc;
    if (n_slabs > 1)
        return fail(PSE_ERR_INVALID, "%s: this handle is a slab rank (n_slabs = %d): it orders only its own cells, the clusters would be partial", who,
                    n_slabs);
    if (known_status)
        return fail(PSE_ERR_INVALID, "%s: an earlier call gave up (status word 0x%x, pse_clusters_status): its labels were not complete", who,
                    known_status);
    return 0;
}

int clusters_span_validate(const void *g, const void *g_handle, unsigned n_max, int n_slabs, unsigned known_status, unsigned N, const void *pos,
                           const void *label, const void *size, const void *stats, const void *hist, unsigned nhist, const void *span,
                           const void *image, const void *rg2, const void *pstats, const void *ex, const void *ex_handle) {
    const char *who = "pse_clusters_span";
    if (!g) return fail(PSE_ERR_INVALID, "%s: null cluster object", who);
    if (N == 0 || N > n_max) return fail(PSE_ERR_INVALID, "%s: N = %u outside (0, n_max = %u]", who, N, n_max);
    if (!pos) return fail(PSE_ERR_INVALID, "%s: null pos", who);
    if (!label && !size && !stats && !hist && !span && !image && !rg2 && !pstats)
        return fail(PSE_ERR_INVALID, "%s: label, size, stats, hist, span, image, rg2 and pstats are all null: nothing to write", who);
    if (((uintptr_t)stats & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: stats is not 8-byte aligned (64-bit words)", who);
    if (((uintptr_t)hist & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: hist is not 8-byte aligned (64-bit words)", who);
    if (hist && nhist == 0) return fail(PSE_ERR_INVALID, "%s: hist given with nhist = 0, need at least one word", who);
    if (ex) if (int rc = pair_excl_validate(who, ex, ex_handle, g_handle)) return rc;
    if (n_slabs > 1)
        return fail(PSE_ERR_INVALID, "%s: this handle is a slab rank (n_slabs = %d): it orders only its own cells, the clusters would be partial", who,
                    n_slabs);
    if (known_status)
        return fail(PSE_ERR_INVALID, "%s: an earlier call gave up (status word 0x%x, pse_clusters_status): its labels were not complete", who,
                    known_status);
    if (((uintptr_t)rg2 & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: rg2 is not 8-byte aligned (doubles)", who);
    if (((uintptr_t)pstats & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: pstats is not 8-byte aligned (64-bit words)", who);
    return 0;
}

int bond_order_create_validate(double rcut, unsigned n_max, unsigned n, const unsigned *types, int ntypes, const double *rnb, int nl,
                               const int *degrees) {
    const char *who = "pse_bond_order_create";
    if (int rc = sizes_in_range(who, n_max, n, ntypes)) return rc;
    if (!rnb) return fail(PSE_ERR_INVALID, "%s: null rnb_host", who);
    const int npt = ntypes * (ntypes + 1) / 2;
    bool on = false;
    for (int p = 0; p < npt; ++p) {
        if (!std::isfinite(rnb[p])) return fail(PSE_ERR_INVALID, "%s: pair type %d has rnb = %g, which is not finite", who, p, rnb[p]);
        if (rnb[p] < 0.0) return fail(PSE_ERR_INVALID, "%s: pair type %d has rnb = %g, which is negative (0 switches a pair type off)", who, p, rnb[p]);
        if (rnb[p] > rcut)
            return fail(PSE_ERR_INVALID, "%s: pair type %d has rnb = %.4f beyond rcut = %.4f: the cell list is built for the hydrodynamic cutoff", who,
                        p, rnb[p], rcut);
        on = on || rnb[p] > 0.0;
    }
    if (!on) return fail(PSE_ERR_INVALID, "%s: every pair type is off (rnb = 0): nobody would have a neighbour", who);
    if (int rc = types_in_range(who, n, types, ntypes)) return rc;
    if (nl < 1 || nl > BOND_ORDER_MAX_DEGREES) return fail(PSE_ERR_INVALID, "%s: nl = %d outside [1, %d]", who, nl, BOND_ORDER_MAX_DEGREES);
    if (!degrees) return fail(PSE_ERR_INVALID, "%s: null degrees_host", who);
    for (int d = 0; d < nl; ++d)
        if (degrees[d] < 2 || degrees[d] > BOND_ORDER_MAX_L || (degrees[d] & 1))
            return fail(PSE_ERR_INVALID, "%s: degree %d = %d is not one of the even degrees 2..%d", who, d, degrees[d], BOND_ORDER_MAX_L);
    for (int d = 0; d < nl; ++d)
        for (int e = 0; e < d; ++e)
            if (degrees[e] == degrees[d]) return fail(PSE_ERR_INVALID, "%s: the degree %d is listed twice (degrees %d and %d)", who, degrees[d], e, d);
    return 0;
}

int bond_order_compute_validate(const void *b, const void *b_handle, int nl, unsigned n_max, int n_slabs, unsigned N, const void *pos,
                                const void *nnb, const void *q, const void *qbar, int solid_degree, double threshold, const void *nconn,
                                const void *stats, const void *ex, const void *ex_handle) {
    const char *who = "pse_bond_order_compute";
    if (!b) return fail(PSE_ERR_INVALID, "%s: null bond-order object", who);
    if (N == 0 || N > n_max) return fail(PSE_ERR_INVALID, "%s: N = %u outside (0, n_max = %u]", who, N, n_max);
    if (!pos) return fail(PSE_ERR_INVALID, "%s: null pos", who);
    if (!nnb && !q && !qbar && !nconn && !stats) return fail(PSE_ERR_INVALID, "%s: nnb, q, qbar, nconn and stats are all null: nothing to write", who);
    if (solid_degree < -1 || solid_degree >= nl)
        return fail(PSE_ERR_INVALID, "%s: solid_degree = %d outside [-1, nl = %d): an index into the degrees, or -1", who, solid_degree, nl);
    if (solid_degree >= 0 && !(std::isfinite(threshold) && threshold >= -1.0 && threshold <= 1.0))
        return fail(PSE_ERR_INVALID, "%s: threshold = %g outside [-1, 1] (s_ij is a normalised scalar product)", who, threshold);
    if (((uintptr_t)stats & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: stats is not 8-byte aligned (64-bit words)", who);
    if (ex) if (int rc = pair_excl_validate(who, ex, ex_handle, b_handle)) return rc;
    if (n_slabs > 1)
        return fail(PSE_ERR_INVALID, "%s: this handle is a slab rank (n_slabs = %d): it orders only its own cells, the neighbours would be partial", who,
                    n_slabs);
    return 0;
}

int bond_order_histogram_validate(const void *b, int nl, int ntypes, unsigned n_max, const void *values, int column, unsigned N, int nbins,
                                  double lo, double hi, const void *counts) {
    const char *who = "pse_bond_order_histogram";
    if (!b) return fail(PSE_ERR_INVALID, "%s: null bond-order object", who);
    if (N == 0 || N > n_max) return fail(PSE_ERR_INVALID, "%s: N = %u outside (0, n_max = %u]", who, N, n_max);
    if (!values) return fail(PSE_ERR_INVALID, "%s: null values", who);
    if (column < 0 || column >= nl) return fail(PSE_ERR_INVALID, "%s: column = %d outside [0, nl = %d)", who, column, nl);
    if (nbins < 1) return fail(PSE_ERR_INVALID, "%s: nbins = %d, need at least one bin", who, nbins);
    if ((long long)ntypes * nbins > BOND_ORDER_MAX_COUNTERS)
        return fail(PSE_ERR_INVALID, "%s: %d types x %d bins = %lld counters, more than %d (the counters are kept in 32 KB of LDS)", who, ntypes, nbins,
                    (long long)ntypes * nbins, BOND_ORDER_MAX_COUNTERS);
    if (!std::isfinite(lo) || !std::isfinite(hi)) return fail(PSE_ERR_INVALID, "%s: lo = %g, hi = %g must be finite", who, lo, hi);
    if (!(hi > lo)) return fail(PSE_ERR_INVALID, "%s: hi = %g must exceed lo = %g", who, hi, lo);
    if (!counts) return fail(PSE_ERR_INVALID, "%s: null counts", who);
    if (((uintptr_t)counts & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: counts is not 8-byte aligned (64-bit counters)", who);
    return 0;
}

void structure_factor_plan(unsigned nk, const int *modes, std::vector<unsigned> &perm, std::vector<unsigned> &uoff, std::vector<int> &segs) {
    perm.resize(nk);
    for (unsigned q = 0; q < nk; ++q) perm[q] = q;
    auto differ = [&](unsigned a, unsigned b) {
        for (int c = 0; c < 3; ++c)
            if (modes[3 * (size_t)a + c] != modes[3 * (size_t)b + c]) return true;
        return false;
    };
    std::sort(perm.begin(), perm.end(), [&](unsigned a, unsigned b) {
        for (int c = 0; c < 3; ++c)
            if (modes[3 * (size_t)a + c] != modes[3 * (size_t)b + c]) return modes[3 * (size_t)a + c] < modes[3 * (size_t)b + c];
        return a < b;
    });
    uoff.clear();
    for (unsigned e = 0; e < nk; ++e)
        if (e == 0 || differ(perm[e - 1], perm[e])) uoff.push_back(e);
    const unsigned nu = (unsigned)uoff.size();
    uoff.push_back(nk);
    auto m = [&](unsigned u, int c) { return modes[3 * (size_t)perm[uoff[u]] + c]; };
    segs.clear();
    for (unsigned q = 0; q < nu;) {
        int d[3] = {0, 0, 0};
        unsigned len = 1;
        auto zero = [&](unsigned u) { return m(u, 0) == 0 && m(u, 1) == 0 && m(u, 2) == 0; };   // (0, 0, 0) is always a seed: rho = N_a exactly
        if (q + 1 < nu && !zero(q + 1)) {
            for (int c = 0; c < 3; ++c) d[c] = m(q + 1, c) - m(q, c);
            len = 2;
            while (len < (unsigned)SF_RUN && q + len < nu && !zero(q + len) && m(q + len, 0) - m(q + len - 1, 0) == d[0] &&
                   m(q + len, 1) - m(q + len - 1, 1) == d[1] && m(q + len, 2) - m(q + len - 1, 2) == d[2])
                ++len;
        }
        const int sg[8] = {m(q, 0), m(q, 1), m(q, 2), (int)len, d[0], d[1], d[2], (int)q};
        segs.insert(segs.end(), sg, sg + 8);
        q += len;
    }
    // the segments of more than SF_SHORT modes first, the short ones behind them, each class in the canonical order: the pass runs
    // the classes as two launches (a scattered list is all pairs and single modes: seven of eight recurrence steps would be wasted)
    std::vector<int> sorted;
    sorted.reserve(segs.size());
    for (int pass = 0; pass < 2; ++pass)
        for (size_t g = 0; g < segs.size(); g += 8)
            if ((segs[g + 3] > SF_SHORT) == (pass == 0)) sorted.insert(sorted.end(), segs.begin() + g, segs.begin() + g + 8);
    segs.swap(sorted);
}

// The layout of pse_host_molecule_rows (include/pse_amd.h), under the name `who` of the entry point that asks.  Adjacency rows by a
// counting sort, each sorted ascending; one breadth-first walk per component from its smallest member; the tiles by a greedy packing.
int molecule_layout(const char *who, unsigned n, unsigned nbonds, const unsigned *pairs, MoleculeLayout &L) {
    if (!pairs) return fail(PSE_ERR_INVALID, "%s: null pairs", who);
    if (n == 0) return fail(PSE_ERR_INVALID, "%s: n = 0", who);
    if (nbonds == 0) return fail(PSE_ERR_INVALID, "%s: nbonds = 0: there is no molecule at all", who);
    if (nbonds > (1u << 30)) return fail(PSE_ERR_INVALID, "%s: nbonds = %u outside (0, 2^30]", who, nbonds);
    std::vector<uint64_t> key(nbonds);
    for (unsigned b = 0; b < nbonds; ++b) {
        const unsigned i = pairs[2 * (size_t)b], j = pairs[2 * (size_t)b + 1];
        if (i >= n || j >= n) return fail(PSE_ERR_INVALID, "%s: bond %u = (%u, %u) has an endpoint >= n = %u", who, b, i, j, n);
        if (i == j) return fail(PSE_ERR_INVALID, "%s: bond %u joins particle %u to itself", who, b, i);
        key[b] = ((uint64_t)std::min(i, j) << 32) | std::max(i, j);
    }
    std::sort(key.begin(), key.end());
    for (unsigned b = 1; b < nbonds; ++b)
        if (key[b] == key[b - 1])
            return fail(PSE_ERR_INVALID, "%s: the bond (%u, %u) is listed twice", who, (unsigned)(key[b] >> 32), (unsigned)key[b]);
    // (the keys are sorted by (min, max): walked in that order every row comes out ascending, as in pse_host_exclusion_rows)
    std::vector<unsigned> off((size_t)n + 1, 0u), adj(2 * (size_t)nbonds);
    for (uint64_t k : key) { ++off[(unsigned)(k >> 32) + 1]; ++off[(unsigned)k + 1]; }
    for (unsigned i = 0; i < n; ++i) off[i + 1] += off[i];
    {
        std::vector<unsigned> fill(off.begin(), off.begin() + n);
        for (uint64_t k : key) {
            const unsigned lo = (unsigned)(k >> 32), hi = (unsigned)k;
            adj[fill[lo]++] = hi;
            adj[fill[hi]++] = lo;
        }
    }
    L = MoleculeLayout();
    L.mol_of.assign(n, -1);
    L.mol_off.push_back(0u);
    std::vector<unsigned> slot_of(n, 0u), maxdepth;
    for (unsigned root = 0; root < n; ++root) {
        if (L.mol_of[root] >= 0 || off[root + 1] == off[root]) continue;
        const int mol = (int)L.nring.size();
        const unsigned first = (unsigned)L.members.size();
        L.mol_of[root] = mol;
        slot_of[root] = first;
        L.members.push_back(root); L.parent.push_back(0u); L.depth.push_back(0u);
        size_t degsum = 0;
        unsigned ones = 0, twos = 0, end_lo = 0u, end_hi = 0u, deepest = 0u;
        for (unsigned q = first; q < L.members.size(); ++q) {   // (the queue is the member list itself)
            const unsigned i = L.members[q], deg = off[i + 1] - off[i];
            degsum += deg;
            if (deg == 1) { (ones == 0 ? end_lo : end_hi) = q; ++ones; }   // (of a linear molecule: its two ends)
            twos += deg == 2;
            for (unsigned e = off[i]; e < off[i + 1]; ++e) {
                const unsigned j = adj[e];
                if (L.mol_of[j] >= 0) continue;
                L.mol_of[j] = mol;
                slot_of[j] = (unsigned)L.members.size();
                L.members.push_back(j); L.parent.push_back(q - first); L.depth.push_back(L.depth[q] + 1u);
                deepest = std::max(deepest, L.depth[q] + 1u);
            }
        }
        const unsigned m = (unsigned)L.members.size() - first;
        if (m > (unsigned)PSE_MOL_TILE)
            return fail(PSE_ERR_INVALID, "%s: the molecule of particle %u has %u members, more than PSE_MOL_TILE = %d", who, root, m, PSE_MOL_TILE);
        const unsigned rings = (unsigned)(degsum / 2) - (m - 1u);
        const bool linear = rings == 0u && ones == 2u && twos == m - 2u;
        if (linear && L.members[end_lo] > L.members[end_hi]) std::swap(end_lo, end_hi);   // lower caller index first
        L.nring.push_back(rings);
        L.ends.push_back(linear ? end_lo - first : 0xffffffffu);
        L.ends.push_back(linear ? end_hi - first : 0xffffffffu);
        L.mol_off.push_back((unsigned)L.members.size());
        maxdepth.push_back(deepest);
    }
    L.nmol = (unsigned)L.nring.size();
    L.tile_mol.push_back(0u);
    unsigned fill = 0u, deepest = 0u;
    auto rounds_of = [](unsigned d) { unsigned r = 0; while ((1u << r) < d + 1u) ++r; return r; };
    for (unsigned mol = 0; mol < L.nmol; ++mol) {
        const unsigned m = L.mol_off[mol + 1] - L.mol_off[mol];
        if (fill + m > (unsigned)PSE_MOL_TILE) {
            L.tile_mol.push_back(mol);
            L.tile_rounds.push_back(rounds_of(deepest));
            fill = 0u; deepest = 0u;
        }
        fill += m;
        deepest = std::max(deepest, maxdepth[mol]);
    }
    L.tile_mol.push_back(L.nmol);
    L.tile_rounds.push_back(rounds_of(deepest));
    L.ntiles = (unsigned)L.tile_rounds.size();
    return 0;
}

int molecule_topology_validate(const char *who, unsigned n_max, unsigned n, unsigned nbonds, const unsigned *pairs, const unsigned *mol_types,
                               int ntypes, MoleculeLayout &L) {
    if (n == 0 || n > n_max) return fail(PSE_ERR_INVALID, "%s: n = %u outside (0, n_max = %u]", who, n, n_max);
    if (nbonds == 0) return fail(PSE_ERR_INVALID, "%s: nbonds = 0: there is no molecule at all", who);
    if (!pairs) return fail(PSE_ERR_INVALID, "%s: null pairs_host", who);
    if (int rc = molecule_layout(who, n, nbonds, pairs, L)) return rc;
    if (ntypes < 1 || ntypes > PAIR_TYPED_MAX_TYPES) return fail(PSE_ERR_INVALID, "%s: ntypes = %d outside [1, %d]", who, ntypes, PAIR_TYPED_MAX_TYPES);
    if (mol_types)
        for (unsigned mol = 0; mol < L.nmol; ++mol)
            if (mol_types[mol] >= (unsigned)ntypes)
                return fail(PSE_ERR_INVALID, "%s: molecule %u has type %u >= ntypes = %d", who, mol, mol_types[mol], ntypes);
    return 0;
}

int molecules_create_validate(unsigned n_max, unsigned n, unsigned nbonds, const unsigned *pairs, const unsigned *mol_types, int ntypes, int nbins,
                              double rg_max, double ree_max, MoleculeLayout &L) {
    const char *who = "pse_molecules_create";
    if (int rc = molecule_topology_validate(who, n_max, n, nbonds, pairs, mol_types, ntypes, L)) return rc;
    if (nbins < 0 || nbins > MOL_MAX_BINS) return fail(PSE_ERR_INVALID, "%s: nbins = %d outside [0, %d]", who, nbins, MOL_MAX_BINS);
    if (nbins > 0 && !(std::isfinite(rg_max) && rg_max > 0.0)) return fail(PSE_ERR_INVALID, "%s: rg_max = %g must be finite and positive", who, rg_max);
    if (nbins > 0 && !(std::isfinite(ree_max) && ree_max > 0.0)) return fail(PSE_ERR_INVALID, "%s: ree_max = %g must be finite and positive", who, ree_max);
    return 0;
}

int molecules_compute_validate(const void *m, int nbins, const void *pos, const void *rows, const void *unfolded, const void *sums,
                               const void *sample, const void *hist) {
    const char *who = "pse_molecules_compute";
    if (!m) return fail(PSE_ERR_INVALID, "%s: null molecule object", who);
    if (!pos) return fail(PSE_ERR_INVALID, "%s: null pos", who);
    if (!rows && !unfolded && !sums && !sample && !hist)
        return fail(PSE_ERR_INVALID, "%s: rows, unfolded, sums, sample and hist are all null: nothing to compute", who);
    if (((uintptr_t)rows & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: rows = %p is not 8-byte aligned (doubles)", who, rows);
    if (((uintptr_t)unfolded & 15u) != 0) return fail(PSE_ERR_INVALID, "%s: unfolded = %p is not 16-byte aligned (rows of four doubles)", who, unfolded);
    if (((uintptr_t)sums & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: sums = %p is not 8-byte aligned (doubles)", who, sums);
    if (((uintptr_t)sample & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: sample = %p is not 8-byte aligned (doubles)", who, sample);
    if (((uintptr_t)hist & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: hist = %p is not 8-byte aligned (64-bit counters)", who, hist);
    if (hist && nbins == 0) return fail(PSE_ERR_INVALID, "%s: hist given, but the object was created with nbins = 0: it has no histogram", who);
    return 0;
}

int molecules_count_validate(const void *m, const void *nmol, const void *nlinear, const void *nmol_type) {
    const char *who = "pse_molecules_count";
    if (!m) return fail(PSE_ERR_INVALID, "%s: null molecule object", who);
    if (!nmol && !nlinear && !nmol_type) return fail(PSE_ERR_INVALID, "%s: nmol, nlinear and nmol_type are all null: nothing to write", who);
    return 0;
}

void molecules_counts(const MoleculeLayout &L, const unsigned *mol_types, int ntypes, unsigned *nmol, unsigned *nlinear, unsigned *nmol_type) {
    if (nmol) *nmol = L.nmol;
    if (nlinear) std::fill(nlinear, nlinear + ntypes, 0u);
    if (nmol_type) std::fill(nmol_type, nmol_type + ntypes, 0u);
    for (unsigned mol = 0; mol < L.nmol; ++mol) {
        const unsigned a = mol_types ? mol_types[mol] : 0u;
        if (nmol_type) ++nmol_type[a];
        if (nlinear && L.ends[2 * (size_t)mol] != 0xffffffffu) ++nlinear[a];
    }
}

// The rank of every member slot (pse_host_chain_order, include/pse_amd.h) from the spanning tree alone: in a linear molecule the walk
// from the lower end up to the root counts 0, 1, ..., the walk from the higher end up to the root counts m - 1, m - 2, ...
static void chain_ranks(unsigned nmol, const unsigned *parent, const unsigned *mol_off, const unsigned *ends, unsigned *rank) {
    for (unsigned mol = 0; mol < nmol; ++mol) {
        const unsigned o = mol_off[mol], m = mol_off[mol + 1] - o, lo = ends[2 * (size_t)mol], hi = ends[2 * (size_t)mol + 1];
        for (unsigned p = 0; p < m; ++p) rank[o + p] = p;
        if (lo == 0xffffffffu) continue;
        unsigned r = 0u;
        for (unsigned p = lo; ; p = parent[o + p]) { rank[o + p] = r++; if (p == 0u) break; }
        r = m;
        for (unsigned p = hi; p != 0u; p = parent[o + p]) rank[o + p] = --r;
    }
}
void chain_order(const MoleculeLayout &L, std::vector<unsigned> &rank) {
    rank.resize(L.members.size());
    chain_ranks(L.nmol, L.parent.data(), L.mol_off.data(), L.ends.data(), rank.data());
}

int molecule_pairs_create_validate(unsigned n_max, unsigned n, unsigned nbonds, const unsigned *pairs, const unsigned *mol_types, int ntypes, int ns,
                                   MoleculeLayout &L) {
    const char *who = "pse_molecule_pairs_create";
    if (int rc = molecule_topology_validate(who, n_max, n, nbonds, pairs, mol_types, ntypes, L)) return rc;
    if (ns < 1 || ns > PSE_MOL_TILE) return fail(PSE_ERR_INVALID, "%s: ns = %d outside [1, %d]", who, ns, PSE_MOL_TILE);
    return 0;
}

int molecule_pairs_compute_validate(const void *p, const void *pos, const void *inv_rh, const void *curves, const void *sums, const void *sample) {
    const char *who = "pse_molecule_pairs_compute";
    if (!p) return fail(PSE_ERR_INVALID, "%s: null molecule-pair object", who);
    if (!pos) return fail(PSE_ERR_INVALID, "%s: null pos", who);
    if (!inv_rh && !curves && !sums && !sample)
        return fail(PSE_ERR_INVALID, "%s: inv_rh, curves, sums and sample are all null: nothing to compute", who);
    if (((uintptr_t)inv_rh & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: inv_rh = %p is not 8-byte aligned (doubles)", who, inv_rh);
    if (((uintptr_t)curves & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: curves = %p is not 8-byte aligned (doubles)", who, curves);
    if (((uintptr_t)sums & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: sums = %p is not 8-byte aligned (doubles)", who, sums);
    if (((uintptr_t)sample & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: sample = %p is not 8-byte aligned (doubles)", who, sample);
    return 0;
}

int molecule_pairs_counts_validate(const void *p, const void *nmol, const void *nmol_type, const void *terms) {
    const char *who = "pse_molecule_pairs_counts";
    if (!p) return fail(PSE_ERR_INVALID, "%s: null molecule-pair object", who);
    if (!nmol && !nmol_type && !terms) return fail(PSE_ERR_INVALID, "%s: nmol, nmol_type and terms are all null: nothing to write", who);
    return 0;
}

void molecule_pairs_terms(const MoleculeLayout &L, const unsigned *mol_types, int ntypes, int ns, unsigned long long *terms) {
    std::fill(terms, terms + (size_t)ntypes * ns * MOLPAIR_COLS, 0ull);
    for (unsigned mol = 0; mol < L.nmol; ++mol) {
        if (L.ends[2 * (size_t)mol] == 0xffffffffu) continue;
        const unsigned a = mol_types ? mol_types[mol] : 0u, m = L.mol_off[mol + 1] - L.mol_off[mol];
        for (unsigned s = 0; s < (unsigned)ns && s < m; ++s) {
            unsigned long long *e = terms + ((size_t)a * ns + s) * MOLPAIR_COLS;
            e[0] += m - s;
            e[1] += m - 1u - s;
        }
    }
}

void chain_modes_linear(const MoleculeLayout &L, const unsigned *mol_types, int ntypes, std::vector<unsigned> &lin_mol,
                        std::vector<unsigned> &lin_size, std::vector<unsigned> &nlin_type) {
    lin_mol.clear(); lin_size.clear();
    nlin_type.assign((size_t)ntypes, 0u);
    for (unsigned mol = 0; mol < L.nmol; ++mol) {
        if (L.ends[2 * (size_t)mol] == 0xffffffffu) continue;
        lin_mol.push_back(mol);
        lin_size.push_back(L.mol_off[mol + 1] - L.mol_off[mol]);
        ++nlin_type[mol_types ? mol_types[mol] : 0u];
    }
}

int chain_modes_create_validate(unsigned n_max, unsigned n, unsigned nbonds, const unsigned *pairs, const unsigned *mol_types, int ntypes,
                                int nmodes, int nsizes, const unsigned *sizes, const double *weights, int norigins, MoleculeLayout &L) {
    const char *who = "pse_chain_modes_create";
    if (int rc = molecule_topology_validate(who, n_max, n, nbonds, pairs, mol_types, ntypes, L)) return rc;
    if (nmodes < 1 || nmodes > CHAIN_MODES_MAX) return fail(PSE_ERR_INVALID, "%s: nmodes = %d outside [1, %d]", who, nmodes, CHAIN_MODES_MAX);
    if (norigins < 0 || norigins > MSD_MAX_ORIGINS) return fail(PSE_ERR_INVALID, "%s: norigins = %d outside [0, %d]", who, norigins, MSD_MAX_ORIGINS);
    std::vector<unsigned> present;   // the distinct sizes of the linear molecules, ascending
    for (unsigned mol = 0; mol < L.nmol; ++mol)
        if (L.ends[2 * (size_t)mol] != 0xffffffffu) present.push_back(L.mol_off[mol + 1] - L.mol_off[mol]);
    if (present.empty()) return fail(PSE_ERR_INVALID, "%s: none of the %u molecules is linear: there is no chain to project", who, L.nmol);
    std::sort(present.begin(), present.end());
    present.erase(std::unique(present.begin(), present.end()), present.end());
    if (nsizes < 1) return fail(PSE_ERR_INVALID, "%s: nsizes = %d, need at least one size", who, nsizes);
    if (!sizes) return fail(PSE_ERR_INVALID, "%s: null sizes_host", who);
    if (!weights) return fail(PSE_ERR_INVALID, "%s: null weights_host", who);
    for (int s = 0; s < nsizes || s < (int)present.size(); ++s) {
        if (s >= nsizes)
            return fail(PSE_ERR_INVALID, "%s: sizes_host has %d entries, the linear molecules %zu sizes: %u is missing", who, nsizes, present.size(),
                        present[s]);
        if (s >= (int)present.size() || sizes[s] != present[s])
            return fail(PSE_ERR_INVALID, "%s: sizes_host[%d] = %u is not the %d-th size of the linear molecules in ascending order", who, s, sizes[s], s);
    }
    size_t at = 0;
    for (int s = 0; s < nsizes; ++s)
        for (int k = 0; k < nmodes; ++k)
            for (unsigned q = 0; q < sizes[s]; ++q, ++at)
                if (!std::isfinite(weights[at]))
                    return fail(PSE_ERR_INVALID, "%s: the weight of size %u, row %d, rank %u is %g, which is not finite", who, sizes[s], k, q, weights[at]);
    return 0;
}

int chain_modes_counts_validate(const void *obj, const void *nmol, const void *nlin, const void *nlin_type, const void *lin_mol,
                                const void *lin_size) {
    const char *who = "pse_chain_modes_counts";
    if (!obj) return fail(PSE_ERR_INVALID, "%s: null chain-modes object", who);
    if (!nmol && !nlin && !nlin_type && !lin_mol && !lin_size)
        return fail(PSE_ERR_INVALID, "%s: nmol, nlin, nlin_type, lin_mol and lin_size are all null: nothing to write", who);
    return 0;
}

int chain_modes_compute_validate(const void *obj, const void *pos, const void *modes, const void *sums, const void *sample) {
    const char *who = "pse_chain_modes_compute";
    if (!obj) return fail(PSE_ERR_INVALID, "%s: null chain-modes object", who);
    if (!pos) return fail(PSE_ERR_INVALID, "%s: null pos", who);
    if (((uintptr_t)modes & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: modes = %p is not 8-byte aligned (doubles)", who, modes);
    if (((uintptr_t)sums & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: sums = %p is not 8-byte aligned (doubles)", who, sums);
    if (((uintptr_t)sample & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: sample = %p is not 8-byte aligned (doubles)", who, sample);
    return 0;
}

int chain_modes_store_validate(const void *obj, int norigins, bool computed, int slot) {
    const char *who = "pse_chain_modes_store";
    if (!obj) return fail(PSE_ERR_INVALID, "%s: null chain-modes object", who);
    if (norigins == 0) return fail(PSE_ERR_INVALID, "%s: the object was created with norigins = 0: it has no origin slots", who);
    if (slot < 0 || slot >= norigins) return fail(PSE_ERR_INVALID, "%s: slot = %d outside [0, norigins = %d)", who, slot, norigins);
    if (!computed) return fail(PSE_ERR_INVALID, "%s: no pse_chain_modes_compute since create: the current buffer holds nothing", who);
    return 0;
}

int chain_modes_correlate_validate(const void *obj, int norigins, bool computed, unsigned long long stored, int npairs, const int *slots,
                                   const int *rows, int nrows, const void *corr) {
    const char *who = "pse_chain_modes_correlate";
    if (!obj) return fail(PSE_ERR_INVALID, "%s: null chain-modes object", who);
    if (norigins == 0) return fail(PSE_ERR_INVALID, "%s: the object was created with norigins = 0: it has no origin slots", who);
    if (!computed) return fail(PSE_ERR_INVALID, "%s: no pse_chain_modes_compute since create: the current buffer holds nothing", who);
    if (npairs < 1 || npairs > MSD_MAX_ORIGINS) return fail(PSE_ERR_INVALID, "%s: npairs = %d outside [1, %d]", who, npairs, MSD_MAX_ORIGINS);
    if (!slots) return fail(PSE_ERR_INVALID, "%s: null slots_host", who);
    if (!rows) return fail(PSE_ERR_INVALID, "%s: null rows_host", who);
    if (nrows < 1) return fail(PSE_ERR_INVALID, "%s: nrows = %d, need at least one row", who, nrows);
    for (int q = 0; q < npairs; ++q)
        if (slots[q] < 0 || slots[q] >= norigins)
            return fail(PSE_ERR_INVALID, "%s: pair %d names the slot %d outside [0, norigins = %d)", who, q, slots[q], norigins);
    for (int q = 0; q < npairs; ++q)
        if (!((stored >> slots[q]) & 1ull)) return fail(PSE_ERR_INVALID, "%s: pair %d names the slot %d, which was never stored", who, q, slots[q]);
    for (int q = 0; q < npairs; ++q)
        if (rows[q] < 0 || rows[q] >= nrows) return fail(PSE_ERR_INVALID, "%s: pair %d names the row %d outside [0, nrows = %d)", who, q, rows[q], nrows);
    for (int q = 0; q < npairs; ++q)
        for (int p = 0; p < q; ++p)
            if (rows[p] == rows[q]) return fail(PSE_ERR_INVALID, "%s: pairs %d and %d both name the row %d", who, p, q, rows[q]);
    if (!corr) return fail(PSE_ERR_INVALID, "%s: null corr", who);
    if (((uintptr_t)corr & 7u) != 0) return fail(PSE_ERR_INVALID, "%s: corr = %p is not 8-byte aligned (doubles)", who, corr);
    return 0;
}

}  // namespace pse

using namespace pse;

extern "C" const char *pse_last_error(void) { return error_text().c_str(); }

extern "C" int pse_host_select_params(const pse_params *p, pse_info *info) {
    if (!p || !info) return fail(PSE_ERR_INVALID, "null argument");
    Derived d;
    std::string e = select_params(Box{p->Lx, p->Ly, p->Lz, p->xy}, p->xi, p->error, p->max_strain, p->Nx, p->Ny, p->Nz,
                                  p->P, p->rcut, d);
    if (!e.empty()) return fail(PSE_ERR_INVALID, "%s", e.c_str());
    if (int rc = gaussian_fits(d, d.hx, d.hy, d.hz)) return rc;
    fill_info(d, info);
    return 0;
}

extern "C" int pse_host_realspace_table(double xi, double rcut, int cap, double *coef, int *n_intervals) {
    const char *who = "pse_host_realspace_table";
    if (!n_intervals) return fail(PSE_ERR_INVALID, "%s: null n_intervals", who);
    if (!(xi > 0.0) || !std::isfinite(xi)) return fail(PSE_ERR_INVALID, "%s: xi = %g must be positive", who, xi);
    if (!(rcut > 0.0) || !(rcut * RS_PER_UNIT < 1e6)) return fail(PSE_ERR_INVALID, "%s: rcut = %g outside (0, %g)", who, rcut, 1e6 / RS_PER_UNIT);
    *n_intervals = realspace_table_intervals(rcut);
    if (!coef) return fail(PSE_ERR_INVALID, "%s: null coef", who);
    if (cap < *n_intervals * 2 * RS_NCOEF)
        return fail(PSE_ERR_INVALID, "%s: cap = %d doubles, the table of rcut = %g has %d intervals of %d", who, cap, rcut, *n_intervals, 2 * RS_NCOEF);
    std::vector<double> c;
    int n = 0;
    build_realspace_table(xi, rcut, c, n);
    std::copy(c.begin(), c.end(), coef);
    return 0;
}

extern "C" int pse_host_lanczos_sqrt_e1(int m, const double *alpha, const double *beta, double *t) {
    if (m < 1 || m > 4096 || !alpha || !beta || !t) return fail(PSE_ERR_INVALID, "bad argument");
    std::vector<double> tv;
    if (!lanczos_sqrt_e1(m, alpha, beta, tv)) return fail(PSE_ERR_NUMERIC, "tridiagonal eigen-solve did not converge");
    std::copy(tv.begin(), tv.end(), t);
    return 0;
}

extern "C" int pse_host_lz_decide(const double *scal_host, int n_dec, const pse_debug_lz_decision *dec, double open0, pse_debug_lz_outcome *out) {
    if (int rc = lz_decisions_validate("pse_host_lz_decide", scal_host, n_dec, dec, out)) return rc;
    LzState st;
    memset(&st, 0xff, sizeof st);   // NaN bytes: only the reset under `first` makes the state valid
    double mirror[5] = {0.0, 0.0, 0.0, 0.0, open0};   // m, step norm, status, seq, open calls: what the device's decision leaves the host
    for (int k = 0; k < n_dec; ++k) {
        const bool was_done = !dec[k].first && st.done;
        int at = 0;
        (void)lz_decide_host(lz_decision(dec[k]), scal_host, st, &at);   // (a failure is status 2 in the state: what the caller asked to see)
        if (st.done && !was_done) {
            mirror[0] = (double)st.m_final; mirror[1] = st.stepnorm; mirror[2] = (double)st.status; mirror[3] = dec[k].seq;
            if (st.status != 0) mirror[4] += 1.0;
        }
        lz_outcome(st, &out[k]);
        std::copy(mirror, mirror + 5, out[k].mirror);
    }
    return 0;
}

// Counting sort of the 2 nbonds bond ends by particle, then each row sorted by (partner, type): O(nbonds) plus the row sorts.
extern "C" int pse_host_cluster_word(unsigned parent, const int *c, unsigned long long *word) {
    const char *who = "pse_host_cluster_word";
    if (!c || !word) return fail(PSE_ERR_INVALID, "%s: null %s", who, !c ? "c" : "word");
    if (parent >= CLUSTER_WORD_MAX_ROWS) return fail(PSE_ERR_INVALID, "%s: parent = %u outside [0, 2^28)", who, parent);
    if (!cluster_offset_fits(c[0], c[1], c[2]))
        return fail(PSE_ERR_INVALID, "%s: offset (%d, %d, %d) has a component outside [-%d, %d]", who, c[0], c[1], c[2], CLUSTER_WORD_MAX_OFFSET,
                    CLUSTER_WORD_MAX_OFFSET);
    *word = cluster_word_pack(parent, c[0], c[1], c[2]);
    return 0;
}
extern "C" int pse_host_cluster_word_parts(unsigned long long word, unsigned *parent, int *c) {
    const char *who = "pse_host_cluster_word_parts";
    if (!parent || !c) return fail(PSE_ERR_INVALID, "%s: null %s", who, !parent ? "parent" : "c");
    cluster_word_unpack(word, *parent, c[0], c[1], c[2]);
    return 0;
}

extern "C" int pse_host_bond_rows(unsigned n, unsigned nbonds, const unsigned *pairs, const unsigned *types, int *row_off, unsigned *entries) {
    if (!pairs || !row_off || !entries) return fail(PSE_ERR_INVALID, "pse_host_bond_rows: null array");
    if (n == 0) return fail(PSE_ERR_INVALID, "pse_host_bond_rows: n = 0");
    if (nbonds == 0 || nbonds > (1u << 30)) return fail(PSE_ERR_INVALID, "pse_host_bond_rows: nbonds = %u outside (0, 2^30]", nbonds);
    for (unsigned b = 0; b < nbonds; ++b) {
        const unsigned i = pairs[2 * (size_t)b], j = pairs[2 * (size_t)b + 1];
        if (i >= n || j >= n) return fail(PSE_ERR_INVALID, "pse_host_bond_rows: bond %u = (%u, %u) has an endpoint >= n = %u", b, i, j, n);
        if (i == j) return fail(PSE_ERR_INVALID, "pse_host_bond_rows: bond %u joins particle %u to itself", b, i);
    }
    // (offsets are counted as unsigned: at the cap of 2^30 bonds the last one is 2^31, which the device reads as unsigned too)
    unsigned *off = reinterpret_cast<unsigned *>(row_off);
    std::fill(off, off + (size_t)n + 1, 0u);
    for (unsigned b = 0; b < nbonds; ++b) { ++off[pairs[2 * (size_t)b] + 1]; ++off[pairs[2 * (size_t)b + 1] + 1]; }
    for (unsigned i = 0; i < n; ++i) off[i + 1] += off[i];
    std::vector<unsigned> fill(off, off + n);
    struct End { unsigned partner, type; };
    End *e = reinterpret_cast<End *>(entries);
    for (unsigned b = 0; b < nbonds; ++b) {
        const unsigned i = pairs[2 * (size_t)b], j = pairs[2 * (size_t)b + 1], t = types ? types[b] : 0u;
        e[fill[i]++] = End{j, t};
        e[fill[j]++] = End{i, t};
    }
    for (unsigned i = 0; i < n; ++i)
        std::sort(e + off[i], e + off[i + 1], [](const End &a, const End &b) { return a.partner != b.partner ? a.partner < b.partner : a.type < b.type; });
    return 0;
}

// Counting sort of the 3 nangles memberships by particle, then each row sorted by the canonical (i, j, k, type), i < k.
extern "C" int pse_host_angle_rows(unsigned n, unsigned nangles, const unsigned *triples, const unsigned *types, int *row_off, unsigned *entries) {
    if (!triples || !row_off || !entries) return fail(PSE_ERR_INVALID, "pse_host_angle_rows: null array");
    if (n == 0) return fail(PSE_ERR_INVALID, "pse_host_angle_rows: n = 0");
    if (nangles == 0 || nangles > (1u << 28)) return fail(PSE_ERR_INVALID, "pse_host_angle_rows: nangles = %u outside (0, 2^28]", nangles);
    for (unsigned a = 0; a < nangles; ++a) {
        const unsigned i = triples[3 * (size_t)a], j = triples[3 * (size_t)a + 1], k = triples[3 * (size_t)a + 2];
        if (i >= n || j >= n || k >= n)
            return fail(PSE_ERR_INVALID, "pse_host_angle_rows: angle %u = (%u, %u, %u) has an index >= n = %u", a, i, j, k, n);
        if (i == j || j == k || i == k)
            return fail(PSE_ERR_INVALID, "pse_host_angle_rows: angle %u = (%u, %u, %u) has two equal members", a, i, j, k);
    }
    std::fill(row_off, row_off + (size_t)n + 1, 0);   // (3 nangles <= 3 * 2^28 < 2^31)
    for (size_t m = 0; m < 3 * (size_t)nangles; ++m) ++row_off[triples[m] + 1];
    for (unsigned p = 0; p < n; ++p) row_off[p + 1] += row_off[p];
    std::vector<int> fill(row_off, row_off + n);
    struct Entry { unsigned i, j, k, type; };
    Entry *e = reinterpret_cast<Entry *>(entries);
    for (unsigned a = 0; a < nangles; ++a) {
        const unsigned x = triples[3 * (size_t)a], j = triples[3 * (size_t)a + 1], y = triples[3 * (size_t)a + 2];
        const Entry en{std::min(x, y), j, std::max(x, y), types ? types[a] : 0u};
        e[fill[en.i]++] = en;
        e[fill[en.j]++] = en;
        e[fill[en.k]++] = en;
    }
    for (unsigned p = 0; p < n; ++p)
        std::sort(e + row_off[p], e + row_off[p + 1], [](const Entry &a, const Entry &b) {
            if (a.i != b.i) return a.i < b.i;
            if (a.j != b.j) return a.j < b.j;
            if (a.k != b.k) return a.k < b.k;
            return a.type < b.type;
        });
    return 0;
}

// Counting sort of the 4 ndihedrals memberships by particle, then each row sorted by the canonical (i, j, k, l, type), i < l.  The
// rows are written as two sections: 4 ndihedrals x (i, j, k, l), then the 4 ndihedrals types in the same order.
extern "C" int pse_host_dihedral_rows(unsigned n, unsigned ndihedrals, const unsigned *quads, const unsigned *types, int *row_off,
                                      unsigned *entries) {
    if (!quads || !row_off || !entries) return fail(PSE_ERR_INVALID, "pse_host_dihedral_rows: null array");
    if (n == 0) return fail(PSE_ERR_INVALID, "pse_host_dihedral_rows: n = 0");
    if (ndihedrals == 0 || ndihedrals > (1u << 28))
        return fail(PSE_ERR_INVALID, "pse_host_dihedral_rows: ndihedrals = %u outside (0, 2^28]", ndihedrals);
    for (unsigned a = 0; a < ndihedrals; ++a) {
        const unsigned *q = quads + 4 * (size_t)a;
        if (q[0] >= n || q[1] >= n || q[2] >= n || q[3] >= n)
            return fail(PSE_ERR_INVALID, "pse_host_dihedral_rows: dihedral %u = (%u, %u, %u, %u) has an index >= n = %u", a, q[0], q[1], q[2], q[3], n);
        if (q[0] == q[1] || q[0] == q[2] || q[0] == q[3] || q[1] == q[2] || q[1] == q[3] || q[2] == q[3])
            return fail(PSE_ERR_INVALID, "pse_host_dihedral_rows: dihedral %u = (%u, %u, %u, %u) has two equal members", a, q[0], q[1], q[2], q[3]);
    }
    std::fill(row_off, row_off + (size_t)n + 1, 0);   // (4 ndihedrals <= 2^30 < 2^31)
    for (size_t m = 0; m < 4 * (size_t)ndihedrals; ++m) ++row_off[quads[m] + 1];
    for (unsigned p = 0; p < n; ++p) row_off[p + 1] += row_off[p];
    std::vector<int> fill(row_off, row_off + n);
    struct Entry { unsigned i, j, k, l, type; };
    std::vector<Entry> e(4 * (size_t)ndihedrals);
    for (unsigned a = 0; a < ndihedrals; ++a) {
        const unsigned *q = quads + 4 * (size_t)a, t = types ? types[a] : 0u;
        const Entry en = q[3] < q[0] ? Entry{q[3], q[2], q[1], q[0], t} : Entry{q[0], q[1], q[2], q[3], t};
        e[fill[en.i]++] = en;
        e[fill[en.j]++] = en;
        e[fill[en.k]++] = en;
        e[fill[en.l]++] = en;
    }
    for (unsigned p = 0; p < n; ++p)
        std::sort(e.begin() + row_off[p], e.begin() + row_off[p + 1], [](const Entry &a, const Entry &b) {
            if (a.i != b.i) return a.i < b.i;
            if (a.j != b.j) return a.j < b.j;
            if (a.k != b.k) return a.k < b.k;
            if (a.l != b.l) return a.l < b.l;
            return a.type < b.type;
        });
    unsigned *ty = entries + 16 * (size_t)ndihedrals;
    for (size_t m = 0; m < e.size(); ++m) {
        entries[4 * m] = e[m].i; entries[4 * m + 1] = e[m].j; entries[4 * m + 2] = e[m].k; entries[4 * m + 3] = e[m].l;
        ty[m] = e[m].type;
    }
    return 0;
}

// The pairs as sorted, unique (min, max) keys; walked in that order, row p receives its partners below p (from the keys whose first
// member they are, ascending) before its partners above p (from the keys that start with p, ascending): every row comes out sorted
// without a sort of its own.  O(npairs log npairs).
extern "C" int pse_host_exclusion_rows(unsigned n, unsigned npairs, const unsigned *pairs, int *row_off, unsigned *entries) {
    if (!pairs || !row_off || !entries) return fail(PSE_ERR_INVALID, "pse_host_exclusion_rows: null array");
    if (n == 0) return fail(PSE_ERR_INVALID, "pse_host_exclusion_rows: n = 0");
    if (npairs == 0 || npairs > (1u << 30)) return fail(PSE_ERR_INVALID, "pse_host_exclusion_rows: npairs = %u outside (0, 2^30]", npairs);
    for (unsigned b = 0; b < npairs; ++b) {
        const unsigned i = pairs[2 * (size_t)b], j = pairs[2 * (size_t)b + 1];
        if (i >= n || j >= n) return fail(PSE_ERR_INVALID, "pse_host_exclusion_rows: pair %u = (%u, %u) has an index >= n = %u", b, i, j, n);
        if (i == j) return fail(PSE_ERR_INVALID, "pse_host_exclusion_rows: pair %u excludes particle %u from itself", b, i);
    }
    std::vector<uint64_t> key(npairs);
    for (unsigned b = 0; b < npairs; ++b) {
        const unsigned i = pairs[2 * (size_t)b], j = pairs[2 * (size_t)b + 1];
        key[b] = ((uint64_t)std::min(i, j) << 32) | std::max(i, j);
    }
    std::sort(key.begin(), key.end());
    key.erase(std::unique(key.begin(), key.end()), key.end());
    // (offsets are counted as unsigned: at the cap of 2^30 distinct pairs the last one is 2^31, which the device reads as unsigned too)
    unsigned *off = reinterpret_cast<unsigned *>(row_off);
    std::fill(off, off + (size_t)n + 1, 0u);
    for (uint64_t k : key) { ++off[(unsigned)(k >> 32) + 1]; ++off[(unsigned)k + 1]; }
    for (unsigned i = 0; i < n; ++i) off[i + 1] += off[i];
    std::vector<unsigned> fill(off, off + n);
    for (uint64_t k : key) {
        const unsigned lo = (unsigned)(k >> 32), hi = (unsigned)k;
        entries[fill[lo]++] = hi;
        entries[fill[hi]++] = lo;
    }
    return 0;
}

// One table after another in the order of the pair types, an off pair type taking no room (see include/pse_amd.h).
extern "C" int pse_host_typed_table_layout(int ntypes, const int *width, const double *rmin, const double *rmax, int *base, double *scale,
                                           double *rmax2, int *total) {
    if (!base || !scale || !rmax2 || !total) return fail(PSE_ERR_INVALID, "pse_host_typed_table_layout: null array (base, scale, rmax2, total)");
    return typed_layout("pse_host_typed_table_layout", ntypes, width, rmin, rmax, base, scale, rmax2, total);
}

// The layout of molecule_layout, copied into the caller's arrays.
extern "C" int pse_host_molecule_rows(unsigned n, unsigned nbonds, const unsigned *pairs, int *mol_of, unsigned *members, unsigned *parent,
                                      unsigned *depth, unsigned *mol_off, unsigned *ends, unsigned *nring, unsigned *tile_mol,
                                      unsigned *tile_rounds, unsigned *counts) {
    if (!pairs || !mol_of || !members || !parent || !depth || !mol_off || !ends || !nring || !tile_mol || !tile_rounds || !counts)
        return fail(PSE_ERR_INVALID, "pse_host_molecule_rows: null array");
    MoleculeLayout L;
    if (int rc = molecule_layout("pse_host_molecule_rows", n, nbonds, pairs, L)) return rc;
    std::copy(L.mol_of.begin(), L.mol_of.end(), mol_of);
    std::copy(L.members.begin(), L.members.end(), members);
    std::copy(L.parent.begin(), L.parent.end(), parent);
    std::copy(L.depth.begin(), L.depth.end(), depth);
    std::copy(L.mol_off.begin(), L.mol_off.end(), mol_off);
    std::copy(L.ends.begin(), L.ends.end(), ends);
    std::copy(L.nring.begin(), L.nring.end(), nring);
    std::copy(L.tile_mol.begin(), L.tile_mol.end(), tile_mol);
    std::copy(L.tile_rounds.begin(), L.tile_rounds.end(), tile_rounds);
    counts[0] = L.nmol; counts[1] = (unsigned)L.members.size(); counts[2] = L.ntiles;
    return 0;
}

// The rank of every member slot of the layout of pse_host_molecule_rows (see include/pse_amd.h).
extern "C" int pse_host_chain_order(unsigned nmol, const unsigned *parent, const unsigned *mol_off, const unsigned *ends, unsigned *rank) {
    if (!parent || !mol_off || !ends || !rank) return fail(PSE_ERR_INVALID, "pse_host_chain_order: null array");
    chain_ranks(nmol, parent, mol_off, ends, rank);
    return 0;
}

// The angle pi p (2 q + 1) / (2 m) as the integer j = p (2 q + 1) mod 4 m of quarter turns / m, folded into the first quadrant, so
// that mirrored ranks meet the same cos call; the call and the division by m in extended precision, rounded once.
extern "C" int pse_host_rouse_weights(unsigned m, int nmodes, double *out) {
    const char *who = "pse_host_rouse_weights";
    if (!out) return fail(PSE_ERR_INVALID, "%s: null out", who);
    if (m < 2) return fail(PSE_ERR_INVALID, "%s: m = %u, a chain has at least two members", who, m);
    if (nmodes < 1 || nmodes > CHAIN_MODES_MAX) return fail(PSE_ERR_INVALID, "%s: nmodes = %d outside [1, %d]", who, nmodes, CHAIN_MODES_MAX);
    if ((unsigned)(nmodes - 1) >= m) return fail(PSE_ERR_INVALID, "%s: nmodes - 1 = %d modes, a chain of m = %u members has only %u", who, nmodes - 1, m, m - 1u);
    std::fill(out, out + m, 0.0);
    out[0] = -1.0; out[m - 1] = 1.0;
    const uint64_t M = m;
    const long double pi = 3.14159265358979323846264338327950288L;
    for (int p = 1; p < nmodes; ++p)
        for (uint64_t q = 0; q < M; ++q) {
            uint64_t j = ((uint64_t)p * (2u * q + 1u)) % (4u * M);
            bool neg = false;
            if (j > 2u * M) j = 4u * M - j;
            if (j > M) { j = 2u * M - j; neg = true; }
            const double c = j == M ? 0.0 : (double)(cosl(pi * (long double)j / (long double)(2u * M)) / (long double)M);
            out[(size_t)p * m + q] = neg ? -c : c;
        }
    return 0;
}
