#include "Stokes.h"

#include <stdexcept>

namespace pse_host {

static void check(int status, const char *what) {
    if (status != PSE_OK) throw std::runtime_error(std::string(what) + ": " + pse_last_error());
}

Stokes::Stokes(unsigned int n_total, BoxDim box, std::shared_ptr<Variant> T, unsigned int seed, double xi, double error, double dt)
    : m_n_total(n_total), m_box(box), m_T(T), m_seed(seed), m_xi(xi), m_error(error), m_deltaT(dt) {
    // hash the user's seed so that it is unlikely to be a low positive integer (PSEv1/Stokes.cc:102)
    m_seed = m_seed * 0x12345677u + 0x12345u;
    m_seed ^= (m_seed >> 16);
    m_seed *= 0x45679u;
    m_shear_func = std::make_shared<SteadyShearFunction>(0.0, 0u, 0.0);   // integrate.py:93-94 default
}

Stokes::~Stokes() {
    if (m_h) pse_destroy(m_h);
}

void Stokes::setParams() {
    if (m_h) { pse_destroy(m_h); m_h = nullptr; }
    m_bonds.objs.clear();   // pse_destroy freed them
    m_angles.objs.clear();
    m_dihedrals.objs.clear();
    m_exclusions.objs.clear();
    m_typed.objs.clear();
    m_m_Lanczos = 2;   // "try two Lanczos iterations to start" (PSEv1/Stokes.cc:131-132)
    pse_params p{};
    p.n_max = m_n_total;
    p.Lx = m_box.Lx; p.Ly = m_box.Ly; p.Lz = m_box.Lz; p.xy = m_box.xy;
    p.xi = m_xi; p.error = m_error; p.max_strain = m_max_strain; p.seed = m_seed;
    p.Nx = m_Nx; p.Ny = m_Ny; p.Nz = m_Nz; p.P = m_P; p.rcut = m_rcut;
    p.device = -1; p.n_slabs = 1; p.slab_rank = 0;
    check(pse_create(&p, &m_h), "Error initializing Stokes");
    if (m_lanczos_op >= 0) check(pse_set_lanczos_operator(m_h, m_lanczos_op), "Stokes::setLanczosOperator");
}

void Stokes::setLanczosOperator(int op) {
    if (op != PSE_LANCZOS_RECORDS16 && op != PSE_LANCZOS_FP64) throw std::invalid_argument("Stokes::setLanczosOperator: unknown operator");
    m_lanczos_op = op;
    if (m_h) check(pse_set_lanczos_operator(m_h, op), "Stokes::setLanczosOperator");
}

void Stokes::setBox(BoxDim box) {
    m_box = box;
    if (m_h) check(pse_set_box(m_h, box.Lx, box.Ly, box.Lz, box.xy), "Stokes::setBox");
}

void Stokes::integrateStepOne(unsigned int timestep, const ParticleArrays &p) {
    if (!m_h) throw std::runtime_error("Stokes::setParams() has not been called");
    if (p.group_size == 0) return;                                       // Stokes.cc:443-444
    const double shear_rate = m_shear_func->getShearRate(timestep);      // Stokes.cc:473
    check(pse_step(m_h, p.pos, p.vel, p.accel, p.image, p.net_force, p.group_members, p.group_size,
                   m_T->getValue(timestep), m_deltaT, timestep, shear_rate, &m_m_Lanczos),
          "Stokes::integrateStepOne");
}

void Stokes::pairRepulsion(const pse_double4 *pos, pse_double4 *force, const unsigned int *group, unsigned int n, double k,
                           double sigma, bool accumulate) {
    if (!m_h) throw std::runtime_error("Stokes::setParams() has not been called");
    if (n == 0) return;
    check(pse_pair_repulsion(m_h, pos, force, group, n, k, sigma, accumulate ? 1 : 0), "Stokes::pairRepulsion");
}

void Stokes::pairRepulsionVirial(const pse_double4 *pos, pse_double4 *force, const unsigned int *group, unsigned int n, double k,
                                 double sigma, bool accumulate, double *out8) {
    if (!m_h) throw std::runtime_error("Stokes::setParams() has not been called");
    // (an empty group is refused by the C-ABI: there is no device code here that could write zeros to out8)
    check(pse_pair_repulsion_virial(m_h, pos, force, group, n, k, sigma, accumulate ? 1 : 0, out8), "Stokes::pairRepulsionVirial");
}

void Stokes::pairTable(const pse_double4 *pos, pse_double4 *force, const unsigned int *group, unsigned int n, const double *table,
                       int width, double rmin, double rmax, bool accumulate, double *out8) {
    if (!m_h) throw std::runtime_error("Stokes::setParams() has not been called");
    check(pse_pair_table(m_h, pos, force, group, n, table, width, rmin, rmax, accumulate ? 1 : 0, out8), "Stokes::pairTable");
}

int Stokes::exclusionsCreate(unsigned int n, unsigned int npairs, const unsigned int *pairs) {
    if (!m_h) throw std::runtime_error("Stokes::setParams() has not been called");
    pse_exclusions *ex = nullptr;
    check(pse_exclusions_create(m_h, n, npairs, pairs, &ex), "Stokes::exclusionsCreate");
    return m_exclusions.push(ex);
}

void Stokes::exclusionsDestroy(int id) {
    check(pse_exclusions_destroy(m_exclusions.get(id)), "Stokes::exclusionsDestroy");
    m_exclusions.drop(id);
}

void Stokes::pairTableExcl(const pse_double4 *pos, pse_double4 *force, const unsigned int *group, unsigned int n, const double *table,
                           int width, double rmin, double rmax, bool accumulate, double *out8, int ex) {
    if (!m_h) throw std::runtime_error("Stokes::setParams() has not been called");
    check(pse_pair_table_excl(m_h, pos, force, group, n, table, width, rmin, rmax, accumulate ? 1 : 0, out8, m_exclusions.get(ex)),
          "Stokes::pairTableExcl");
}

void Stokes::pairRepulsionExcl(const pse_double4 *pos, pse_double4 *force, const unsigned int *group, unsigned int n, double k,
                               double sigma, bool accumulate, double *out8, int ex) {
    if (!m_h) throw std::runtime_error("Stokes::setParams() has not been called");
    if (n == 0 && !out8) return;   // (as pairRepulsion; with out8 an empty group is refused by the C-ABI, as in pairRepulsionVirial)
    check(pse_pair_repulsion_excl(m_h, pos, force, group, n, k, sigma, accumulate ? 1 : 0, out8, m_exclusions.get(ex)),
          "Stokes::pairRepulsionExcl");
}

int Stokes::typedTableCreate(unsigned int n, const unsigned int *types, int ntypes, const int *width, const double *rmin, const double *rmax,
                             const double *tables) {
    if (!m_h) throw std::runtime_error("Stokes::setParams() has not been called");
    pse_typed_table *t = nullptr;
    check(pse_typed_table_create(m_h, n, types, ntypes, width, rmin, rmax, tables, &t), "Stokes::typedTableCreate");
    return m_typed.push(t);
}

void Stokes::typedTableDestroy(int id) {
    check(pse_typed_table_destroy(m_typed.get(id)), "Stokes::typedTableDestroy");
    m_typed.drop(id);
}

void Stokes::pairTableTyped(const pse_double4 *pos, pse_double4 *force, const unsigned int *group, unsigned int n, bool accumulate,
                            double *out8, int typed, int ex) {
    if (!m_h) throw std::runtime_error("Stokes::setParams() has not been called");
    check(pse_pair_table_typed(m_typed.get(typed), pos, force, group, n, accumulate ? 1 : 0, out8, ex < 0 ? nullptr : m_exclusions.get(ex)),
          "Stokes::pairTableTyped");
}

int Stokes::bondsCreate(unsigned int n, unsigned int nbonds, const unsigned int *pairs, const unsigned int *types, int ntypes, const int *kind,
                        const double *k, const double *r0) {
    if (!m_h) throw std::runtime_error("Stokes::setParams() has not been called");
    pse_bonds *b = nullptr;
    check(pse_bonds_create(m_h, n, nbonds, pairs, types, ntypes, kind, k, r0, &b), "Stokes::bondsCreate");
    return m_bonds.push(b);
}

void Stokes::bondForces(int id, const pse_double4 *pos, pse_double4 *force, bool accumulate, double *out8) {
    check(pse_bond_forces(m_bonds.get(id), pos, force, accumulate ? 1 : 0, out8), "Stokes::bondForces");
}

unsigned long long Stokes::bondsOverstretched(int id) {
    unsigned long long c = 0;
    check(pse_bonds_overstretched(m_bonds.get(id), &c), "Stokes::bondsOverstretched");
    return c;
}

void Stokes::bondsDestroy(int id) {
    check(pse_bonds_destroy(m_bonds.get(id)), "Stokes::bondsDestroy");
    m_bonds.drop(id);
}

int Stokes::anglesCreate(unsigned int n, unsigned int nangles, const unsigned int *triples, const unsigned int *types, int ntypes,
                         const int *kind, const double *k, const double *theta0) {
    if (!m_h) throw std::runtime_error("Stokes::setParams() has not been called");
    pse_angles *a = nullptr;
    check(pse_angles_create(m_h, n, nangles, triples, types, ntypes, kind, k, theta0, &a), "Stokes::anglesCreate");
    return m_angles.push(a);
}

void Stokes::angleForces(int id, const pse_double4 *pos, pse_double4 *force, bool accumulate, double *out8) {
    check(pse_angle_forces(m_angles.get(id), pos, force, accumulate ? 1 : 0, out8), "Stokes::angleForces");
}

void Stokes::anglesDestroy(int id) {
    check(pse_angles_destroy(m_angles.get(id)), "Stokes::anglesDestroy");
    m_angles.drop(id);
}

int Stokes::dihedralsCreate(unsigned int n, unsigned int ndihedrals, const unsigned int *quads, const unsigned int *types, int ntypes,
                            const int *kind, const double *params) {
    if (!m_h) throw std::runtime_error("Stokes::setParams() has not been called");
    pse_dihedrals *d = nullptr;
    check(pse_dihedrals_create(m_h, n, ndihedrals, quads, types, ntypes, kind, params, &d), "Stokes::dihedralsCreate");
    return m_dihedrals.push(d);
}

void Stokes::dihedralForces(int id, const pse_double4 *pos, pse_double4 *force, bool accumulate, double *out8) {
    check(pse_dihedral_forces(m_dihedrals.get(id), pos, force, accumulate ? 1 : 0, out8), "Stokes::dihedralForces");
}

void Stokes::dihedralsDestroy(int id) {
    check(pse_dihedrals_destroy(m_dihedrals.get(id)), "Stokes::dihedralsDestroy");
    m_dihedrals.drop(id);
}

pse_info Stokes::info() const {
    pse_info i{};
    if (m_h) pse_get_info(m_h, &i);
    return i;
}

}  // namespace pse_host
