// Host integrator class of the PSE method, HOOMD-free: the counterpart of `class Stokes : IntegrationMethodTwoStep`
// (PSEv1/Stokes.h:86-161, PSEv1/Stokes.cc:85-530).  It owns a pse_handle and calls the C-ABI (include/pse_amd.h);
// the particle arrays stay with the caller (HOOMD's ParticleData in the reference, PSEv1/Stokes.cc:454-461).
#pragma once
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/pse_amd.h"
#include "ShearFunction.h"

namespace pse_host {

struct BoxDim {   // the part of HOOMD's BoxDim the path uses: lengths and the xy tilt factor
    double Lx, Ly, Lz, xy;
};

// device pointers of the particle data the step touches (ArrayHandle acquisitions at PSEv1/Stokes.cc:454-461)
struct ParticleArrays {
    pse_double4 *pos; pse_double4 *vel; pse_double3 *accel; pse_int3 *image; const pse_double4 *net_force;
    const unsigned int *group_members;   // may be null: all particles
    unsigned int group_size;
};

// The objects of one kind that a Stokes made on its engine, by id -- the position in the table; null once destroyed.
template <class T>
struct IdTable {
    const char *what;   // "bond", "angle", "dihedral", "exclusion", "typed table": what the error calls them
    std::vector<T *> objs;
    int push(T *o) { objs.push_back(o); return (int)objs.size() - 1; }
    T *get(int id) const {
        if (id < 0 || id >= (int)objs.size() || !objs[id])
            throw std::invalid_argument(std::string("Stokes: no ") + what + " object with id " + std::to_string(id) + " (setParams invalidates the ids)");
        return objs[id];
    }
    void drop(int id) { objs[id] = nullptr; }
};

class Stokes {
public:
    // (sysdef, group, T, seed, nlist, xi, error) of the reference become (n_total, box, T, seed, xi, error): the
    // neighbour list is internal to the engine (PSEv1/Stokes.cc:85-111)
    Stokes(unsigned int n_total, BoxDim box, std::shared_ptr<Variant> T, unsigned int seed, double xi, double error, double dt);
    ~Stokes();
    void setT(std::shared_ptr<Variant> T) { m_T = T; }                                     // Stokes.h:106-109
    void setShear(std::shared_ptr<ShearFunction> f, double max_strain) { m_shear_func = f; m_max_strain = max_strain; }  // Stokes.h:118-121
    void setDeltaT(double dt) { m_deltaT = dt; }
    // explicit overrides of the parameter rule (0 = reference rule); must precede setParams
    void setOverrides(int Nx, int Ny, int Nz, int P, double rcut) { m_Nx = Nx; m_Ny = Ny; m_Nz = Nz; m_P = P; m_rcut = rcut; }
    void setParams();                                                                      // Stokes.cc:129-424
    // the near-field operator of the Lanczos noise (enum pse_lanczos_operator; -1: the engine's default): applied now if the engine
    // exists, and again by every setParams.  No reference counterpart (the reference's Lanczos is single precision throughout)
    void setLanczosOperator(int op);
    void setBox(BoxDim box);                                                               // per-step box under shear
    void integrateStepOne(unsigned int timestep, const ParticleArrays &p);                 // Stokes.cc:429-523
    void integrateStepTwo(unsigned int) {}                                                 // Stokes.cc:528-530
    // force provider on the integrator's own cell list (the reference takes net_force from HOOMD, Stokes.cc:447)
    void pairRepulsion(const pse_double4 *pos, pse_double4 *force, const unsigned int *group, unsigned int n, double k,
                       double sigma, bool accumulate);
    // ... and the same pass with the pair observables a rheology run samples (pse_pair_repulsion_virial): out8 = U, Wxx, Wxy, Wxz, Wyy,
    // Wyz, Wzz, npairs, eight DEVICE doubles written by the stream; force may be null (observables only)
    void pairRepulsionVirial(const pse_double4 *pos, pse_double4 *force, const unsigned int *group, unsigned int n, double k,
                             double sigma, bool accumulate, double *out8);
    // a tabulated central pair potential on the same cell list (pse_pair_table): table = width x (V, F) DEVICE doubles at the nodes
    // rmin + k (rmax - rmin)/(width - 1), linear in between; force or out8 may be null (observables only / forces only), not both
    void pairTable(const pse_double4 *pos, pse_double4 *force, const unsigned int *group, unsigned int n, const double *table, int width,
                   double rmin, double rmax, bool accumulate, double *out8);
    // pair exclusions (pse_exclusions_create; HOOMD's nlist.reset_exclusions): exclusionsCreate copies the HOST array of npairs x 2
    // caller-order particle indices to the engine and returns the id the two passes below take; the ids live and die as those of the
    // bond objects do
    int exclusionsCreate(unsigned int n, unsigned int npairs, const unsigned int *pairs);
    void exclusionsDestroy(int id);
    // pairTable with the pairs of exclusion object `ex` contributing nothing (pse_pair_table_excl)
    void pairTableExcl(const pse_double4 *pos, pse_double4 *force, const unsigned int *group, unsigned int n, const double *table, int width,
                       double rmin, double rmax, bool accumulate, double *out8, int ex);
    // the repulsion likewise (pse_pair_repulsion_excl): out8 null is pairRepulsion, out8 given is pairRepulsionVirial
    void pairRepulsionExcl(const pse_double4 *pos, pse_double4 *force, const unsigned int *group, unsigned int n, double k, double sigma,
                           bool accumulate, double *out8, int ex);
    // typed pair tables (pse_typed_table_create; HOOMD's pair.table with one pair_coeff per pair of types): typedTableCreate copies the
    // HOST arrays -- n types, and per pair type p(a, b) of the header a width (0: off), rmin and rmax, then the (V, F) tables one after
    // another -- to the engine and returns the id that pairTableTyped takes; the ids live and die as those of the bond objects do
    int typedTableCreate(unsigned int n, const unsigned int *types, int ntypes, const int *width, const double *rmin, const double *rmax,
                         const double *tables);
    void typedTableDestroy(int id);
    // the pass of typed table `typed` (pse_pair_table_typed); ex: the id of an exclusion object, or negative: nothing is excluded
    void pairTableTyped(const pse_double4 *pos, pse_double4 *force, const unsigned int *group, unsigned int n, bool accumulate, double *out8,
                        int typed, int ex);
    // bonded forces (pse_bonds_create / pse_bond_forces / pse_bonds_overstretched): bondsCreate copies the HOST arrays -- nbonds x 2
    // particle indices, nbonds types or null, ntypes x (kind, k, r0) -- to the engine and returns the id the other calls take.  The
    // bond objects belong to the engine: setParams, which makes a new one, invalidates every id
    int bondsCreate(unsigned int n, unsigned int nbonds, const unsigned int *pairs, const unsigned int *types, int ntypes, const int *kind,
                    const double *k, const double *r0);
    // force or out8 (eight DEVICE doubles: U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, nbonds) may be null, not both
    void bondForces(int id, const pse_double4 *pos, pse_double4 *force, bool accumulate, double *out8);
    unsigned long long bondsOverstretched(int id);   // waits for the stream
    void bondsDestroy(int id);
    // angle forces (pse_angles_create / pse_angle_forces): anglesCreate copies the HOST arrays -- nangles x 3 particle indices (end,
    // vertex, end), nangles types or null, ntypes x (kind, k, theta0) -- to the engine and returns the id the other calls take; the
    // ids live and die as those of the bond objects do
    int anglesCreate(unsigned int n, unsigned int nangles, const unsigned int *triples, const unsigned int *types, int ntypes, const int *kind,
                     const double *k, const double *theta0);
    // force or out8 (eight DEVICE doubles: U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, nangles) may be null, not both
    void angleForces(int id, const pse_double4 *pos, pse_double4 *force, bool accumulate, double *out8);
    void anglesDestroy(int id);
    // dihedral forces (pse_dihedrals_create / pse_dihedral_forces): dihedralsCreate copies the HOST arrays -- ndihedrals x 4 particle
    // indices (i, j, k, l), ndihedrals types or null, ntypes kinds and ntypes x 4 parameters -- to the engine and returns the id the
    // other calls take; the ids live and die as those of the bond objects do
    int dihedralsCreate(unsigned int n, unsigned int ndihedrals, const unsigned int *quads, const unsigned int *types, int ntypes,
                        const int *kind, const double *params);
    // force or out8 (eight DEVICE doubles: U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, ndihedrals) may be null, not both
    void dihedralForces(int id, const pse_double4 *pos, pse_double4 *force, bool accumulate, double *out8);
    void dihedralsDestroy(int id);
    pse_info info() const;
    int lanczosIterations() const { return m_m_Lanczos; }
    unsigned int hashedSeed() const { return m_seed; }
    pse_handle *handle() const { return m_h; }
private:
    unsigned int m_n_total;
    BoxDim m_box;
    std::shared_ptr<Variant> m_T;
    unsigned int m_seed;
    double m_xi, m_error, m_deltaT;
    std::shared_ptr<ShearFunction> m_shear_func;
    double m_max_strain = 0.5;
    int m_Nx = 0, m_Ny = 0, m_Nz = 0, m_P = 0;
    double m_rcut = 0.0;
    int m_m_Lanczos = 2;                                                                   // Stokes.cc:132
    int m_lanczos_op = -1;
    pse_handle *m_h = nullptr;
    IdTable<pse_bonds> m_bonds{"bond"};
    IdTable<pse_angles> m_angles{"angle"};
    IdTable<pse_dihedrals> m_dihedrals{"dihedral"};
    IdTable<pse_exclusions> m_exclusions{"exclusion"};
    IdTable<pse_typed_table> m_typed{"typed table"};
};

}  // namespace pse_host
