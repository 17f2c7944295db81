// Internal host-side declarations shared by the parameter/table builder and the C-ABI driver.
#pragma once
#include <string>
#include <vector>

namespace pse {

// Degree of the per-interval polynomials of the real-space (smooth part) table and interval count per unit r.
constexpr int RS_DEG = 9;           // 10 coefficients per function
constexpr int RS_NCOEF = RS_DEG + 1;
constexpr int RS_PER_UNIT = 8;      // intervals of width 1/8 (in units of the particle radius)

constexpr int PAIR_TABLE_MAX_WIDTH = 2048;   // entries of a pair table (pse_pair_table): staged in 32 KB of LDS
constexpr int PAIR_HIST_MAX_COUNTERS = 8192;   // counters of a pair histogram (pse_pair_hist_create), pair types x bins: 32 KB of LDS
constexpr int SF_MAX_INDEX = 4096;     // |mx|, |my|, |mz| of a structure-factor mode (pse_structure_factor_create; PSE_SF_MAX_INDEX)
constexpr int SF_MAX_MODES = 32768;    // modes of one structure-factor object (PSE_SF_MAX_MODES)
constexpr int SF_RUN = 8;              // modes of one segment: a lane of k_sf_partial keeps their sums in registers, seeded exactly, 7 steps
constexpr int SF_SHORT = 2;            // a segment of at most this many modes is walked by the short form of the kernel (k_sf_partial<SF_SHORT>)
constexpr int MSD_MAX_ORIGINS = 64;   // slots of one displacement object, and pairs (slot, row) of one pse_msd_accumulate (PSE_MSD_MAX_ORIGINS)
constexpr int MSD_MOMENTS = 10;       // dx dy dz, dx^2 dy^2 dz^2 dxdy dxdz dydz, |d|^4 (PSE_MSD_MOMENTS)
constexpr int ISF_MAX_ORIGINS = 64;   // slots of one scattering object, and pairs (slot, row) of one pse_isf_correlate (PSE_ISF_MAX_ORIGINS)
constexpr int ISF_MAX_MODES = 4096;   // modes of one scattering object (PSE_ISF_MAX_MODES): the self pass keeps a partial sum per (span, pair, type, mode)
constexpr int BOND_ORDER_MAX_DEGREES = 4;   // degrees of one bond-order object (pse_bond_order_create; PSE_BOND_ORDER_MAX_DEGREES)
constexpr int BOND_ORDER_MAX_L = 12;        // the largest degree, even degrees 2..12 (PSE_BOND_ORDER_MAX_L)
constexpr int BOND_ORDER_MAX_COUNTERS = 8192;   // counters of pse_bond_order_histogram, types x bins: 32 KB of LDS
constexpr int MOL_COLS = 14;          // columns of a molecule's row and of a type's sums (pse_molecules_compute; PSE_MOL_COLS)
constexpr int MOL_MAX_BINS = 4096;    // bins of each histogram of a molecule object (pse_molecules_create)
constexpr int MOLPAIR_COLS = 2;       // per separation of a chain-statistics curve: D, C (pse_molecule_pairs_compute; PSE_MOLPAIR_COLS)
constexpr int MOLPAIR_SUMS = 2;       // per type: the sum of 1/Rh and of (1/Rh)^2 (PSE_MOLPAIR_SUMS)
constexpr int CHAIN_MODES_MAX = 32;   // functionals of one chain-modes object (pse_chain_modes_create; PSE_CHAIN_MODES_MAX)
constexpr int CHAIN_MODES_STATIC = 6; // per type and functional: the sums of X_x^2, X_y^2, X_z^2, X_x X_y, X_x X_z, X_y X_z (PSE_CHAIN_MODES_STATIC)
constexpr int CHAIN_MODES_CORR = 9;   // per row, type and functional: the sums of X_a(now) X_b(slot), 3 a + b (PSE_CHAIN_MODES_CORR)
constexpr int PAIR_TYPED_MAX_TYPES = 8;     // particle types of a typed pair table (pse_typed_table_create): at most 36 pair types
constexpr int PAIR_TYPED_MAX_ENTRIES = 3584; // entries of all its tables together: 56 KB of LDS, next to 1.4 KB of static LDS, inside 64 KB
constexpr int BOND_MAX_TYPES = 64;   // parameter sets of a bond object (pse_bonds_create): staged in 2 KB of LDS
constexpr int ANGLE_MAX_TYPES = 64;  // parameter sets of an angle object (pse_angles_create): staged in 2 KB of LDS
constexpr int DIHEDRAL_MAX_TYPES = 64;   // parameter sets of a dihedral object (pse_dihedrals_create): staged in 3 KB of LDS

struct Box {
    double Lx, Ly, Lz, xy;
};

// Everything Stokes::setParams derives (PSEv1/Stokes.cc:129-319).
struct Derived {
    double xi, error, max_strain;
    double rcut;          // Stokes.cc:135
    int kmax;             // Stokes.cc:138
    int Nx, Ny, Nz;       // Stokes.cc:143-199
    double lambda;        // Stokes.cc:217-219
    double gaussm;        // Stokes.cc:225-228
    int P;                // Stokes.cc:229-233
    double eta;           // Stokes.cc:234-236
    double hx, hy, hz;    // Stokes.cc:222
    double self;          // Stokes.cc:319
};

// Returns empty string on success, otherwise an error message.
std::string select_params(const Box &box, double xi, double error, double max_strain,
                          int Nx, int Ny, int Nz, int P, double rcut, Derived &out);

// Real-space table: for interval k (r in [k/8,(k+1)/8)) and local t = 2*(8r-k)-1 in [-1,1):
//   f_w(r) = sum_q coef[k][q] t^q,  g_w(r) = sum_q coef[k][RS_NCOEF+q] t^q
// are the *smooth* (free-space wave) parts; the device adds the analytic RPY branch:
//   f = f_RPY - f_w, g = g_RPY - g_w   (replaces m_ewaldC1, PSEv1/Stokes.cc:334-422).
void build_realspace_table(double xi, double rcut, std::vector<double> &coef, int &n_intervals);
int realspace_table_intervals(double rcut);   // ceil(8 rcut) + 1: the interval that holds rcut, and one beyond

// Symmetric tridiagonal eigen-decomposition (implicit QL), replaces LAPACKE_spteqr (PSEv1/Brownian.cu:540).
// d[0..n) diagonal, e[0..n-1) off-diagonal. On return d = eigenvalues, z (n x n, row-major) = eigenvectors in
// columns. Returns false if it fails to converge.
bool tridiag_eigen(int n, std::vector<double> &d, std::vector<double> &e, std::vector<double> &z);

// t = T^{1/2} e_1 for the Lanczos tridiagonal T(alpha[0..m), beta[1..m)) (PSEv1/Brownian.cu:563-582).
bool lanczos_sqrt_e1(int m, const double *alpha, const double *beta, std::vector<double> &t);

// ---- the convergence decision of the Lanczos iteration: ONE contract, LzDecide in, LzState out --------------------------------------
// What ends the iteration is the reference's while loop (its breakdown test, PSEv1/Brownian.cu:503, the eigen-solve and the step-norm
// test, PSEv1/Brownian.cu:540-582,606-724): walk m upward one size at a time and stop once the step norm is below the tolerance.  A
// driver issues one decision per batch of iterations; the state carries the walk from one decision to the next.  Two implementations:
// k_lz_decide (pse_vectors.hip) for the queue-only drivers, which may not wait for the host, and lz_decide_host (pse_params.cpp) for
// the host-checked ones.
constexpr int M_MAX = 100;   // Lanczos basis cap (PSEv1/Brownian.cu:397)
constexpr int LZ_ALPHA = 0, LZ_BETA = 128, LZ_NORM = 256;   // slots of the scalars (device doubles, and the host's copy): alpha_j, beta_j, the norm of psi
struct LzState {
    int done;            // the iteration has ended: m_final and coef are valid; later iteration kernels leave at once
    int m_final;
    int checked;         // t_prev holds T^{1/2} e_1 of this size (0: nothing yet)
    int status;          // 0 converged, 1 the queued iterations ran out first (result from the last size checked), 2 non-finite coefficient / eigen-solve failure
    double stepnorm;
    double t_prev[104];
    double coef[104];    // coefficients of the basis vectors in the final combination (t divided by the norms the basis carries)
};
struct LzDecide {
    int m_lo, m_hi;      // sizes to check (the device: at most two, m_lo = m_hi - 1 or m_hi)
    int done_iters;      // iterations whose alpha exists; one-step driver: beta[done_iters] does not exist yet
    int have_last_beta;  // 1: beta[done_iters] exists as well (two-step driver of a team)
    int pending_beta;    // > 0: first test beta[pending_beta] for breakdown (it arrived with this batch)
    int first;           // first decision of a call: reset the state
    int last;            // last queued decision: if still open, end the iteration at the last size checked (status 1)
    int normalised;      // the basis holds normalised v_q for q >= 1 (two-step driver); else unnormalised x_q (divide by beta_q)
    int m_max;
    double tol;
};
// The host twin of k_lz_decide, its body line for line, on the host's copy of the scalars; every size of m_lo .. m_hi is solved by
// lanczos_sqrt_e1 (host batches grow, so the range may hold any number of sizes).  Both failures are status 2 in the state; the
// return value tells them apart and `at` names the place: the iteration j of the coefficient, or the size m of the eigen-solve.
// One value differs from the device's: after a failure before any size was solved coef[0] is NaN here, whatever the solver's buffer
// held there -- the host drivers never read it: they return an error on either failure.
enum LzFailure { LZ_OK = 0, LZ_NONFINITE, LZ_EIGEN_FAILED };
LzFailure lz_decide_host(const LzDecide &d, const double *scal, LzState &st, int *at);

}  // namespace pse
