/*
 * pse_amd.h -- C-ABI of the MI355X-native Positively-Split-Ewald (PSE) engine.
 *
 * This is the drop-in boundary for the hot path of stochasticHydroTools/PSE (HOOMD plugin PSEv1):
 * everything below `Stokes::integrateStepOne` (PSEv1/Stokes.cc:429-523), i.e. the driver
 * `gpu_stokes_step_one` (PSEv1/Stokes.cuh:75-111, PSEv1/Stokes.cu:234-365) and the set-up work of
 * `Stokes::setParams` (PSEv1/Stokes.cc:129-424).  Plain C types only; every array argument is a
 * caller-owned DEVICE pointer (as HOOMD's GPUArray handles are, PSEv1/Stokes.cc:436-470) unless a
 * comment says "host".  All entry points return 0 on success or a negative pse_status; the message
 * is available from pse_last_error().  Nothing here ever calls exit() (the reference does:
 * PSEv1/Stokes.cc:203-214, PSEv1/Brownian.cu:543-560).
 *
 * Units and conventions are the reference's: particle radius a = 1, mobility in units of
 * 1/(6 pi eta a) (PSEv1/Stokes.cc:314-319, PSEv1/Helper.cu:326); box centred on the origin with
 * HOOMD's triclinic tilt xy: a1=(Lx,0,0), a2=(xy*Ly,Ly,0), a3=(0,0,Lz) (PSEv1/Mobility.cu:223-230).
 * Arithmetic is fp64 (the reference is effectively fp32), with one stated exception: inside the Lanczos iteration
 * of M_real^{1/2} psi (tolerance `error`) the near-field operator reads its pair coefficients -- f(r) and d sqrt|(g - f) / r^2| -- from
 * the 16-byte records of the per-step pair list, rounded to single-precision accuracy (f to 2^-25 absolute, the vector to 2^-22 of its
 * largest component), and (single GPU) its neighbours' vector rows to 2^-39 of their largest component; sums accumulate in fp64, the
 * operator stays exactly symmetric, the deterministic U = M.F never sees those numbers (oracle/pse_oracle.c pair_term restates the
 * rounding of the coefficients operation by operation; DESIGN.md sections 2 and 4).  That rounding bounds what the tolerance can buy:
 * below about 1e-6 the 16-byte records do NOT honour it (their own error is 1e-6 - 1e-5 of M_real^{1/2} psi in dense suspensions, at
 * large xi or with close pairs).  pse_set_lanczos_operator(h, PSE_LANCZOS_FP64) keeps the operator of the iteration in fp64 throughout
 * -- coefficients, the neighbours' rows and the root -- and then the tolerance holds down to the fp64 round-off.
 */
#ifndef PSE_AMD_H
#define PSE_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

/* HOOMD Scalar4 / Scalar3 / int3 with Scalar = double */
typedef struct { double x, y, z, w; } pse_double4;
typedef struct { double x, y, z; } pse_double3;
typedef struct { int x, y, z; } pse_int3;

typedef struct pse_handle pse_handle;

enum pse_status {
    PSE_OK = 0,
    PSE_ERR_INVALID = -1,   /* bad argument / parameter combination */
    PSE_ERR_HIP = -2,       /* HIP runtime error */
    PSE_ERR_FFT = -3,       /* rocFFT error */
    PSE_ERR_COMM = -4,      /* RCCL error */
    PSE_ERR_NUMERIC = -5    /* Lanczos / eigen-solve breakdown */
};

/* Constructor arguments: what Stokes::Stokes + setShear + setParams receive
 * (PSEv1/Stokes.cc:85-111, PSEv1/Stokes.h:118-121, PSEv1/Stokes.cc:129-236), plus explicit
 * overrides the reference's rule cannot express. Zero means "use the reference rule". */
typedef struct pse_params {
    unsigned int n_max;      /* capacity in particles (N_total of the reference) */
    double Lx, Ly, Lz, xy;   /* box; |xy| <= 0.5 (HOOMD flips the box there; beyond it the minimum image is not exact): else PSE_ERR_INVALID */
    double xi;               /* Ewald splitting parameter (PSEv1/Stokes.cc:91) */
    double error;            /* tolerance for all approximations (m_error); the Lanczos noise honours it below ~1e-6 only with
                                PSE_LANCZOS_FP64 (pse_set_lanczos_operator): the default 16-byte pair records are single-precision accurate */
    double max_strain;       /* largest |xy| the box will take; sizes P (PSEv1/Stokes.cc:217-229) */
    unsigned int seed;       /* RNG seed as used on the device (the host class hashes the user seed, Stokes.cc:102) */
    int Nx, Ny, Nz;          /* FFT grid override (0 = PSEv1/Stokes.cc:138-199).  The reference's rule makes the three spacings equal up
                                to the rounding of the sizes; an override whose coarsest spacing takes the spreading Gaussian (width from
                                the finest) out of the double range over its support is refused: PSE_ERR_INVALID (pse_set_box likewise) */
    int P;                   /* support override (0 = PSEv1/Stokes.cc:225-233) */
    double rcut;             /* real-space cutoff override (0 = PSEv1/Stokes.cc:135) */
    int device;              /* HIP device ordinal, -1 = current device */
    int n_slabs;             /* far-field slab decomposition: number of ranks (<=1: single GPU) */
    int slab_rank;           /* this rank's slab index */
    int local_rows;          /* != 0 (with n_slabs >= 2): an OWNED-PARTICLE rank -- it is driven through pse_team_step_local, n_max is the
                                capacity of its row space (own particles + the ghost layers of both neighbours), not the particle count
                                of the suspension; the replicated-state team calls refuse such a handle */
} pse_params;

typedef struct pse_info {
    int Nx, Ny, Nz, P;
    double rcut, xi, eta, gaussm, lambda, self_mobility, hx, hy, hz;
    int ncell_x, ncell_y, ncell_z;
    int lanczos_m;            /* vectors used by the last Brownian call */
    int lanczos_matvecs;      /* near-field mat-vecs of the last Brownian call */
    double lanczos_stepnorm;  /* last relative step norm */
    /* device time of the phases of the most recent call, ms (hipEvent, only if timing enabled) */
    double t_sort, t_spread, t_fft_fwd, t_scale, t_fft_inv, t_gather, t_real, t_lanczos, t_integrate, t_comm, t_total;
    unsigned long long device_bytes;  /* workspace owned by the handle */
    double t_matvec;                  /* one near-field mat-vec from the per-step pair list (inside t_lanczos) */
    double t_records;                 /* binning + the 64-byte far-field particle records (t_spread is the spread kernel alone) */
    int lanczos_exchanges;            /* team calls: exchanges the last Brownian call's Lanczos iteration issued (two iterations
                                         per exchange where the decomposition allows: ceil(m / 2) instead of m) */
    int lanczos_status;               /* queue-only Brownian calls (pse_set_async): 0 the step norm passed, 1 the queued iterations ran
                                         out first (the result uses the last size checked: raise the starting count), 2 a
                                         non-finite coefficient or a failed eigen-solve */
    unsigned long long lanczos_open_calls;   /* queue-only calls of this handle so far that ended with lanczos_status != 0 (sticky: a loop
                                                that reads pse_info every hundred steps still learns that one of them ran out) */
} pse_info;

/* -- life cycle: replaces Stokes::Stokes/setParams/~Stokes (PSEv1/Stokes.cc:85-118,129-424) ------------- */
int pse_create(const pse_params *params, pse_handle **out);
int pse_destroy(pse_handle *h);
/* box change under Lees-Edwards shear: what gpu_stokes_SetGridk_kernel re-derives every step
 * (PSEv1/Helper.cu:285-332, called at PSEv1/Stokes.cu:298). Only xy may differ from the creation box by more
 * than round-off unless the cell grid still fits. */
int pse_set_box(pse_handle *h, double Lx, double Ly, double Lz, double xy);
/* run on this hipStream_t (default: the null stream, as the reference does).  The work of every entry point is ordered on
 * this stream.  By default the entry points are not free of host synchronisation: (1) with a neighbour skin in use (the
 * default, below) every evaluation whose kept list may still be valid waits for the stream and reads one flag back before it
 * queues anything (the distance check HOOMD's NeighborList does on the host side too); (2) Brownian calls read the Lanczos
 * scalars back once per convergence check, as the reference does per iteration (PSEv1/Brownian.cu:446-499).
 * pse_set_async(h, 1) (or pse_set_neighbor_skin(h, 0)) removes (1): deterministic evaluations then only queue work. */
int pse_set_stream(pse_handle *h, void *hip_stream);
/* Asynchronous submission (off by default).  With it on, the deterministic entry points (pse_mobility, pse_pair_repulsion) only
 * QUEUE work on the handle's stream and return: nothing is read back, the host never waits, so a call can be captured into a
 * hipGraph by the caller (hipStreamBeginCapture on the handle's stream ... pse_mobility ... hipStreamEndCapture) and replayed
 * with new positions and forces in the same arrays -- tests/test_gpu_async.py does exactly that.  Whether the kept neighbour list
 * is still valid is then decided ON THE DEVICE: a call gathers the particles into the order of the last build, checks every
 * displacement against r_buff / 2, and queues BOTH chains -- sort + cell walk + new list, and the kept-list pass -- whose kernels
 * read the outcome and leave at once if it is not theirs (never a stale list, no round trip; about eight empty launches per
 * call are the price).  Brownian calls (pse_brownian_velocity, pse_step, pse_sqrt_mreal) rebuild the list every time in this mode
 * and take the Lanczos decision ON THE DEVICE too: the iterations of the starting count *lanczos_m are queued, one workgroup
 * computes the tridiagonal square roots and the step norm the reference computes on the host (LAPACKE_spteqr and the loops at
 * PSEv1/Brownian.cu:540-582, 673-724), PSE_LANCZOS_EXTRA (default 2) further iterations follow, each with its own decision
 * and gated on the outcome so far, and the final combination reads m and its coefficients from device memory.  Such a call can be
 * captured and replayed like the deterministic ones; on return *lanczos_m is the m of the most recent call whose outcome has
 * already reached the host (feed it to the next call), pse_get_info after a stream synchronisation gives the m, the step norm
 * and pse_info.lanczos_status of the last completed call (1: the queue ran out before the step norm passed).  Starting counts
 * above 98 minus the gated extras of the call (PSE_LANCZOS_EXTRA, or what pse_set_lanczos_extra set) take the host-checked path.  Per-phase timing (pse_set_timing) synchronises by definition and
 * takes the host-checked path as well.  One warm-up call outside the capture first (kernels set their shared-memory attributes
 * on first use). */
int pse_set_async(pse_handle *h, int enabled);
/* The random numbers of a Brownian call are keyed by (particle or grid node, timestep): a captured call would replay the timestep
 * it was captured with.  With a device word registered here every Brownian call draws its noise at timestep + *device_word,
 * read on the device when the kernels run -- the caller advances the word between replays.  NULL (default): timestep alone. */
int pse_set_timestep_offset(pse_handle *h, const unsigned int *device_word);
/* test hook: the device-side decision of the most recent deterministic evaluation in asynchronous mode (synchronises):
 * 0 the kept list was reused, != 0 it was rebuilt, -1 the call did not take the two-chain path */
int pse_debug_last_gate(pse_handle *h, int *gate);
/* Neighbour list kept across calls: replaces the NeighborListGPUBinned(rcut, r_buff = 0.4) with setEvery(1, dist_check)
 * that PSEv1/integrate.py:60,79 builds and Stokes::integrateStepOne refreshes with m_nlist->compute (PSEv1/Stokes.cc:433).
 * Pairs closer than rcut + r_buff are remembered at a build; later calls with the same N, group and box first check that no
 * particle has moved more than r_buff / 2 since (one flag read back per call) and then skip the cell sort and the cell
 * walk.  Default 0.4 (PSE_SKIN in the environment overrides; 0 = rebuild every call).  r_buff may not exceed the
 * creation value: cells and list capacity are sized for it.  Not kept on slab ranks (multi-GPU) or when rcut + r_buff
 * exceeds half the box.  Results do not depend on it beyond the order of the fp64 pair sums. */
int pse_set_neighbor_skin(pse_handle *h, double r_buff);
/* the r_buff in use and how many calls built / reused the list so far (any pointer may be null) */
int pse_neighbor_stats(pse_handle *h, double *r_buff, unsigned long long *builds, unsigned long long *reuses);
/* per-phase hipEvent timing into pse_info (adds host synchronisation; off by default) */
int pse_set_timing(pse_handle *h, int enabled);
int pse_get_info(pse_handle *h, pse_info *info);
const char *pse_last_error(void);

/* -- the hot path ------------------------------------------------------------------------------------- */
/* U = M.F, deterministic (kT = 0 branch of gpu_stokes_CombinedMobilityBrownian_wrap, PSEv1/Brownian.cu:772-923;
 * the reference's dedicated but uncalled entry is gpu_stokes_Mobility_wrap, PSEv1/Mobility.cu:729-782).
 * group_members (device, may be NULL = identity) lists the N particle indices acted on, exactly like
 * d_group_members / group_size; vel[idx].xyz is written, vel[idx].w is preserved (PSEv1/Mobility.cu:473-475).
 * parts: 1 = real-space (+self) only (gpu_stokes_Mreal_kernel), 2 = wave-space only
 * (gpu_stokes_Mwave_wrap, PSEv1/Mobility.cu:515-575), 3 = both. */
int pse_mobility(pse_handle *h, const pse_double4 *pos, const pse_double4 *force, pse_double4 *vel,
                 const unsigned int *group_members, unsigned int N, int parts);

/* U = M.F + sqrt(2kT/dt) M^{1/2} psi  (PSEv1/Brownian.cu:772-923) without moving the particles.
 * lanczos_m: in = number of Lanczos vectors to start from, out = number used (the reference's int& m_Lanczos). */
int pse_brownian_velocity(pse_handle *h, const pse_double4 *pos, const pse_double4 *force, pse_double4 *vel,
                          const unsigned int *group_members, unsigned int N,
                          double kT, double dt, unsigned int timestep, int *lanczos_m);

/* The two halves of that evaluation on their own -- a FUNCTIONAL split for two GPUs (one GPU the real-space half, the other the
 * wave-space half, each on ALL particles: no slab all-to-all over the one link between them).  parts = 1:
 * M_real.F + sqrt(2kT/dt) M_real^{1/2} psi (the Lanczos half: *lanczos_m as above); parts = 2: M_wave.F + the k-space noise
 * (gpu_stokes_BrownianGridGenerate, PSEv1/Brownian.cu:153-345; *lanczos_m untouched); 3 = pse_brownian_velocity.  The halves of one
 * (kT, dt, timestep, seed) add up to the whole: the caller sums them (an all-reduce between the two ranks) and integrates with
 * pse_integrate -- K15 alone (gpu_stokes_step_one_kernel, PSEv1/Stokes.cu:137-192: pos += (vel + shear_rate y xhat) dt, wrap, accel). */
int pse_brownian_velocity_part(pse_handle *h, const pse_double4 *pos, const pse_double4 *force, pse_double4 *vel,
                               const unsigned int *group_members, unsigned int N, double kT, double dt, unsigned int timestep,
                               int parts, int *lanczos_m);
int pse_integrate(pse_handle *h, pse_double4 *pos, const pse_double4 *vel, pse_double3 *accel, pse_int3 *image,
                  const pse_double4 *net_force, const unsigned int *group_members, unsigned int N, double dt, double shear_rate);

/* One full integration step: the replacement for gpu_stokes_step_one (PSEv1/Stokes.cuh:75-111).
 * Computes vel, then pos += (vel + shear_rate*y*xhat)*dt, wraps into the box updating image, accel = F/mass
 * with mass = vel.w (PSEv1/Stokes.cu:137-192). */
int pse_step(pse_handle *h, pse_double4 *pos, pse_double4 *vel, pse_double3 *accel, pse_int3 *image,
             const pse_double4 *net_force, const unsigned int *group_members, unsigned int N,
             double kT, double dt, unsigned int timestep, double shear_rate, int *lanczos_m);

/* M_real^{1/2} psi by Lanczos alone (gpu_stokes_BrealLanczos_wrap, PSEv1/Brownian.cu:357-765, without the
 * sqrt(2kT/dt) factor): out = M_real^{1/2} psi for a caller-supplied psi. */
int pse_sqrt_mreal(pse_handle *h, const pse_double4 *pos, const pse_double4 *psi, pse_double4 *out,
                   const unsigned int *group_members, unsigned int N, double tol, int *lanczos_m);

/* The random vectors the Brownian step draws (for parity tests against the oracle's Philox stream):
 * psi[idx].xyz = particle noise (gpu_stokes_BrownianGenerate_kernel, PSEv1/Brownian.cu:99-130). */
int pse_random_psi(pse_handle *h, pse_double4 *psi, const unsigned int *group_members, unsigned int N,
                   unsigned int timestep);

/* -- introspection used by the parity tests ------------------------------------------------------------ */
/* evaluate the device's real-space functions f(r), g(r) (the replacement of the m_ewaldC1 table,
 * PSEv1/Stokes.cc:334-422) at n host radii -> host arrays.  Accuracy: the table is degree 9 on intervals of width 1/8, and what that
 * format costs depends on xi (tests/realspace_ref.py format_eps, from the closed forms alone): below 3e-15 for xi <= 2, 7e-15 at 3,
 * 6.6e-14 at 4 -- the contract |f - f_ref|, |g - g_ref| < 2e-13 holds up to XI_TABLE = 4 -- then 4.9e-13 at xi = 6, 2.1e-10 at 10,
 * 2e-8 at 20 (larger xi is admitted, at that accuracy).  PSE_ERR_INVALID for an r outside (0, (ceil(8 rcut) + 1) / 8 (1 - 2^-50)): the
 * kernel looks up r^2 rsqrt(r^2), which may exceed r in its last bits, and no interval lies behind the last one. */
int pse_eval_realspace(pse_handle *h, const double *r_host, int n, double *f_host, double *g_host);
/* Force provider next to the path (the step consumes net_force from its host, PSEv1/Stokes.cc:447, and the
 * reference's example has none): soft repulsion F_i = sum_j k (sigma - r)(r_i - r_j)/r over minimum-image pairs with
 * r < sigma <= rcut, evaluated from the engine's cell list.  force[group[i]].xyz is overwritten (accumulate = 0) or
 * incremented (accumulate = 1); w is kept. */
int pse_pair_repulsion(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *group, unsigned N,
                       double k, double sigma, int accumulate);
/* The same pass with the pair observables a rheology run samples (no reference counterpart: the reference leaves forces, and with them
 * their stress, to HOOMD): out8 (DEVICE, 8 doubles) = U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, npairs of the pairs with r < sigma among the N
 * group members, each unordered pair once.  U = sum k/2 (sigma - r)^2;  W_ab = sum_{i<j} d_a F_b with d = r_i - r_j (minimum image) and
 * F = k (sigma - r) d / r the force ON i FROM j -- symmetric (central force), positive on the diagonal for a repulsion; the particle
 * stress is sigma_ab = -W_ab / V with V = Lx Ly Lz, and dU/d(strain xy) = -Wxy.  npairs counts 1.0 per pair.  force as in
 * pse_pair_repulsion, or NULL: observables only.  The sums use no atomics and the cell sort is stable: equal inputs give the same
 * eight doubles bit for bit.  The call only queues work on the handle's stream wherever pse_pair_repulsion does and reads nothing
 * back; out8 may point into a larger device array (row r of a log that is read once at the end of a run).  Single-GPU handles only:
 * a slab rank (n_slabs >= 2) orders only its own cells, its sums would be partial -- PSE_ERR_INVALID. */
int pse_pair_repulsion_virial(pse_handle *h, const pse_double4 *pos, pse_double4 *force /* may be NULL */,
                              const unsigned *group, unsigned N, double k, double sigma, int accumulate, double *out8);
/* A tabulated central pair potential on the same cell list, the counterpart of HOOMD's pair.table for the one particle type of this
 * engine (no reference counterpart: the reference leaves forces to HOOMD).  table (DEVICE, width x 2 doubles, 16-byte aligned) holds
 * V_k, F_k interleaved at the nodes r_k = rmin + k dr, dr = (rmax - rmin)/(width - 1): V_k the pair energy, F_k the magnitude of the
 * radial force, positive for a repulsion.  Between the nodes both are linear: t = (r - rmin)(width - 1)/(rmax - rmin),
 * k = min(floor(t), width - 2), w = t - k, V(r) = V_k + w (V_k+1 - V_k), F(r) likewise.  The pass acts on the minimum-image pairs among
 * the N group members with rmin <= r < rmax and r > 0; a pair outside that interval contributes nothing (no extrapolation, as in
 * HOOMD's table).  The force ON i FROM j is F(r) d / r, d = r_i - r_j.  force is overwritten (accumulate = 0) or incremented
 * (accumulate = 1) as in pse_pair_repulsion, w is kept; force = NULL: observables only.  out8 (DEVICE, 8 doubles, or NULL) = U, Wxx,
 * Wxy, Wxz, Wyy, Wyz, Wzz, npairs with the meaning and signs of pse_pair_repulsion_virial: U = sum V(r), W_ab = sum_{i<j} d_a F_b,
 * each unordered pair once, stress = -W / V, no atomics, bit-reproducible on equal inputs.  out8 = NULL: forces only, and the
 * reduction is not run.  PSE_ERR_INVALID: pos or table null, force and out8 both null, width outside [2, 2048] (the table is staged
 * in 32 KB of LDS per workgroup), rmin or rmax not finite, rmin < 0, rmax <= rmin, rmax > rcut (the cell list is built for the
 * hydrodynamic cutoff), a table that is not 16-byte aligned, out8 on a slab rank (n_slabs >= 2: its sums would be partial).  The
 * call only queues work on the handle's stream wherever pse_pair_repulsion does and reads nothing back: the table is read by the
 * stream, the caller keeps it alive and unchanged until the stream has passed the call.  Particles of several types, with one
 * table per pair of types: pse_pair_table_typed below. */
int pse_pair_table(pse_handle *h, const pse_double4 *pos, pse_double4 *force /* may be NULL */, const unsigned *group, unsigned N,
                   const double *table /* DEVICE, width x 2: V_k, F_k interleaved */, int width, double rmin, double rmax,
                   int accumulate, double *out8 /* DEVICE, may be NULL */);

/* ---- pair exclusions: HOOMD's nlist.reset_exclusions (no reference counterpart: the reference leaves forces to HOOMD) ----
 * In HOOMD the neighbour list drops bonded pairs from the pair potentials by default (nlist.reset_exclusions(['bond']), optionally
 * 'angle' and 'dihedral'): force fields are fitted with that understanding.  A pse_exclusions object is such a SET of npairs particle
 * pairs, and the two passes below are pse_pair_table and pse_pair_repulsion with the pairs of the set contributing nothing -- not to
 * the forces, not to U or W, not to npairs.  The indices are CALLER-order particle indices: rows of pos and force, the values of
 * `group` -- not positions in the group, not rows of the engine's sorted order.  A particle whose index is >= the object's n has no
 * exclusions.  A pair may be listed more than once and in either order: it is one exclusion (a set, unlike a bond list).  Which
 * pairs to put in it is the caller's choice: HOOMD's sets are both members of a bond, the two ends of an angle, the two ends of a
 * dihedral.  Scaled 1-4 interactions ("special pairs") are not provided, and neither the hydrodynamic near field nor the kept
 * neighbour list knows exclusions: the mobility acts between all particles.
 * The object is stored as one sorted row of partners per particle, every pair in both rows (pse_host_exclusion_rows): results are
 * bit-identical for any order of the list and either order of a pair's members.  It belongs to its handle: pse_destroy frees the
 * objects still alive, pse_exclusions_destroy after that is a caller error.
 * pse_exclusions_create returns PSE_ERR_INVALID, with a message naming the value, for: a null h, pairs_host or out, n == 0 or
 * n > n_max, npairs == 0 or npairs > 2^30, an index >= n, a pair with i == j.  *out is null after a refusal. */
typedef struct pse_exclusions pse_exclusions;
int pse_exclusions_create(pse_handle *h, unsigned n, unsigned npairs, const unsigned *pairs_host /* npairs x 2 particle indices */,
                          pse_exclusions **out);
int pse_exclusions_destroy(pse_exclusions *ex);
/* pse_pair_table with the pairs of ex excluded.  Arguments, results, refusals and their order are those of pse_pair_table (its
 * checks run first); in addition PSE_ERR_INVALID for a null ex and for an ex created on another handle.  The kept pairs are summed
 * in the order of pse_pair_table: with an object none of whose pairs is in range, forces and out8 equal pse_pair_table's bit for
 * bit.  Queue-only wherever pse_pair_table is, no atomics, bit-reproducible; ex must stay alive until the stream has passed the call
 * (pse_exclusions_destroy waits for the stream). */
int pse_pair_table_excl(pse_handle *h, const pse_double4 *pos, pse_double4 *force /* may be NULL */, const unsigned *group, unsigned N,
                        const double *table /* DEVICE, width x 2: V_k, F_k interleaved */, int width, double rmin, double rmax,
                        int accumulate, double *out8 /* DEVICE, may be NULL */, const pse_exclusions *ex);
/* The harmonic repulsion with the pairs of ex excluded: out8 == NULL is pse_pair_repulsion (force is required), out8 != NULL is
 * pse_pair_repulsion_virial (force may be NULL, refused on a slab rank); the checks of the one or the other run first, then those of
 * ex as above.  Summation order, reproducibility and queueing as for pse_pair_table_excl. */
int pse_pair_repulsion_excl(pse_handle *h, const pse_double4 *pos, pse_double4 *force, const unsigned *group, unsigned N,
                            double k, double sigma, int accumulate, double *out8 /* DEVICE, may be NULL */, const pse_exclusions *ex);

/* ---- typed pair tables: HOOMD's pair.table with pair_coeff.set('A', 'B', ...) (no reference counterpart: the reference leaves forces to HOOMD) ----
 * Equal-radius beads that differ only in how they interact -- the blocks of a copolymer, sticky end groups, a binary mixture: every
 * particle has one of ntypes <= 8 types, and every unordered pair of types its own table.  The hydrodynamics knows no types.
 * Pair types: npt = ntypes (ntypes + 1)/2 of them; the pair of types a <= b has the index p(a, b) = a ntypes - a (a - 1)/2 + (b - a),
 * the upper triangle row by row: AA, AB, AC, ..., BB, BC, ...; a pair of particles with types (b, a) uses p(a, b).
 * Tables: pair type p has width_host[p] nodes between rmin_host[p] and rmax_host[p], with exactly the meaning of pse_pair_table: V and
 * F linear between the nodes, acting on rmin <= r, r^2 < rmax^2, r > 0, no extrapolation.  tables_host holds the (V_k, F_k) entries
 * of the pair types one after another in the order of p, sum(width) x 2 doubles.  width_host[p] == 0 switches pair type p off: it
 * contributes nothing, its rmin and rmax are ignored, it takes no room in tables_host.  All tables together are staged in LDS by every
 * workgroup: sum(width) <= 3584 entries = 56 KB, which with the kernel's 1.4 KB of static LDS stays inside the 64 KB a workgroup gets
 * without raising a limit (pse_host_typed_table_layout is the one place that computes where each table lies).
 * Types: types_host[t] is the type of CALLER-order particle t -- a row of pos and force, a value of `group` -- not of a position in the
 * group or of a row of the engine's sorted order.  A particle whose index is >= the object's n acts as type 0.
 * The object belongs to its handle: pse_destroy frees the objects still alive, pse_typed_table_destroy after that is a caller error;
 * pse_typed_table_destroy waits for the stream.  Everything is copied at creation: the host arrays may go afterwards.
 * pse_typed_table_create returns PSE_ERR_INVALID, with a message naming the value, for: a null argument, n == 0 or n > n_max, ntypes
 * outside [1, 8], a type >= ntypes, a width of 1, a negative width or a width > 2048, all widths zero, a sum of widths > 3584, and for
 * a pair type that is on: rmin or rmax not finite, rmin < 0, rmax <= rmin, rmax > rcut, a table entry that is not finite.  *out is
 * null after a refusal. */
typedef struct pse_typed_table pse_typed_table;
int pse_typed_table_create(pse_handle *h, unsigned n, const unsigned *types_host /* n: type of caller-order row t */, int ntypes,
                           const int *width_host, const double *rmin_host, const double *rmax_host /* npt each */,
                           const double *tables_host /* sum(width) x 2: V_k, F_k, the pair types' tables one after another */,
                           pse_typed_table **out);
int pse_typed_table_destroy(pse_typed_table *t);
/* The pass of pse_pair_table_excl on the handle of t with, for every pair, the table and the range of its pair type.  force,
 * accumulate, w, out8 (meaning and signs of its eight numbers), group and N as there; ex == NULL: nothing is excluded, otherwise the
 * pairs of ex contribute nothing.  No floating-point atomics, every sum in the engine's sorted order: bit-reproducible on equal
 * inputs, and unchanged bit for bit when two types swap their labels together with their tables.  Against pse_pair_table with the one
 * table for all pair types the results agree to rounding, not bit for bit (another kernel).  Queue-only wherever pse_pair_table is:
 * t (and ex) must stay alive until the stream has passed the call.  PSE_ERR_INVALID, in this order: a null t, N == 0 or N > n_max,
 * a null pos, force and out8 both null, out8 on a slab rank, an ex created on another handle than t. */
int pse_pair_table_typed(pse_typed_table *t, const pse_double4 *pos, pse_double4 *force /* may be NULL */, const unsigned *group,
                         unsigned N, int accumulate, double *out8 /* DEVICE, may be NULL */, const pse_exclusions *ex /* may be NULL */);

/* ---- pair-distance histograms: the counts behind g(r), the partial g_ab(r) and coordination numbers (no reference counterpart) ----
 * A pse_pair_hist object fixes the types of the particles and the bins: every particle has one of ntypes <= 8 types (types_host[t]: the
 * type of CALLER-order particle t, as for pse_typed_table_create; NULL: all of type 0; a
 * particle whose index is >= n acts as type 0), and every pair type p(a, b) = a ntypes - a (a - 1)/2 + (b - a), a <= b, of the
 * npt = ntypes (ntypes + 1)/2 has one row of nbins uniform bins on [rmin, rmax), shared by all pair types.
 * pse_pair_hist_accumulate walks the handle's cell list once: every unordered minimum-image pair among the N group members with
 * rmin <= r, r^2 < rmax^2, r > 0 that is not in ex adds 1 to counts[p nbins + b], b = min((int)((r - rmin) nbins/(rmax - rmin)),
 * nbins - 1) -- bin b covers [rmin + b w, rmin + (b + 1) w), w = (rmax - rmin)/nbins.  counts (DEVICE, npt x nbins unsigned 64-bit words,
 * 8-byte aligned) is ADDED to: the caller zeroes it once and accumulates as many samples as it likes; nothing is read back and the
 * host never waits (queue-only wherever pse_pair_table is).  Only integers are summed (32-bit counters in LDS per workgroup, 64-bit
 * atomics into counts): the result is exact, independent of the order of the particles and of the launch, and bit-reproducible.
 * From the counts of S samples: g_ab(r_b) = counts / (S P_ab V_shell / V) with P_aa = N_a (N_a - 1)/2, P_ab = N_a N_b,
 * V_shell = 4 pi/3 (r_hi^3 - r_lo^3), V = Lx Ly Lz (pse_amd.analyze.RDF does this).
 * npt x nbins <= 8192 (32 KB of LDS).  rmax may not exceed rcut: the cell list is built for the hydrodynamic cutoff.  A slab rank
 * (n_slabs >= 2) orders only its own cells, its counts would be partial: refused.
 * The object belongs to its handle: pse_destroy frees the objects still alive, pse_pair_hist_destroy after that is a caller error;
 * pse_pair_hist_destroy waits for the stream.  The types are copied at creation.
 * pse_pair_hist_create returns PSE_ERR_INVALID, with a message naming the value, for, in this order: a null out or h, n == 0 or
 * n > n_max, ntypes outside [1, 8], nbins < 1, npt x nbins > 8192, rmin or rmax not finite, rmin < 0, rmax <= rmin, rmax > rcut, a slab
 * rank, a type >= ntypes.  *out is null after a refusal.  pse_pair_hist_accumulate, in this order: a null g, N == 0 or N > n_max, a
 * null pos, a null counts or one that is not 8-byte aligned, an ex created on another handle than g; counts is untouched then. */
typedef struct pse_pair_hist pse_pair_hist;
int pse_pair_hist_create(pse_handle *h, unsigned n, const unsigned *types_host /* n, or NULL: one type */, int ntypes, int nbins,
                         double rmin, double rmax, pse_pair_hist **out);
int pse_pair_hist_destroy(pse_pair_hist *g);
int pse_pair_hist_accumulate(pse_pair_hist *g, const pse_double4 *pos, const unsigned *group, unsigned N,
                             unsigned long long *counts /* DEVICE, npt x nbins, ADDED to */, const pse_exclusions *ex /* may be NULL */);

/* ---- static structure factors: the densities rho_a(k) on the box's reciprocal lattice and their products S_ab(k) (no reference counterpart) ----
 * A pse_structure_factor object fixes the types of the particles (types_host, ntypes <= 8, exactly as for pse_pair_hist_create:
 * CALLER-order, NULL: all of type 0, a particle whose index is >= n acts as type 0) and a list of nk integer triples m = (mx, my, mz),
 * |m_i| <= PSE_SF_MAX_INDEX, nk <= PSE_SF_MAX_MODES.  (0, 0, 0), a mode and its negative, and duplicates are allowed
 * (a mode listed twice is computed once: equal bits in both places).
 * With the handle's CURRENT box (Lx, Ly, Lz, xy) -- whatever pse_set_box last set -- and the fractional coordinates s_x = (x - xy y)/Lx,
 * s_y = y/Ly, s_z = z/Lz (not shifted, not wrapped), pse_structure_factor_accumulate computes, over the N group members j,
 *   rho_a(m) = sum_{type(j) = a} exp(-2 pi i (mx s_x + my s_y + mz s_z)),
 * the density of type a at k = 2 pi (mx/Lx, my/Ly - xy mx/Lx, mz/Lz).  A particle moved by any lattice vector, the tilted
 * (xy Ly, Ly, 0) included, gives the same rho.  The phase is reduced exactly before it is evaluated (every product m_i s_i loses its
 * integer part in one fused operation, the sum its own, then sincospi): no sine or cosine of a large argument is taken, and the error
 * of one term is that of s itself -- two roundings in s_x, one in s_y and s_z, times 2 pi |m_i| -- plus a few 1e-16.
 * rho (DEVICE, ntypes x nk x 2 doubles, (re, im) interleaved, or NULL) is OVERWRITTEN; sums (DEVICE, npt x nk doubles, or NULL) is ADDED
 * to: sums[p nk + q] += Re(rho_a(m_q) conj rho_b(m_q)) for the pair type p(a, b) = a ntypes - a (a - 1)/2 + (b - a), a <= b, of the
 * npt = ntypes (ntypes + 1)/2, with the rho of this call: the caller zeroes it once and accumulates as many samples as it likes,
 * S_ab(k) = sums / (samples sqrt(N_a N_b)) (pse_amd.analyze.StructureFactor does this).  Both are in the caller's order of the modes.
 * A type without particles has rho exactly 0, and (0, 0, 0) gives rho_a = N_a exactly.
 * No floating-point atomics: every sum has a fixed order, equal inputs give equal bits.  The distinct modes are sorted at creation (mx, then
 * my, then mz) and cut into arithmetic progressions m0 + t d of at most 8 modes, each seeded from the exactly reduced phase and
 * continued by one complex multiplication per mode: the value of a mode is a function of the mode SET, not of the order of the list,
 * and a permuted list gives the same bits, permuted.  A permuted particle order changes the order of the sums: equal to rounding.
 * The call only queues work on the handle's stream and reads nothing back.  It does not sort and does not touch the cell list, the
 * kept neighbour list or its counters, and it works on a slab rank's handle (n_slabs >= 2: positions are replicated there, the sums
 * are complete), as the bonded passes do.
 * The object belongs to its handle: pse_destroy frees the objects still alive, pse_structure_factor_destroy after that is a caller
 * error; pse_structure_factor_destroy waits for the stream.  Types and modes are copied at creation, and the object holds the
 * workspace of the partial sums, sized from n_max, ntypes and nk (at most 256 MB).
 * pse_structure_factor_create returns PSE_ERR_INVALID, with a message naming the value, for, in this order: a null out or h, n == 0
 * or n > n_max, ntypes outside [1, 8], nk == 0 or nk > 32768, a null modes_host, an index beyond +-4096, a type >= ntypes.  *out is
 * null after a refusal.  pse_structure_factor_accumulate, in this order: a null f, N == 0 or N > n_max, a null pos, rho and sums both
 * null, either of them not 8-byte aligned; nothing is launched and nothing is written then. */
#define PSE_SF_MAX_INDEX 4096    /* |mx|, |my|, |mz| */
#define PSE_SF_MAX_MODES 32768   /* nk */
typedef struct pse_structure_factor pse_structure_factor;
int pse_structure_factor_create(pse_handle *h, unsigned n, const unsigned *types_host /* n, or NULL: one type */, int ntypes,
                                unsigned nk, const int *modes_host /* nk x 3 */, pse_structure_factor **out);
int pse_structure_factor_destroy(pse_structure_factor *f);
int pse_structure_factor_accumulate(pse_structure_factor *f, const pse_double4 *pos, const unsigned *group, unsigned N,
                                    double *rho  /* DEVICE, ntypes x nk x 2 (re, im), OVERWRITTEN, may be NULL */,
                                    double *sums /* DEVICE, npt x nk, ADDED to, may be NULL */);

/* ---- displacement moments: the drift, the mean-squared displacement tensor and the fourth moment per type, against up to 64 time origins (no reference counterpart) ----
 * A pse_msd object fixes the types of the particles (types_host, ntypes <= 8, exactly as for pse_pair_hist_create: CALLER-order, NULL:
 * all of type 0, a particle whose index is >= n acts as type 0; copied at creation) and holds norigins <= PSE_MSD_MAX_ORIGINS slots of
 * n_max UNWRAPPED positions in fp64, three planes (x, y, z) of n_max doubles per slot, zeroed at creation, indexed by the caller-order
 * particle index.  The unwrapped position of a particle at (x, y, z) with image (ix, iy, iz) in the box (Lx, Ly, Lz) is
 *   x_u = x + ix Lx + iy (strain Ly),   y_u = y + iy Ly,   z_u = z + iz Lz,
 * where `strain` is the ACCUMULATED tilt: the current xy plus the whole lattice vectors that Lees-Edwards flips have removed so far
 * (pse_amd.system.System.strain).  It stands where xy would: position + image . box with the current xy jumps by iy Lx at every flip;
 * r_u with the strain is the same point before and after a flip and through every re-wrap of x behind a changed tilt, every x and z
 * wrap of pse_integrate and every y wrap BEFORE the first flip.  LIMIT: it is NOT continuous through a y image gained after a flip --
 * the wrap of pse_integrate takes xy Ly, the CURRENT tilt, off x, the formula adds strain Ly, so x_u shifts by flips Ly per such
 * image.  y_u and z_u are always right: the moments without x (dy, dz, dy^2, dz^2, dy dz) hold for any run; those with x (dx, dx^2,
 * dx dy, dx dz, |d|^4) and the x of pse_msd_displacement hold for a sheared run only while no particle gains a y image after a flip.
 * Lx, Ly, Lz are the handle's CURRENT box lengths (pse_set_box); its xy is not used.  sLy = strain Ly is formed once on the host, in
 * double; the device evaluates x_u = fma(iy, sLy, fma(ix, Lx, x)), y_u = fma(iy, Ly, y), z_u = fma(iz, Lz, z): two roundings in x_u,
 * one in y_u and z_u.
 * pse_msd_store writes r_u of the N group members into `slot` and marks the slot stored (host bookkeeping: no device wait).
 * pse_msd_accumulate computes r_u(now) of every group member once and, for every listed pair q = (slots_host[q], rows_host[q]) and
 * every type a, with d = r_u(now) - r_u(slot),
 *   sums[(rows_host[q] ntypes + a) PSE_MSD_MOMENTS + c] += sum over the members of type a of moment_c(d),
 * c = 0..2: dx, dy, dz;  3..8: dx^2, dy^2, dz^2, dx dy, dx dz, dy dz;  9: (dx^2 + dy^2 + dz^2)^2.  A type without members adds exactly
 * +0.0; rows of sums that no pair names are not touched.  The two host lists (at most 64 pairs) travel by value as a kernel argument:
 * no copy, no wait.  The caller must use the same group for the store and the accumulate of one slot (documented, not checked).
 * pse_msd_displacement writes, for every group member t, out[t] = (d.x, d.y, d.z, |d|^2) against `slot`; rows outside the group are
 * not touched.
 * No floating-point atomics: a wave owns 256 consecutive group members, four per lane; a lane adds the moments of its particles in
 * registers, the wave adds the lanes' sums with a fixed halving tree and writes one row per listed pair and type into a workspace the
 * object owns (sized for 64 pairs, whatever norigins is: a slot may be listed for several rows); a finishing kernel adds the rows of
 * the waves in a fixed interleaved order and then adds to sums: equal inputs give equal bits.  All calls only queue work on the handle's stream and read nothing back.  They do
 * not sort and do not touch the cell list, the kept neighbour list or its counters, and they work on a slab rank's handle
 * (n_slabs >= 2: positions are replicated there, the sums are complete).
 * The object belongs to its handle: pse_destroy frees the objects still alive, pse_msd_destroy after that is a caller error;
 * pse_msd_destroy waits for the stream.  A failed allocation returns PSE_ERR_HIP, frees what it took and leaves *out null.
 * PSE_ERR_INVALID, with a message naming the value, nothing launched, nothing written: pse_msd_create, in this order: a null out or
 * h, n == 0 or n > n_max, ntypes outside [1, 8], norigins outside [1, 64], a type >= ntypes (*out is null after a refusal).
 * pse_msd_store and pse_msd_displacement, in this order: a null m, slot outside [0, norigins), N == 0 or N > n_max, a null pos, a null
 * image, a strain that is not finite; pse_msd_displacement then: a slot never stored, a null out or one that is not 8-byte aligned.
 * pse_msd_accumulate, in this order: a null m, N == 0 or N > n_max, a null pos, a null image, a strain that is not finite, npairs
 * outside [1, 64], a null slots_host or rows_host, nrows < 1, a slot out of range, a slot never stored, a row outside [0, nrows), a
 * row listed twice in this call (the finishing pass would race), a null sums or one that is not 8-byte aligned. */
#define PSE_MSD_MAX_ORIGINS 64
#define PSE_MSD_MOMENTS     10
typedef struct pse_msd pse_msd;
int pse_msd_create(pse_handle *h, unsigned n, const unsigned *types_host /* n, or NULL: one type */, int ntypes, int norigins, pse_msd **out);
int pse_msd_destroy(pse_msd *m);
int pse_msd_store(pse_msd *m, int slot, const pse_double4 *pos, const pse_int3 *image, const unsigned *group, unsigned N, double strain);
int pse_msd_accumulate(pse_msd *m, const pse_double4 *pos, const pse_int3 *image, const unsigned *group, unsigned N, double strain,
                       int npairs, const int *slots_host, const int *rows_host, int nrows,
                       double *sums /* DEVICE, nrows x ntypes x 10, ADDED to */);
int pse_msd_displacement(pse_msd *m, int slot, const pse_double4 *pos, const pse_int3 *image, const unsigned *group, unsigned N, double strain,
                         pse_double4 *out /* DEVICE, caller order: d.xyz, |d|^2 in w; rows outside the group untouched */);

/* ---- intermediate scattering functions: the self part F_s(k, t) and the collective part F(k, t) against up to 64 time origins (no reference counterpart) ----
 * A pse_isf object fixes the types of the particles and a list of nk <= PSE_ISF_MAX_MODES integer modes exactly as a
 * pse_structure_factor does (types_host, ntypes <= 8, |m_i| <= PSE_SF_MAX_INDEX; (0, 0, 0), a mode with its negative and duplicates are
 * allowed) and holds a CURRENT BUFFER and norigins <= PSE_ISF_MAX_ORIGINS slots of the same shape: three planes of n_max doubles with
 * the fractional coordinates s of a sample, indexed by the caller-order particle index, and the densities rho of that sample.
 * Conventions are those of pse_structure_factor_accumulate: in the handle's CURRENT box, s_x = fma(-xy, y, x) / Lx (two roundings), s_y =
 * y / Ly, s_z = z / Lz (one each), not shifted, not wrapped; rho_a(m) = sum_{type(j) = a} exp(-2 pi i m.s_j).
 * pse_isf_sample fills the current buffer from the N group members: s of every member, and rho of the sample by the pass of
 * pse_structure_factor_accumulate itself -- the rho it writes (ntypes x nk x 2, (re, im), or NULL) and what it ADDS to static_sums
 * (npt x nk, or NULL) are the bits of that call on the same inputs.  It remembers N and the group pointer for pse_isf_correlate.  Every
 * sample of one object must use the same group (documented; N is checked).
 * pse_isf_store copies the current buffer into origin slot `slot` (a device-to-device copy on the handle's stream) and marks the slot
 * stored with the N of the sample (host bookkeeping, as pse_msd_store).
 * pse_isf_correlate, for every listed pair (slot, row), types a and b and mode q, with the current buffer as `now`:
 *   self[((row ntypes + a) nk + q) 2 + {0, 1}] += sum over the members j of type a of (re, im) exp(-2 pi i m_q.(s_j(now) - s_j(slot)))
 *   coll[((row ntypes + a) ntypes + b) nk + q] += Re(rho_a(m_q; now) conj rho_b(m_q; slot))
 * F_s = Re self / (origins N_a) and F_ab = coll / (origins sqrt(N_a N_b)) (pse_amd.analyze.IntermediateScattering does this).  The phase
 * of the self part uses fractional coordinates and integer modes: it needs NO images and NO unwrapping -- a particle that wrapped by any
 * lattice vector between the origin and now gives the same value.  In a tilting box the integer mode is the ADVECTED wave vector k(t)
 * = 2 pi (mx/Lx, my/Ly - xy(t) mx/Lx, mz/Lz): purely affine motion leaves self = N_a, the usual choice under shear.  A Lees-Edwards
 * flip relabels the modes (s_x changes by a multiple of s_y): slots stored before a flip must not be correlated with samples after
 * it -- the caller's rule, not checked here.  The collective block is ORDERED: a is the type now, b the type at the origin, all
 * ntypes^2 blocks are kept, because under shear <rho_a(t) rho_b*(0)> != <rho_b(t) rho_a*(0)> (as the nine entries of
 * PSE_CHAIN_MODES_CORR).  At most 64 pairs, by value in the launch: no copy, no wait.  A slot may be listed for several rows; rows that
 * no pair names are not touched.  A type without members adds exactly +0.0; (0, 0, 0) gives self = (N_a, 0) and coll = N_a N_b
 * exactly; a mode listed twice is computed once and has the same bits in every place.
 *   ORDER OF THE SUMS.  Self part, per particle: ds_c = s_c(now) - s_c(slot), one subtraction per component; the distinct modes in the
 *   segments of the structure-factor plan (arithmetic progressions m0 + t d of at most 8 modes); f_c = fma(m_c, ds_c, -rint(m_c ds_c))
 *   -- the integer part goes exactly --, t = (f_x + f_y) + f_z, t -= rint(t), sincospi(-2 t) for m0 and for d, then one complex
 *   multiplication per further mode of the segment: no sine or cosine of a large argument is taken.  Per (pair, type, mode): the group
 *   members in spans of `span` consecutive positions of the group (span: a multiple of 256 fixed at creation from n_max, ntypes, nk),
 *   within a span in ascending order from +0.0 by one lane; across the spans lane l of 64 adds the spans l, l + 64, ... in ascending
 *   order from +0.0, then the xor butterfly (every lane adds the lane l xor o for o = 32, 16, ..., 1); then the one addition to self.
 *   The value of a mode is a function of the mode SET, not of the order of the list.  Collective part: re_a re_b + im_a im_b (the
 *   compiler may fuse one product), then the one addition to coll.  No floating-point atomics anywhere: equal inputs give equal bits.
 * Everything is allocated at creation: the plan, the workspace of the structure-factor pass, the current buffer, norigins slots (3 n_max
 * + 2 ntypes nk doubles each) and the workspace of the self part, one complex number per (span, pair, type, mode) for 64 pairs, at
 * most 256 MB (which is why nk <= 4096 here).  A failed allocation returns PSE_ERR_HIP, frees what it took and leaves *out null.  The
 * device calls only queue work on the handle's stream and read nothing back; they can be captured in a graph.  They use no sort, no
 * cell list and no kept neighbour list, and they work on a slab rank's handle (positions are replicated there).  The object belongs to
 * its handle exactly as a pse_msd does: pse_destroy frees the objects still alive, pse_isf_destroy waits for the stream.
 * OUT OF SCOPE: owned-particle ranks (local_rows), multi-tau lag schemes, the van Hove function in real space, re-labelling origins
 * through a flip, wave vectors off the reciprocal lattice.
 * PSE_ERR_INVALID, with a message naming the value, nothing launched, nothing written: pse_isf_create, in this order: everything
 * pse_structure_factor_create refuses, in its order, with nk > 4096 in place of nk > 32768, then norigins outside [1, 64] (*out is
 * null after a refusal).  pse_isf_sample, in this order: a null f, N == 0 or N > n_max, a null pos, rho or static_sums not 8-byte
 * aligned.  pse_isf_store: a null f, slot outside [0, norigins), no sample since create.  pse_isf_correlate, in this order: a null f,
 * no sample since create, npairs outside [1, 64], a null slots_host, a null rows_host, nrows < 1, in the order of the list a slot
 * outside [0, norigins), then a slot never stored, then a slot stored with another N than the current sample's, then a row outside
 * [0, nrows), then a row listed twice, then self and coll both null, then either not 8-byte aligned. */
#define PSE_ISF_MAX_ORIGINS 64
#define PSE_ISF_MAX_MODES   4096      /* |m_i| <= PSE_SF_MAX_INDEX as for the structure factor */
typedef struct pse_isf pse_isf;
int pse_isf_create(pse_handle *h, unsigned n, const unsigned *types_host /* n, or NULL: one type */, int ntypes, unsigned nk,
                   const int *modes_host /* nk x 3 */, int norigins, pse_isf **out);
int pse_isf_destroy(pse_isf *f);
int pse_isf_sample(pse_isf *f, const pse_double4 *pos, const unsigned *group, unsigned N,
                   double *rho         /* DEVICE, ntypes x nk x 2 (re, im), WRITTEN, may be NULL */,
                   double *static_sums /* DEVICE, npt x nk, ADDED to, may be NULL */);
int pse_isf_store(pse_isf *f, int slot);
int pse_isf_correlate(pse_isf *f, int npairs, const int *slots_host, const int *rows_host, int nrows,
                      double *self /* DEVICE, nrows x ntypes x nk x 2, ADDED to, may be NULL */,
                      double *coll /* DEVICE, nrows x ntypes x ntypes x nk, ADDED to, may be NULL */);

/* ---- cluster analysis: the connected components of a distance criterion (no reference counterpart) ----
 * A pse_clusters object fixes the types of the particles and the link distances: types_host, ntypes <= 8 and the pair types
 * p(a, b) exactly as for pse_pair_hist_create (NULL: one type; a caller index >= n acts as type 0); rlink_host holds one link
 * distance per pair type, npt = ntypes (ntypes + 1)/2 of them in that order: 0 switches a pair type off, every other entry must be
 * finite, > 0 and <= rcut (the cell list is built for the hydrodynamic cutoff), and at least one must be on.
 * pse_clusters_label: two of the N group members are LINKED when their minimum-image distance has 0 < r^2 < rlink[p]^2 and the pair
 * is not in ex; a cluster is a connected component of the links.  All outputs are DEVICE arrays, each may be NULL but not all:
 *   label[t]  (unsigned, by CALLER index) the smallest caller index in t's cluster: a member of it, independent of the sort and of
 *             the order of the launch; entries of indices outside the group are left alone
 *   size[t]   (unsigned, by caller index) the number of members of t's cluster
 *   stats     four unsigned 64-bit words, 8-byte aligned, OVERWRITTEN: the number of clusters, the size of the largest, the sum of
 *             s^2 over the clusters, N
 *   hist      nhist >= 1 unsigned 64-bit words, 8-byte aligned, ADDED to: every cluster of size s adds 1 to hist[min(s, nhist) - 1]
 *             (the last word counts every cluster of nhist members or more); samples accumulate on the device
 * Queue-only wherever pse_pair_hist_accumulate is: the sort, the type mirror and a fixed sequence of five launches (a union-find over
 * the sorted rows), nothing is read back, no lane waits for another, only integers are summed: equal inputs give equal bits and a
 * permuted particle order gives the same partition.  The loops of the union-find are proven to end; each nevertheless
 * carries a trip cap of N, and a lane that reaches it sets a bit of the object's sticky status word: that call then writes label = ~0u
 * and size = 0 everywhere.  pse_clusters_status waits for the stream and returns the word (0: every call so far was complete); once it
 * has returned a non-zero word, pse_clusters_label refuses.  Until the host has read the word, later calls are still queued and,
 * the word being sticky on the device, write ~0u labels too: a caller that meets a ~0u label asks pse_clusters_status.
 * Whether a cluster is connected to its own periodic image (percolation), the clusters made whole across the boundaries and their
 * radii of gyration: pse_clusters_span below.  Not computed: the centre of mass and the gyration tensor per cluster (the unfolded
 * positions give the host what it needs); links longer than the real-space cutoff.  A slab rank (n_slabs >= 2) orders only its own cells: pse_clusters_label refuses
 * it; teams and owned-particle steps have no cluster entry point.
 * The object belongs to its handle as a pse_pair_hist does (pse_destroy frees it; pse_clusters_destroy waits for the stream).
 * PSE_ERR_INVALID, with a message naming the value, nothing launched, nothing written: pse_clusters_create, in this order: a null out
 * or h, n == 0 or n > n_max, ntypes outside [1, 8], a null rlink_host, an entry that is not finite, negative or > rcut, no entry on, a
 * type >= ntypes (*out is null after a refusal).  pse_clusters_label, in this order: a null g, N == 0 or N > n_max, a
 * null pos, all four outputs null, stats or hist not 8-byte aligned, hist with nhist == 0, an ex created on another handle than g, a
 * slab rank, a status word already known to be non-zero.  pse_clusters_status: a null g or status. */
typedef struct pse_clusters pse_clusters;
int pse_clusters_create(pse_handle *h, unsigned n, const unsigned *types_host /* n, or NULL: one type */, int ntypes,
                        const double *rlink_host /* npt */, pse_clusters **out);
int pse_clusters_destroy(pse_clusters *g);
int pse_clusters_label(pse_clusters *g, const pse_double4 *pos, const unsigned *group, unsigned N, unsigned *label /* DEVICE, may be NULL */,
                       unsigned *size /* DEVICE, may be NULL */, unsigned long long *stats /* DEVICE, 4, may be NULL */,
                       unsigned long long *hist /* DEVICE, nhist, ADDED to, may be NULL */, unsigned nhist,
                       const pse_exclusions *ex /* may be NULL */);
int pse_clusters_status(pse_clusters *g, unsigned *status /* HOST */);

/* ---- cluster analysis with percolation: spanning flags, images and radii of gyration (no reference counterpart) ----
 * Definitions.  The lattice is a1 = (Lx, 0, 0), a2 = (xy Ly, Ly, 0), a3 = (0, 0, Lz).  For a linked pair (i, j) the minimum image turns
 * d = r_i - r_j into d - (n1 a1 + n2 a2 + n3 a3), n2 = rint(d_y / Ly), n1 = rint((d_x - n2 xy Ly) / Lx), n3 = rint(d_z / Lz), the
 * integers the device's own; a link is never near a tie of rint (a tie means |d| ~ L/2 > rcut >= rlink).  n_ij = (n1, n2, n3) is
 * the SHIFT of the link.  An UNFOLDING of a cluster gives every member an integer vector c with c_j = c_i + n_ij on every link: then
 * U_i = r_i + c_i (a1, a2, a3) has U_i - U_j equal to the minimum-image vector on every link.  The WINDING of a closed walk over
 * links is the sum of its shifts; a cluster SPANS lattice axis k when some closed walk in it has a winding whose k-th component is
 * not zero.  An unfolding exists exactly when the cluster spans no axis, and is then unique up to one constant vector.
 * pse_clusters_span runs on a pse_clusters object, with the links of pse_clusters_label, and writes DEVICE arrays, each may be NULL
 * but not all:
 *   label, size, stats, hist   the outputs of pse_clusters_label, bit for bit
 *   span[t]    (unsigned, by caller index) bits 0, 1, 2 are set when t's cluster spans a1, a2, a3
 *   image[3 t .. 3 t + 2]  (int) c_t - c_label for a member of a cluster that spans nothing, label the cluster's label member: that
 *              member has (0, 0, 0) and the value does not depend on the sort; stated for the positions as the caller passes them,
 *              wrapped or not: pos[t] + image (a1, a2, a3) is the cluster made whole around its label member.  A member of a spanning
 *              cluster gets (0, 0, 0): an unfolding of it would depend on the order of the hooks
 *   rg2[t]     (double) the squared radius of gyration of t's cluster, 0 for a singleton, -1 for a spanning cluster: with 0 the
 *              label member, D_i = (r_i - r_0) + image_i (a1, a2, a3) in fp64 in this order,
 *                Dx = ((x_i - x_0) + i1 Lx) + i2 (xy Ly),  Dy = (y_i - y_0) + i2 Ly,  Dz = (z_i - z_0) + i3 Lz,
 *              q_i = llrint(D_i 2^20) per component, the integer sums sum q (three signed 64-bit words) and sum q^2 (two unsigned
 *              64-bit words: the low 32 bits of every q_k^2 into one, q_k^2 >> 32 into the other), and
 *                Rg^2 = 2^-40 (S2 / s - ((sx sx + sy sy) + sz sz) / (s s)),  S2 = (double)hi 2^32 + (double)lo,
 *              evaluated in fp64 in this order without contraction (the resolution of a coordinate is 2^-20, under 1e-6)
 *   pstats     eight unsigned 64-bit words, 8-byte aligned, OVERWRITTEN: spanning clusters; their members; clusters spanning a1; a2;
 *              a3; all three; the largest size among the clusters that span nothing; the sum of s^2 over those
 * Queue-only as pse_clusters_label, in a fixed sequence of launches of its own (the union-find with a 64-bit word per row: the
 * parent in 28 bits and the image offset to it in three 12-bit fields; the geometry launch only with rg2); no floating-point
 * atomics, only integers are summed: equal inputs give equal bits, rg2 included.  The first call on an object places its scratch
 * (68 bytes per particle of n_max), so a capture needs one call before it.
 * Three caps set further bits of the object's sticky status word and behave as the trip caps do (label = ~0u, size = 0, span = 0,
 * image = 0, rg2 = -1, stats and pstats zero; pse_clusters_status reports the word): 4, an image offset beyond +-2047 box lengths; 8,
 * a |q| >= 2^31, a member further than 2048 length units from its label member; 16, N > 2^28.  None is reachable at any size that is
 * tested or run.
 * PSE_ERR_INVALID as for pse_clusters_label and in its order -- the all-outputs-null refusal covering all eight outputs -- then rg2
 * or pstats not 8-byte aligned.  A slab rank is refused.
 * pse_host_cluster_word packs (parent < 2^28, c[3] each in [-2047, 2047]) into the word of the union-find as the device does,
 * pse_host_cluster_word_parts unpacks one; a value out of range or a null pointer is refused. */
int pse_clusters_span(pse_clusters *g, const pse_double4 *pos, const unsigned *group, unsigned N, unsigned *label /* DEVICE, may be NULL */,
                      unsigned *size /* DEVICE, may be NULL */, unsigned long long *stats /* DEVICE, 4, may be NULL */,
                      unsigned long long *hist /* DEVICE, nhist, ADDED to, may be NULL */, unsigned nhist,
                      unsigned *span /* DEVICE, may be NULL */, int *image /* DEVICE, 3 per particle, may be NULL */,
                      double *rg2 /* DEVICE, may be NULL */, unsigned long long *pstats /* DEVICE, 8, may be NULL */,
                      const pse_exclusions *ex /* may be NULL */);
int pse_host_cluster_word(unsigned parent, const int *c /* 3 */, unsigned long long *word);
int pse_host_cluster_word_parts(unsigned long long word, unsigned *parent, int *c /* 3 */);

/* ---- bond-orientational order: the Steinhardt q_l per particle, the neighbour-averaged q-bar_l and solid-like bonds (no reference counterpart) ----
 * A pse_bond_order object fixes the types of the particles, the neighbour distances and the degrees: types_host, ntypes <= 8 and the
 * pair types p(a, b) exactly as for pse_pair_hist_create (NULL: one type; a caller index >= n acts as type 0); rnb_host holds one
 * neighbour distance per pair type under the rules of rlink in pse_clusters_create: 0 switches a pair type off, every other entry
 * must be finite, > 0 and <= rcut, and at least one must be on; degrees_host holds nl distinct even degrees from {2, 4, ..., 12},
 * 1 <= nl <= PSE_BOND_ORDER_MAX_DEGREES (odd degrees vanish on centrosymmetric shells).
 * Two of the N group members i, j are NEIGHBOURS when their minimum-image distance has 0 < r^2 < rnb[p]^2 and the pair is not in ex;
 * the relation is symmetric.  For particle i with nb(i) neighbours and unit vectors d_ij = (r_j - r_i)/r, minimum image:
 *   c_lm(i)   = (1/nb) sum_j C_lm(d_ij), m = -l..l, C_lm = sqrt(4 pi/(2l + 1)) Y_lm the semi-normalised harmonics with the
 *               Condon-Shortley phase; only m = 0..l is formed, c_l,-m = (-1)^m conj c_lm; nb = 0 gives c_lm = 0
 *   q_l(i)    = sqrt(|c_l0|^2 + 2 sum_{m>0} |c_lm|^2), the usual sqrt(4 pi/(2l + 1) sum_m |q_lm|^2)
 *   qbar_l(i) from cbar_lm(i) = (c_lm(i) + sum_{j in nb(i)} c_lm(j)) / (nb(i) + 1) with the same norm (Lechner and Dellago)
 *   s_ij      = Re sum_m c_Lm(i) conj c_Lm(j) / (q_L(i) q_L(j)) for ONE designated degree L = degrees[solid_degree], defined as 0 when
 *               either q_L is 0; n_conn(i) is the number of neighbours with s_ij > threshold, and i is SOLID-LIKE when
 *               n_conn(i) >= min_conn (ten Wolde, Ruiz-Montero and Frenkel)
 * pse_bond_order_compute writes, all DEVICE arrays, each may be NULL but not all:
 *   nnb[t]            (unsigned, by CALLER index) nb(t)
 *   q[t nl + d]       (double, by caller index) q_l of degree d of the object;  qbar[t nl + d] likewise
 *   nconn[t]          (unsigned, by caller index) n_conn(t); not written when solid_degree < 0
 *   stats             2 ntypes unsigned 64-bit words, 8-byte aligned, OVERWRITTEN: stats[2a] the number of group members of type a,
 *                     stats[2a + 1] the number of those that are solid-like (0 when solid_degree < 0)
 * Rows of indices outside the group are left alone.
 * The harmonics are evaluated without an angle: C_lm = T_l^m(z) (x + i y)^m with the polynomial T_l^m = sqrt((l - m)!/(l + m)!)
 * P_l^m(z)/sin^m(theta) from the three-term recurrence upward in l and (x + i y)^m by repeated multiplication: no trigonometric call,
 * nothing singular at the poles.  DESIGN.md derives the error bound of c_lm, q_l and qbar_l from the order of the operations.
 * Queue-only wherever pse_pair_hist_accumulate is: the sort, the type mirror, one launch per degree (pass 1: c_lm and q_l) and one
 * more per degree that needs qbar or the solid bonds (pass 2, which gathers the neighbours' rows of c_lm); nothing is read back and
 * there are no floating-point atomics: every per-particle sum runs in the walk order of the stable-sorted rows, so equal inputs give
 * equal bits; stats is summed with integer atomics.  A permuted particle order changes the order of the sums: equal to rounding.
 * A slab rank (n_slabs >= 2) orders only its own cells: pse_bond_order_compute refuses it; teams and owned-particle steps have no
 * bond-order entry point.  Not computed: the third-order invariants w_l; neighbours by anything but a distance.
 * pse_bond_order_histogram bins one column of a caller-order array of nl columns (q or qbar of a compute, say) per type: the group
 * member t of type a with lo <= v < hi, v = values[t nl + column], adds 1 to counts[a nbins + b], b = min((int)((v - lo) nbins /
 * (hi - lo)), nbins - 1); other values, NaN included, are not counted.  counts (ntypes x nbins, ntypes nbins <= 8192) is ADDED to with
 * integer atomics: exact, samples accumulate on the device.  It needs neither the sort nor the cell list and works on any handle.
 * The object belongs to its handle as a pse_pair_hist does (pse_destroy frees it, pse_bond_order_destroy after that is a caller error;
 * pse_bond_order_destroy waits for the stream).  It holds the type mirror, the q_l of the sorted rows and the c_lm workspace: n_max
 * rows of sum_l (l + 1) complex doubles.  A failed allocation returns PSE_ERR_HIP, frees what it took and leaves *out null.
 * PSE_ERR_INVALID, with a message naming the value, nothing launched, nothing written: pse_bond_order_create, in this order: a null
 * out or h, n == 0 or n > n_max, ntypes outside [1, 8], a null rnb_host, an entry that is not finite, negative or > rcut, no entry on,
 * a type >= ntypes, nl outside [1, 4], a null degrees_host, a degree that is not even or outside [2, 12], a degree listed twice (*out
 * is null after a refusal).  pse_bond_order_compute, in this order: a null b, N == 0 or N > n_max, a null pos, all five outputs null,
 * solid_degree outside [-1, nl), with solid_degree >= 0 a threshold that is not finite or outside [-1, 1], stats not 8-byte aligned,
 * an ex created on another handle than b, a slab rank.  pse_bond_order_histogram, in this order: a null b, N == 0 or N > n_max, a
 * null values, column outside [0, nl), nbins < 1, ntypes nbins > 8192, lo or hi not finite, hi <= lo, a null counts or one that is not
 * 8-byte aligned. */
#define PSE_BOND_ORDER_MAX_DEGREES 4
#define PSE_BOND_ORDER_MAX_L       12
typedef struct pse_bond_order pse_bond_order;
int pse_bond_order_create(pse_handle *h, unsigned n, const unsigned *types_host /* n, or NULL: one type */, int ntypes,
                          const double *rnb_host /* npt */, int nl, const int *degrees_host /* nl */, pse_bond_order **out);
int pse_bond_order_destroy(pse_bond_order *b);
int pse_bond_order_compute(pse_bond_order *b, const pse_double4 *pos, const unsigned *group, unsigned N,
                           unsigned *nnb   /* DEVICE, by caller index, may be NULL */,
                           double   *q     /* DEVICE, caller index x nl, may be NULL */,
                           double   *qbar  /* DEVICE, caller index x nl, may be NULL */,
                           int solid_degree /* index into the degrees, or -1: no solid-bond pass */, double threshold, unsigned min_conn,
                           unsigned *nconn /* DEVICE, by caller index, may be NULL */,
                           unsigned long long *stats /* DEVICE, ntypes x 2, 8-byte aligned, OVERWRITTEN, may be NULL */,
                           const pse_exclusions *ex /* may be NULL */);
int pse_bond_order_histogram(pse_bond_order *b, const double *values /* DEVICE, caller index x nl, e.g. q or qbar */, int column,
                             const unsigned *group, unsigned N, int nbins, double lo, double hi,
                             unsigned long long *counts /* DEVICE, ntypes x nbins, 8-byte aligned, ADDED to */);

/* ---- chain conformations: the gyration tensor and the end-to-end vector of every molecule of a bond topology (no reference counterpart) ----
 * A pse_molecules object fixes the molecules: the connected components with at least two particles of the nbonds bonds pairs_host
 * (CALLER-order indices below n), laid out by pse_host_molecule_rows (below, which documents numbering, spanning tree, ends and tiles),
 * one type per MOLECULE (mol_types_host: nmol entries below ntypes <= 8 in the order of the molecule numbers, NULL: one type; copied at
 * creation) and nbins bins for the histogram of Rg on [0, rg_max) and of |R| on [0, ree_max) (nbins == 0: no histograms).  There is no
 * group argument: the topology names its particles.  Every particle has mass 1.
 * pse_molecules_compute, per molecule of m members, in the handle's CURRENT box (pse_set_box, tilt included):
 *   UNFOLDING.  The offset of member i from the root is u_i = the sum along the tree path root -> i of min_image(r_child - r_parent), the
 *   minimum image of the force passes (y first with the tilt taken off x, then x, then z; one rint per axis).  It is right through any
 *   number of Lees-Edwards flips and whatever image the integrator left a bead in, and VALID WHILE EVERY TREE EDGE IS SHORTER THAN HALF OF
 *   min(Lx, Ly, Lz); this is documented, not checked.  The sum runs by pointer jumping: round k adds to every member's partial sum the
 *   partial sum of its 2^k-th ancestor, so u_i is the balanced-tree sum of its path's edges, pairs first (a function of the layout alone).
 *   CENTRE.  su = sum of u_i by a halving tree over the breadth-first positions (position p adds position p + s for s = the powers of
 *   two below m, descending, where p + s < m);  c = r_root + su / m, NOT re-wrapped into the box.
 *   SECOND PASS.  v_i = u_i - su / m;  G_ab = (sum of v_a v_b, the same tree) / m;  Rg^2 = (G_xx + G_yy) + G_zz;  for a linear molecule
 *   R = u_hi - u_lo and R^2 = fma(R_z, R_z, fma(R_y, R_y, R_x R_x)): three roundings.
 *   rows[mol PSE_MOL_COLS + ...] = c(3), G_xx, G_yy, G_zz, G_xy, G_xz, G_yz, Rg^2, R(3), R^2; the four R columns are NaN for a molecule
 *   without ends.  unfolded[i] = (r_root + u_i, the molecule number in w) for every member i; rows of non-members are not touched.
 *   sums and sample, per molecule type a, PSE_MOL_COLS columns: 0-5 the sum of G_ab in the order above, 6 the sum of (Rg^2)^2, 7-12 the
 *   sum of R_a R_b in the same order, 13 the sum of (R^2)^2; 7-13 over the linear molecules only.  `sample` is WRITTEN with this call's
 *   sums alone, `sums` is ADDED to.  A type without molecules adds exactly +0.0.
 *   hist: row (0, a) bins Rg = sqrt(Rg^2), row (1, a) bins |R| = sqrt(R^2) (linear molecules), nbins + 1 counters a row, ADDED to:
 *   bin = (int)(value f), f = nbins / max formed once on the host; a value with value f >= nbins goes to the extra last counter.
 * One workgroup of PSE_MOL_TILE lanes handles one tile: it gathers the positions of its members once, keeps the partial sums of the
 * pointer jumping in two LDS buffers (56 KB), and reduces first the members of every molecule, then the molecules of every type with
 * halving trees whose order the layout alone fixes; it writes one partial row per type into a workspace the object owns, and a
 * finishing kernel adds the tiles in a fixed order, writes `sample` and adds to `sums`.  A 1024-bead chain costs 10 rounds.  No
 * floating-point atomics (the counters of hist are integers): equal inputs give equal bits.  The call only queues work on the handle's
 * stream and reads nothing back; it can be captured in a graph.  It does not sort and touches neither the cell list nor the kept
 * neighbour list, and it works on a slab rank's handle (positions are replicated there).
 * pse_molecules_count writes to HOST memory: *nmol, and per type the linear molecules and all molecules (ntypes entries each).
 * The object belongs to its handle exactly as a pse_msd does: pse_destroy frees the objects still alive, pse_molecules_destroy waits for
 * the stream.  A failed allocation returns PSE_ERR_HIP, frees what it took and leaves *out null.
 * OUT OF SCOPE: mass weighting, molecules of more than PSE_MOL_TILE members, and owned-particle ranks
 * (local_rows).  The pair sums of a molecule -- R^2(s), the bond correlation, the hydrodynamic radius -- are pse_molecule_pairs_compute;
 * the time correlations of R and of the normal modes are pse_chain_modes_correlate.
 * PSE_ERR_INVALID, with a message naming the value, nothing launched, nothing written: pse_molecules_create, in this order: a null out or
 * h, n == 0 or n > n_max, nbonds == 0, a null pairs_host, every refusal of pse_host_molecule_rows in its order, ntypes outside [1, 8], a
 * molecule type >= ntypes, nbins outside [0, 4096], with nbins > 0 an rg_max and then a ree_max that is not finite and positive (*out is
 * null after a refusal).  pse_molecules_compute, in this order: a null m, a null pos, every output NULL, rows, unfolded, sums, sample
 * or hist not aligned (8 bytes; unfolded 16), hist given to an object with nbins == 0.  pse_molecules_count: a null m, every output NULL. */
#define PSE_MOL_TILE 1024   /* members of one tile, and of the largest molecule */
#define PSE_MOL_COLS 14
typedef struct pse_molecules pse_molecules;
int pse_molecules_create(pse_handle *h, unsigned n, unsigned nbonds, const unsigned *pairs_host /* nbonds x 2 particle indices */,
                         const unsigned *mol_types_host /* nmol, or NULL: one type */, int ntypes, int nbins, double rg_max, double ree_max,
                         pse_molecules **out);
int pse_molecules_destroy(pse_molecules *m);
int pse_molecules_count(pse_molecules *m, unsigned *nmol, unsigned *nlinear /* ntypes */, unsigned *nmol_type /* ntypes */);
int pse_molecules_compute(pse_molecules *m, const pse_double4 *pos, double *rows /* DEVICE, nmol x 14, may be NULL */,
                          pse_double4 *unfolded /* DEVICE, caller order, may be NULL; non-members untouched */,
                          double *sums /* DEVICE, ntypes x 14, ADDED to, may be NULL */,
                          double *sample /* DEVICE, ntypes x 14, WRITTEN, may be NULL */,
                          unsigned long long *hist /* DEVICE, 2 x ntypes x (nbins + 1), ADDED to, may be NULL */);

/* ---- chain statistics: 1/Rh of every molecule, internal distances and bond correlations of the linear ones (no reference counterpart) ----
 * A pse_molecule_pairs object fixes the molecules of a bond list exactly as a pse_molecules does (its own layout of
 * pse_host_molecule_rows, one type per molecule, ntypes <= 8; its lifetime is not tied to a pse_molecules), the RANK of every member
 * (pse_host_chain_order: along the chain from the end with the lower caller index for a linear molecule, the breadth-first position
 * otherwise) and ns, the number of separations kept, 1 <= ns <= PSE_MOL_TILE.
 * pse_molecule_pairs_compute, per molecule of m members in the handle's CURRENT box: the offsets u are unfolded by the code of
 * pse_molecules_compute (the same bits); u_q is the offset of the member of rank q, and for a pair d = u_{c + s} - u_c,
 * r2 = fma(d_z, d_z, fma(d_y, d_y, d_x d_x)).
 *   H(s) = sum over c = 0 .. m - 1 - s of 1.0 / sqrt(r2), s = 1 .. m - 1; a pair with r2 == 0 adds nothing (the rule of the pair
 *   passes).  inv_rh[mol] = 2 (sum of H(s)) / m^2 = 1/Rh (Kirkwood), for every molecule, linear or not.
 *   For LINEAR molecules and 0 <= s < ns, with b_c = u_{c + 1} - u_c:  D(s) = sum over c = 0 .. m - 1 - s of r2 (D(0) = +0.0);
 *   C(s) = sum over c = 0 .. m - 2 - s of fma(b_z b'_z, fma(b_y b'_y, b_x b'_x)), b' = b_{c + s}, so that C(0) has the bits of D(1).
 *   A molecule with m <= s (m - 1 <= s for C) adds +0.0.  curves[(a ns + s) 2 + {0, 1}] += the sum of D(s), C(s) over the linear
 *   molecules of type a.  sums and sample, per type a, over ALL molecules of the type: column 0 the sum of inv_rh, column 1 the sum of
 *   inv_rh inv_rh (the product rounded, then added).  `sample` is WRITTEN with this call's sums alone, `sums` and `curves` are ADDED to.
 *   ORDER OF THE SUMS.  Within a (molecule, s): ascending c, one term after another, from +0.0.  The sum of H(s) over s: the halving
 *   tree of pse_molecules_compute over the ranks (rank q adds rank q + t for t = the powers of two below the largest molecule of the
 *   tile, descending, where q < t and q + t < m).  Within a (tile, type, s) and for the sums of a (tile, type): the molecules in
 *   ascending number, one after another, from +0.0.  Across the tiles: the finishing kernel of pse_molecules_compute (lane k of 64 adds
 *   the tiles k, k + 64, ... in ascending order, then the xor butterfly).  No floating-point atomics: equal inputs give equal bits.
 * pse_molecule_pairs_counts writes to HOST memory: *nmol, the molecules of every type, and terms, the number of summands behind each
 * entry of curves: the sum over the linear molecules of type a of max(m - s, 0) for D and of max(m - 1 - s, 0) for C.
 * One workgroup of PSE_MOL_TILE lanes handles one tile (the tiles of pse_host_molecule_rows): after the unfolding u lies in LDS as
 * three planes in rank order per molecule and the bond vectors as three more (56 KB with the plane of the H(s)); the lane of rank q
 * takes the separation s = q.  The workspaces of per-tile partial sums (ntiles x ntypes x ns x 2 and ntiles x ntypes x 2 doubles)
 * belong to the object: nothing is allocated in compute.  The call only queues work on the handle's stream and reads nothing back;
 * it can be captured in a graph.  It does not sort and touches neither the cell list nor the kept neighbour list, and it works on a
 * slab rank's handle.  The object belongs to its handle exactly as a pse_molecules does.
 * OUT OF SCOPE: mass weighting, molecules of more than PSE_MOL_TILE members, Rh with the RPY regularisation for overlapping beads,
 * owned-particle ranks, histograms of Rh.  Time correlations of a chain are pse_chain_modes_correlate.
 * PSE_ERR_INVALID, with a message naming the value, nothing launched, nothing written: pse_molecule_pairs_create, in this order:
 * everything pse_molecules_create refuses up to and including the molecule types, in its order, then ns outside [1, PSE_MOL_TILE].
 * pse_molecule_pairs_compute, in this order: a null p, a null pos, every output NULL, inv_rh, curves, sums or sample not 8-byte
 * aligned.  pse_molecule_pairs_counts: a null p, every output NULL. */
#define PSE_MOLPAIR_COLS 2   /* per separation: D, C */
#define PSE_MOLPAIR_SUMS 2   /* per type: sum of 1/Rh, sum of (1/Rh)^2 */
typedef struct pse_molecule_pairs pse_molecule_pairs;
int pse_molecule_pairs_create(pse_handle *h, unsigned n, unsigned nbonds, const unsigned *pairs_host /* nbonds x 2 particle indices */,
                              const unsigned *mol_types_host /* nmol, or NULL: one type */, int ntypes, int ns, pse_molecule_pairs **out);
int pse_molecule_pairs_destroy(pse_molecule_pairs *p);
int pse_molecule_pairs_counts(pse_molecule_pairs *p, unsigned *nmol, unsigned *nmol_type /* ntypes */,
                              unsigned long long *terms /* HOST, ntypes x ns x 2 */);
int pse_molecule_pairs_compute(pse_molecule_pairs *p, const pse_double4 *pos,
                               double *inv_rh /* DEVICE, nmol, WRITTEN, may be NULL */,
                               double *curves /* DEVICE, ntypes x ns x 2, ADDED to, may be NULL */,
                               double *sums   /* DEVICE, ntypes x 2, ADDED to, may be NULL */,
                               double *sample /* DEVICE, ntypes x 2, WRITTEN, may be NULL */);

/* ---- chain normal modes: K linear functionals of every linear molecule and their time correlations (no reference counterpart) ----
 * A pse_chain_modes object fixes the molecules of a bond list exactly as a pse_molecule_pairs does (its own layout of
 * pse_host_molecule_rows, one type per molecule, ntypes <= 8, the ranks q = 0 .. m - 1 of pse_host_chain_order), K = nmodes <=
 * PSE_CHAIN_MODES_MAX weight rows per distinct size of its LINEAR molecules, and norigins <= 64 stored time origins (0: static only).
 * Only the linear molecules (the `ends` of the layout) take part: nlin of them, numbered j = 0 .. nlin - 1 in ascending molecule
 * number.  sizes_host lists the distinct sizes m of the linear molecules in ascending order, weights_host holds, size after size, a
 * K x m row-major block of doubles w_{k,q}, copied at creation (the device keeps each block transposed).  The device layer knows no
 * trigonometry: Rouse modes are one choice of weights, made by pse_host_rouse_weights (below).
 * pse_chain_modes_compute, per linear molecule, in the handle's CURRENT box: X_k = sum over q of w_{k,q} u_q for k = 0 .. K - 1, u_q
 * the offset of the member of rank q as mol_unfold produces it -- the bits of pse_molecules_compute; no other unwrapping is used, so X is
 * continuous through Lees-Edwards flips wherever pse_molecules_compute is.  X goes into the object's CURRENT BUFFER, and to
 * modes[(j K + k) 3 + axis] if modes is given.  sums (ADDED to) and sample (WRITTEN), per type a and per k, PSE_CHAIN_MODES_STATIC
 * columns at ((a K + k) 6 + column): the sums over the linear molecules of the type of X_x^2, X_y^2, X_z^2, X_x X_y, X_x X_z, X_y X_z.
 * A type without linear molecules adds exactly +0.0.  Each of the three outputs may be NULL, and all three: the current buffer is an output.
 * pse_chain_modes_store copies the current buffer into origin slot `slot` (a device-to-device copy on the handle's stream) and marks
 * the slot stored (host bookkeeping, as pse_msd_store).
 * pse_chain_modes_correlate, for every listed pair (slot, row), every type a and every k, over the linear molecules of type a:
 *   corr[((row ntypes + a) K + k) PSE_CHAIN_MODES_CORR + 3 alpha + beta] += sum of X_alpha(current buffer) X_beta(slot);
 * all nine are kept because under shear <X_x(t) X_y(0)> != <X_y(t) X_x(0)>.  At most 64 pairs, by value in the launch.
 *   ORDER OF THE SUMS.  X_k: the ranks of a molecule in chunks of 16 (chunk c: q = 16 c .. min(16 c + 16, m) - 1); within a chunk
 *   ascending q, acc = fma(w, u, acc) from +0.0, per axis; then the chunks in ascending order, X += chunk, from +0.0: a function of m
 *   alone.  Static sums, within a (tile, type, k, column): the linear molecules of the tile in ascending number, acc = fma(X_a, X_b,
 *   acc) from +0.0; across the tiles the finishing kernel of pse_molecules_compute (lane l of 64 adds the tiles l, l + 64, ... in
 *   ascending order, then the xor butterfly: every lane adds the lane l xor o for o = 32, 16, ..., 1).  Correlations: the linear
 *   molecules in blocks of 256 consecutive j; lane l of 64 takes j0 + l, j0 + 64 + l, j0 + 128 + l, j0 + 192 + l in that order, acc =
 *   fma(X_alpha(now), X_beta(slot), acc) from +0.0 over those of type a (none: +0.0), then the xor butterfly: one partial row per (block,
 *   pair, type, k); across the blocks the same finishing rule (lane l adds the blocks l, l + 64, ..., then the butterfly), then the
 *   one addition to corr.  No floating-point atomics anywhere: equal inputs give equal bits.
 * pse_chain_modes_counts writes to HOST memory: *nmol, *nlin, the linear molecules of every type, and the molecule number and the
 * size of every linear molecule.
 * One workgroup of PSE_MOL_TILE lanes handles one tile: after the unfolding u lies in LDS as three padded planes in rank order; one
 * lane takes one (molecule, k, chunk), so that a tile of many short chains and a tile of one 1024-bead chain both fill their lanes;
 * 56 KB of LDS.  The weight tables, the current buffer, the norigins origin buffers (3 K nlin doubles each) and the workspaces of
 * partial sums (ntiles x ntypes x K x 6 and ceil(nlin / 256) x 64 x ntypes x K x 9 doubles) are allocated at creation: nothing is
 * allocated later.  A failed allocation returns PSE_ERR_HIP, frees what it took and leaves *out null.  The four device calls only
 * queue work on the handle's stream and read nothing back; they can be captured in a graph.  They use no sort, no cell list and no
 * kept neighbour list, and they work on a slab rank's handle.  The object belongs to its handle exactly as a pse_molecule_pairs does:
 * pse_destroy frees the objects still alive, pse_chain_modes_destroy waits for the stream.
 * OUT OF SCOPE: mass weighting, molecules of more than PSE_MOL_TILE members, non-linear molecules, the centre-of-mass mode p = 0 and
 * chain diffusion (that needs the unwrapped root, with the limit analyze.unwrap documents), owned-particle ranks (local_rows),
 * multi-tau (logarithmic) lag schemes.
 * PSE_ERR_INVALID, with a message naming the value, nothing launched, nothing written: pse_chain_modes_create, in this order:
 * everything pse_molecules_create refuses up to and including the molecule types, in its order, then nmodes outside [1,
 * PSE_CHAIN_MODES_MAX], norigins outside [0, 64], a bond set without a linear molecule, nsizes < 1, a null sizes_host, a null
 * weights_host, a size list that is not exactly the ascending set of the sizes of the linear molecules, a weight that is not finite
 * (*out is null after a refusal).  pse_chain_modes_counts: a null obj, every output NULL.  pse_chain_modes_compute, in this order: a
 * null obj, a null pos, modes, sums or sample not 8-byte aligned.  pse_chain_modes_store: a null obj, an object with norigins == 0,
 * slot outside [0, norigins), no compute since create.  pse_chain_modes_correlate, in this order: a null obj, an object with
 * norigins == 0, no compute since create, npairs outside [1, 64], a null slots_host, a null rows_host, nrows < 1, in the order of the
 * list a slot outside [0, norigins), then a slot never stored, then a row outside [0, nrows), then a row listed twice, then a null
 * corr or one that is not 8-byte aligned. */
#define PSE_CHAIN_MODES_MAX 32     /* functionals of one object */
#define PSE_CHAIN_MODES_STATIC 6   /* xx, yy, zz, xy, xz, yz */
#define PSE_CHAIN_MODES_CORR 9     /* 3 alpha + beta: alpha of now, beta of the origin */
typedef struct pse_chain_modes pse_chain_modes;
int pse_chain_modes_create(pse_handle *h, unsigned n, unsigned nbonds, const unsigned *pairs_host /* nbonds x 2 particle indices */,
                           const unsigned *mol_types_host /* nmol, or NULL: one type */, int ntypes, int nmodes, int nsizes,
                           const unsigned *sizes_host /* nsizes, ascending */,
                           const double *weights_host /* size after size nmodes x m, row-major */, int norigins, pse_chain_modes **out);
int pse_chain_modes_destroy(pse_chain_modes *obj);
int pse_chain_modes_counts(pse_chain_modes *obj, unsigned *nmol, unsigned *nlin, unsigned *nlin_type /* ntypes */,
                           unsigned *lin_mol /* HOST, nlin */, unsigned *lin_size /* HOST, nlin */);
int pse_chain_modes_compute(pse_chain_modes *obj, const pse_double4 *pos, double *modes /* DEVICE, nlin x K x 3, WRITTEN, may be NULL */,
                            double *sums   /* DEVICE, ntypes x K x 6, ADDED to, may be NULL */,
                            double *sample /* DEVICE, ntypes x K x 6, WRITTEN, may be NULL */);
int pse_chain_modes_store(pse_chain_modes *obj, int slot);
int pse_chain_modes_correlate(pse_chain_modes *obj, int npairs, const int *slots_host, const int *rows_host, int nrows,
                              double *corr /* DEVICE, nrows x ntypes x K x 9, ADDED to */);

/* ---- bonded forces: HOOMD's bond.harmonic and bond.fene(no reference counterpart: the reference leaves forces to HOOMD) ----
 * A pse_bonds object is a fixed bond topology on the device: nbonds pairs of particle indices into the caller-order arrays of n rows,
 * each with one of ntypes <= 64 parameter sets (kind, k, r0).  With d = r_i - r_j (minimum image in the handle's current box,
 * pse_set_box) and r = |d|, the force ON i FROM j is c d:
 *   PSE_BOND_HARMONIC  V = k/2 (r - r0)^2,                    c = -k (r - r0)/r
 *   PSE_BOND_FENE      V = -k/2 r0^2 ln(1 - (r/r0)^2), r < r0, c = -k / (1 - (r/r0)^2)
 * A bond with r == 0 contributes nothing and is not counted (the rule of the pair passes).  A FENE bond with r >= r0 contributes
 * nothing to the force, U or W, is not counted in nbonds and adds one to a counter in the object (HOOMD aborts there; a call that only
 * queues work cannot, so it counts): read it with pse_bonds_overstretched.  Duplicate bonds are legal and act once each, as in HOOMD.
 * The minimum image is the nearest one only for bonds shorter than half the smallest perpendicular box width: longer bonds are the
 * caller's error and are not detected.
 * The object is stored as one row of (partner, type) entries per particle, every bond in both endpoints' rows, each row sorted
 * (pse_host_bond_rows): forces and sums are therefore bit-identical for any order of the bond list and either order of a bond's endpoints.
 * The object belongs to its handle: pse_destroy frees the bond objects still alive, pse_bonds_destroy after that is a caller error.
 * pse_bonds_create returns PSE_ERR_INVALID, with a message naming the value, for: a null h, pairs_host, out or parameter array,
 * n == 0 or n > n_max, nbonds == 0 or nbonds > 2^30, an endpoint >= n, a bond with i == j, ntypes outside [1, 64], a type >= ntypes,
 * an unknown kind, a non-finite k or r0, r0 < 0, FENE with r0 <= 0. */
#define PSE_BOND_HARMONIC 0   /* V = k/2 (r - r0)^2 */
#define PSE_BOND_FENE     1   /* V = -k/2 r0^2 ln(1 - (r/r0)^2), r < r0 */
typedef struct pse_bonds pse_bonds;
int pse_bonds_create(pse_handle *h, unsigned n, unsigned nbonds,
                     const unsigned *pairs_host /* nbonds x 2 particle indices */,
                     const unsigned *types_host /* nbonds, or NULL: all type 0 */,
                     int ntypes, const int *kind_host, const double *k_host, const double *r0_host /* ntypes each */,
                     pse_bonds **out);
int pse_bonds_destroy(pse_bonds *b);
/* The bonded forces of the object on the n rows of pos, and their observables.  force (n rows, or NULL: observables only):
 * accumulate = 1 adds to .xyz of the bonded particles, rows of unbonded particles are neither read nor written; accumulate = 0
 * overwrites .xyz of all n rows, with zero for unbonded particles; w is kept in every case.  out8 (DEVICE, 8 doubles -- a row of a
 * larger array will do -- or NULL: forces only, the reduction is not run) = U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, nbonds with the signs of
 * pse_pair_repulsion_virial: U = sum V, W_ab = sum d_a (c d_b) with each bond once, stress = -W / V, dU/d(xy) = -Wxy, nbonds = 1.0
 * per bond that acted.  force and out8 both NULL: PSE_ERR_INVALID.  The pass walks the object's rows, not the cell list: it does not
 * sort, leaves the kept neighbour list and its counters alone, and works on a slab rank's handle too (positions are replicated there,
 * the sums over all bonds are complete); owned-particle steps are not supported.  The call only queues work on the handle's stream
 * and reads nothing back; no floating-point atomics, bit-reproducible on equal inputs. */
int pse_bond_forces(pse_bonds *b, const pse_double4 *pos, pse_double4 *force /* may be NULL */,
                    int accumulate, double *out8 /* DEVICE, may be NULL */);
/* FENE bonds found at r >= r0 by all pse_bond_forces calls on this object since its creation.  Waits for the handle's stream: the
 * only call of the bond interface that reads back. */
int pse_bonds_overstretched(pse_bonds *b, unsigned long long *count);

/* ---- angle forces: HOOMD's angle.harmonic and angle.cosinesq (no reference counterpart: the reference leaves forces to HOOMD) ----
 * A pse_angles object is a fixed set of nangles triples (i, j, k) of particle indices into the caller-order arrays of n rows, j the
 * VERTEX, each with one of ntypes <= 64 parameter sets (kind, k, theta0).  With d1 = r_i - r_j and d2 = r_k - r_j (each by minimum
 * image in the handle's current box, pse_set_box, as for the bonds), r1 = |d1|, r2 = |d2| and c = d1.d2 / (r1 r2) clamped to [-1, 1]:
 *   PSE_ANGLE_HARMONIC  V = k/2 (theta - theta0)^2, theta = acos(c),  g = -dV/dc = k (theta - theta0) / s, s = max(sqrt(1 - c^2), 1e-3)
 *   PSE_ANGLE_COSINESQ  V = k/2 (c - cos theta0)^2,                   g = -dV/dc = -k (c - cos theta0)
 *   F_i = g (d2 / (r1 r2) - c d1 / r1^2),  F_k = g (d1 / (r1 r2) - c d2 / r2^2),  F_j = -(F_i + F_k)
 * The floor on s is HOOMD's rule for the straight (and the folded) angle, where 1/s diverges: for sin(theta) < 1e-3 the harmonic
 * force is no longer exactly minus the gradient of the harmonic energy (it is smaller); at theta0 = pi the force still goes to zero
 * with theta -> pi.  The cosine-squared kind has no singularity and takes no acos.
 * An angle with r1 == 0 or r2 == 0 contributes nothing and is not counted (the rule of the pair and bond passes).  Duplicate angles are
 * legal and act once each.  The minimum image is the nearest one only for arms shorter than half the smallest perpendicular box
 * width: longer arms are the caller's error and are not detected.
 * The object is stored as one row of (i, j, k, type) entries per particle, every angle in the rows of all three of its particles, ends
 * canonicalised to i < k and each row sorted (pse_host_angle_rows): forces and sums are therefore bit-identical for any order of the
 * list and either order of an angle's ends.
 * The object belongs to its handle: pse_destroy frees the angle objects still alive, pse_angles_destroy after that is a caller error.
 * pse_angles_create returns PSE_ERR_INVALID, with a message naming the value, for: a null h, triples_host, out or parameter array,
 * n == 0 or n > n_max, nangles == 0 or nangles > 2^28, an index >= n, an angle with two equal members, ntypes outside [1, 64], a
 * type >= ntypes, an unknown kind, a non-finite k, a theta0 that is not finite or outside [0, pi].  *out is null after a refusal. */
#define PSE_ANGLE_HARMONIC 0   /* V = k/2 (theta - theta0)^2 */
#define PSE_ANGLE_COSINESQ 1   /* V = k/2 (cos theta - cos theta0)^2 */
typedef struct pse_angles pse_angles;
int pse_angles_create(pse_handle *h, unsigned n, unsigned nangles,
                      const unsigned *triples_host /* nangles x 3 particle indices: end, vertex, end */,
                      const unsigned *types_host /* nangles, or NULL: all type 0 */,
                      int ntypes, const int *kind_host, const double *k_host, const double *theta0_host /* ntypes each */,
                      pse_angles **out);
int pse_angles_destroy(pse_angles *a);
/* The angle forces of the object on the n rows of pos, and their observables.  force (n rows, or NULL: observables only):
 * accumulate = 1 adds to .xyz of the particles that are in an angle, rows of the others are neither read nor written; accumulate = 0
 * overwrites .xyz of all n rows, with zero for particles in no angle; w is kept in every case.  out8 (DEVICE, 8 doubles -- a row of a
 * larger array will do -- or NULL: forces only, the reduction is not run) = U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz, nangles with the signs of
 * pse_pair_repulsion_virial: U = sum V, W_ab = sum (d1_a F_i,b + d2_a F_k,b) with each angle once, stress = -W / V,
 * dU/d(xy) = -Wxy, nangles = 1.0 per angle that acted.  W is symmetric and its trace is zero to rounding for both kinds (an angle
 * does not change when everything is scaled).  force and out8 both NULL: PSE_ERR_INVALID.  The pass walks the object's rows, not
 * the cell list: it does not sort, leaves the kept neighbour list and its counters alone, and works on a slab rank's handle too
 * (positions are replicated there, the sums over all angles are complete); owned-particle steps are not supported.  The call only
 * queues work on the handle's stream and reads nothing back; no floating-point atomics, bit-reproducible on equal inputs. */
int pse_angle_forces(pse_angles *a, const pse_double4 *pos, pse_double4 *force /* may be NULL */,
                     int accumulate, double *out8 /* DEVICE, may be NULL */);

/* ---- dihedral forces: HOOMD's dihedral.harmonic and dihedral.opls (no reference counterpart: the reference leaves forces to HOOMD) ----
 * A pse_dihedrals object is a fixed set of ndihedrals quadruples (i, j, k, l) of four distinct particle indices into the caller-order
 * arrays of n rows, each with one of ntypes <= 64 parameter sets (kind and four doubles).  Every difference is taken by minimum image
 * in the handle's current box (pse_set_box), as for the bonds:
 *   d1 = r_i - r_j,  d2 = r_k - r_j,  d3 = r_k - r_l,   m = d1 x d2,  nn = d2 x d3,  b = |d2|
 *   phi = atan2(b (d1 . nn), m . nn)  in (-pi, pi]
 * This is the IUPAC convention: the planar cis arrangement is phi = 0, trans is phi = pi, and i = (0,1,0), j = 0, k = (1,0,0),
 * l = (1,0,1) has phi = +pi/2.  It is this convention whatever sign a given HOOMD version uses.  The pass takes no atan2: cos phi and
 * sin phi are m.nn and b d1.nn over |m| |nn|, the multiple angles follow by the angle-addition recurrence.
 *   PSE_DIHEDRAL_HARMONIC  params (k, d, mult, phi0):  V = k/2 (1 + d cos(mult phi - phi0)),  dV/dphi = -k d mult/2 sin(mult phi - phi0)
 *   PSE_DIHEDRAL_OPLS      params (k1, k2, k3, k4):    V = 1/2 [k1 (1 + cos phi) + k2 (1 - cos 2phi) + k3 (1 + cos 3phi) + k4 (1 - cos 4phi)]
 * Forces, with g = dV/dphi (the form without a division by sin phi):
 *   F_i = -g b / |m|^2 m,   F_l = +g b / |nn|^2 nn,   s = d1.d2 / b^2,  t = d3.d2 / b^2
 *   F_j = -F_i + s F_i - t F_l,   F_k = -F_l - s F_i + t F_l
 * The four forces sum to zero; reversing a quadruple to (l, k, j, i) gives the same phi and the same forces on the same particles.
 * A dihedral with |m|^2 == 0 or |nn|^2 == 0 -- a zero-length arm, three consecutive collinear particles -- contributes nothing and
 * is not counted (the rule of the pair, bond and angle passes for r == 0).  Duplicate dihedrals are legal and act once each.  The
 * minimum image is the nearest one only for arms (d1, d2, d3) shorter than half the smallest perpendicular box width: longer arms
 * are the caller's error and are not detected.
 * The object is stored as one row of (i, j, k, l) entries, with a parallel array of types, per particle, every dihedral in the rows
 * of all four of its particles, oriented so that i < l and each row sorted (pse_host_dihedral_rows): forces and sums are therefore
 * bit-identical for any order of the list and either direction a quadruple is written in.
 * The object belongs to its handle: pse_destroy frees the dihedral objects still alive, pse_dihedrals_destroy after that is a caller
 * error.
 * pse_dihedrals_create returns PSE_ERR_INVALID, with a message naming the value, for: a null h, quads_host, out or parameter array,
 * n == 0 or n > n_max, ndihedrals == 0 or ndihedrals > 2^28, an index >= n, a quadruple with two equal members, ntypes outside
 * [1, 64], a type >= ntypes, an unknown kind, a non-finite parameter, a harmonic d that is not exactly -1 or +1, a harmonic mult that
 * is not an integer in [1, 6].  *out is null after a refusal. */
#define PSE_DIHEDRAL_HARMONIC 0   /* V = k/2 (1 + d cos(mult phi - phi0)) */
#define PSE_DIHEDRAL_OPLS     1   /* V = 1/2 [k1 (1 + cos phi) + k2 (1 - cos 2phi) + k3 (1 + cos 3phi) + k4 (1 - cos 4phi)] */
typedef struct pse_dihedrals pse_dihedrals;
int pse_dihedrals_create(pse_handle *h, unsigned n, unsigned ndihedrals,
                         const unsigned *quads_host /* ndihedrals x 4 particle indices: i, j, k, l */,
                         const unsigned *types_host /* ndihedrals, or NULL: all type 0 */,
                         int ntypes, const int *kind_host /* ntypes */, const double *params_host /* ntypes x 4 */,
                         pse_dihedrals **out);
int pse_dihedrals_destroy(pse_dihedrals *d);
/* The dihedral forces of the object on the n rows of pos, and their observables.  force (n rows, or NULL: observables only):
 * accumulate = 1 adds to .xyz of the particles that are in a dihedral, rows of the others are neither read nor written;
 * accumulate = 0 overwrites .xyz of all n rows, with zero for particles in no dihedral; w is kept in every case.  out8 (DEVICE, 8
 * doubles -- a row of a larger array will do -- or NULL: forces only, the reduction is not run) = U, Wxx, Wxy, Wxz, Wyy, Wyz, Wzz,
 * ndihedrals with the signs of pse_pair_repulsion_virial: U = sum V, W_ab = sum (d1_a F_i,b + d2_a F_k,b + (d2 - d3)_a F_l,b) with
 * each dihedral once, stress = -W / V, dU/d(xy) = -Wxy, ndihedrals = 1.0 per dihedral that acted.  W is symmetric and its trace is
 * zero to rounding for both kinds (a dihedral angle does not change when everything is scaled or rotated).  force and out8 both
 * NULL: PSE_ERR_INVALID.  The pass walks the object's rows, not the cell list: it does not sort, leaves the kept neighbour list and
 * its counters alone, and works on a slab rank's handle too (positions are replicated there, the sums over all dihedrals are
 * complete); owned-particle steps are not supported.  The call only queues work on the handle's stream and reads nothing back; no
 * floating-point atomics, bit-reproducible on equal inputs. */
int pse_dihedral_forces(pse_dihedrals *d, const pse_double4 *pos, pse_double4 *force /* may be NULL */,
                        int accumulate, double *out8 /* DEVICE, may be NULL */);
/* copy the three real-space grids (x-major, z fastest: idx = (x*Ny + y)*Nz + z, PSEv1/Mobility.cu:233) of the
 * most recent spread (stage 0) or inverse FFT (stage 1) to a host buffer of 3*nx_local*Ny*Nz doubles */
int pse_debug_copy_grid(pse_handle *h, int stage, double *host_out);
/* sort + spread only (gpu_stokes_Spread_kernel, PSEv1/Mobility.cu:114-252): leaves the three force grids in place for
 * pse_debug_copy_grid, so the spread can be compared node by node and not only through the gather */
int pse_debug_spread(pse_handle *h, const pse_double4 *pos, const pse_double4 *force, const unsigned int *group_members,
                     unsigned int N);
/* sort + gather only (gpu_stokes_Contract_kernel, PSEv1/Mobility.cu:325-477), the twin of pse_debug_spread: the three velocity grids
 * are taken from grid_host (HOST array of 3*nx_local*Ny*Nz doubles in the layout pse_debug_copy_grid returns) and gathered at the
 * particles; vel_out (DEVICE, rows in the caller's order like pse_mobility's vel, .w kept) = h^3 sum_nodes w u_grid, so the gather can
 * be checked against any grid -- a single nonzero node gives one weight -- and not only behind spread and transforms.  No slab
 * ranks. */
int pse_debug_gather(pse_handle *h, const pse_double4 *pos, const double *grid_host, const unsigned int *group_members,
                     unsigned int N, pse_double4 *vel_out);
/* which far-field kernels a call with N particles launches on this handle, by the host functions that decide the launches:
 * out6 = {spread by blocks (k_spread_tiles; 0: k_spread_atomic), its TZ (8 | 16), its NW (1 | 4), gather by bins (k_gather_bins;
 * 0: k_gather), its BZ (1 | 2), SHEAR instantiations (xy != 0)}; TZ, NW, BZ are 0 where the generic kernel runs.  Lets a test
 * assert the instantiation it was written for (PSE_SPREAD_TZ, PSE_SPREAD_NW, PSE_GATHER_BZ are read per handle in pse_create). */
int pse_debug_far_path(pse_handle *h, unsigned int N, int *out6);
/* the wave-space stage of a step from grid to grid, by the code a step runs (the transforms of part 0, parts 1 and 2 of the chain): the
 * three real grids are taken from grid_in_host (HOST, 3*Nx*Ny*Nz doubles in the layout pse_debug_copy_grid returns; NULL: zeros),
 * transformed forward (z, y, x), multiplied by the k-space operator -- with xi / eta in place of the handle's own where > 0; eta = 1
 * switches the exponential of the operator off, so that no mode is damped out of sight -- plus the k-space noise of (kT, dt, timestep)
 * if noise != 0, transformed back and copied to grid_out_host (HOST, same layout).  poison != 0: before the input is copied in, every
 * byte of the real grids and of the spectra is set to 0xFF (NaN doubles: the pad columns of the spectrum rows included), so that a
 * kernel that lets pad or stale data into a live mode turns the output into NaN.  Every tuning switch acts as on a step.  No slab ranks. */
int pse_debug_wave_grid(pse_handle *h, const double *grid_in_host, double xi, double eta, int noise, double kT, double dt,
                        unsigned int timestep, int poison, double *grid_out_host);
/* which transform kernels this handle runs, by the functions the launchers switch on: out8 = {xfuse, own_y, own_z,
 * x kernel (0: rocFFT + k_scale, 1: k_xfft_scale in LDS, 2: k_xfft_scale_cols in registers, 3 / 4: k_xfft_scale_mixed with a
 * compile-time / runtime plan), its kz columns per workgroup,
 * y kernel (0: rocFFT, 1 / 2: k_fft_cols with a compile-time / runtime plan, 3: k_yfft_regs), its kz columns per workgroup,
 * z kernel (0: rocFFT, 1: k_zfft_rows, 2: k_zfft_rows_g)}.  The PSE_* switches are read per handle in pse_create. */
int pse_debug_fft_path(pse_handle *h, int *out8);
/* the k-space operator of n grid nodes (i, j, k) (host array of 3 n ints, 0 <= k < Nz: any node of the reference's full C2C
 * grid) exactly as the scaling kernels evaluate it, for the current box: out_host[5 t ..] = kx, ky, kz, w sinc^2,
 * sqrt(w) sinc -- what gpu_stokes_SetGridk_kernel tabulates (PSEv1/Helper.cu:285-332: index folding, sheared ky, scale
 * factor w) and gpu_stokes_Green_kernel / gpu_stokes_BrownianGridGenerate_kernel multiply by (PSEv1/Mobility.cu:290,
 * PSEv1/Brownian.cu:274-276) */
int pse_debug_kvector(pse_handle *h, int n, const int *ijk_host, double *out_host);
/* what pse_create's grid-placement planner did (single-GPU engines with grids of >= 96 MB of spectra; PSE_PLACE_TRIALS=K, default 10,
 * 0 or 1: off): the transform passes that read the spectra run 5 - 20 % faster or slower depending on where the driver placed the
 * two far-field grids, for the life of the allocation, so pse_create allocates the pair up to K times (it stops at the first pair 5 % below the slowest seen), times the x pass and the
 * inverse y + z passes on each and keeps the fastest (+ 5 - 20 ms at create; results do not depend on the choice).  *tried = pairs timed (0: planner off or
 * not applicable), ms_first / ms_kept = the probe's time on the first pair and on the kept one.  No reference counterpart (cuFFT
 * plans own their work areas, PSEv1/Stokes.cc:262-269). */
int pse_debug_grid_placement(pse_handle *h, int *tried, float *ms_first, float *ms_kept);
/* the 16-byte form in which the single GPU's pair-list mat-vec reads its NEIGHBOURS' rows of the Lanczos vector (three 40-bit
 * mantissas under one exponent, written beside every new vector; the double rows stay the truth for the diagonal term, the sums and
 * the final combination): rows_host [n][3] -> packed on the device -> unpacked -> out_host [n][3].  |out - in| <= 2^-39 of the row's
 * largest component.  Why: a gather of 64 scattered rows costs the texture path the same whether it fetches 8 or 16 bytes per lane,
 * and 24 bytes of doubles are two of them per pair.  PSE_VQ=0 reads doubles (A/B).  No reference counterpart (the reference's
 * mat-vec recomputes every pair from single-precision positions, PSEv1/Mobility.cu:495-600). */
int pse_debug_vq_roundtrip(int n, const double *rows_host, double *out_host);
/* the device-side Lanczos decision (k_lz_decide: what ends every queue-only Brownian call and every owned-particle team step) on GIVEN
 * coefficients, for tests: scal_host is one image of the device scalars (PSE_DEBUG_LZ_NSCAL doubles: alpha at 0, beta at 128, the
 * norm of psi at 256), dec the decisions of one call in the order a driver issues them (fields as LzDecide, pse_host.h; seq is the
 * call's number as the host mirror gets it), open0 the initial value of the mirror's count of calls that ended open.  The decision
 * state starts as NaN bytes -- the reset under `first` is what makes it valid --, the decisions are launched in order on one stream,
 * and after each launch the state and the five mirror slots (m, step norm, status, seq, open calls) are copied to out[k].  Current
 * device, no handle.  PSE_ERR_INVALID, before anything is launched: a null array, n_dec outside [1, 40], a first decision without
 * `first`, m_hi that pse_debug_lz_decide_supported refuses (the eigenvectors of the sizes m_hi - 1 and m_hi must fit the LDS of one
 * workgroup: 1 .. 98), m_lo not m_hi - 1 or m_hi or below 1, done_iters < m_hi or > 100, pending_beta outside [0, m_hi], m_max > 100. */
#define PSE_DEBUG_LZ_NSCAL 400
typedef struct pse_debug_lz_decision {
    int m_lo, m_hi, done_iters, have_last_beta, pending_beta, first, last, normalised, m_max;
    double tol, seq;
} pse_debug_lz_decision;
typedef struct pse_debug_lz_outcome {
    int done, m_final, checked, status;
    double stepnorm;
    double t_prev[104];
    double coef[104];
    double mirror[5];
} pse_debug_lz_outcome;
int pse_debug_lz_decide(const double *scal_host, int n_dec, const pse_debug_lz_decision *dec, double open0, pse_debug_lz_outcome *out);
int pse_debug_lz_decide_supported(int m_hi);   /* 1: a decision may check the sizes m_hi - 1 and m_hi */
/* the dominant kernel of a Brownian step by itself: `reps` launches of the pair-list mat-vec of a Lanczos iteration (k_mreal_list; the
 * list, the vectors and the mirror of the Brownian call that has just ended; results go to scratch) back to back on the engine's
 * stream between ONE pair of events -> milliseconds per launch.  What bench.py's `roofline` divides by: an event pair around a single
 * launch inside a step carries 5 - 8 us of marker latency, this one a fraction of a microsecond.  Single-GPU engines, right after
 * pse_step / pse_brownian_velocity with kT > 0 (PSE_ERR_INVALID otherwise). */
int pse_debug_matvec_ms(pse_handle *h, int reps, float *ms_per_launch);

/* -- multi-GPU: slab-decomposed far field + row-sharded near field (new design; the reference is single-GPU,
 *    PSEv1/Stokes.cc:104) ---------------------------------------------------------------------------------------
 * Each rank is a handle created with pse_params.n_slabs = G and its own slab_rank.  The far-field grid is cut into
 * G slabs of x planes (the slowest index of the reference layout, PSEv1/Mobility.cu:233): spread and the 2-D (y,z)
 * transforms are slab-local, an all-to-all transposes to y-slabs for the 1-D x transforms and the k-space scaling,
 * and back; the gather takes (P-1)/2 halo planes from the previous slab and (P+1)/2 from the next.  The near-field cell
 * layers along x are split the same way, so a rank owns one contiguous block of the cell-sorted rows: its near field,
 * its rows of every Lanczos vector and its gathered velocities, exchanged once per call.  The Lanczos iteration of a team
 * runs TWO iterations per exchange where the decomposition allows (two ghost cell layers per neighbour, the second near-field
 * product of a block on the own rows, the recurrence coefficients from eight summed products: pse_info.lanczos_exchanges),
 * one per iteration otherwise; every exchange of a team -- ghost rows with the ranks' partial sums, all-to-alls, plane halos,
 * the final row all-gather -- is ONE group of point-to-point transfers, all posted on one communication stream in program
 * order, while the far-field chain and the near field / Lanczos chain run on two compute streams next to each other.
 * Particle arrays are replicated: every rank passes the same pos/force and ends the call with the same vel/pos.
 * A team binds the local ranks to a transport: one member per process + the RCCL unique id of rank 0 (production, one
 * process per GPU), or all G members in one process with id = NULL (in-process loopback on one device, for tests). */
typedef struct pse_team pse_team;
int pse_team_unique_id(void *id128_host);   /* host buffer of 128 bytes, call on rank 0 and distribute */
int pse_team_create(pse_handle **members, int n_members, const void *id128_host, pse_team **out);
/* A third transport, supplied by the host program: one member per process as with RCCL, but every exchange is staged through
 * pinned host memory and handed to a callback -- a list of point-to-point transfers between ranks (every rank of the team
 * calls with its own list at the same point of the step; transfers between one pair of ranks match in list order).  Buffers are
 * host memory, counts are in doubles, send_to / recv_from = -1 where an entry has no send / no
 * receive; return 0 on success.  The exchanges are exactly those of the RCCL transport (same buffers, counts, peers and
 * order: both run through one transfer list), which is what makes the process-per-rank driver testable where RCCL cannot run
 * (two ranks on one GPU), e.g. over torch.distributed's gloo backend; it is also a fallback for nodes without xGMI. */
typedef struct pse_host_xfer {
    const double *send; size_t send_count; int send_to;
    double *recv; size_t recv_count; int recv_from;
} pse_host_xfer;
typedef struct pse_transport {
    void *user;
    int (*exchange)(void *user, int n_xfers, const pse_host_xfer *xfers);
    int (*allreduce_sum)(void *user, double *host_buf, size_t count);   /* not called since round 4 (may be NULL): the Lanczos sums
                                                                           travel as small blocks inside `exchange` */
} pse_transport;
int pse_team_create_transport(pse_handle *member, const pse_transport *transport, pse_team **out);
/* Destroy the team BEFORE its members: the members must outlive it (an in-process team lends member 0's side stream to the
 * others and hands every member its own back here). */
int pse_team_destroy(pse_team *team);
/* the three hot-path entry points for a team; pointer arrays have one entry per local member, in members order */
int pse_team_mobility(pse_team *team, const pse_double4 *const *pos, const pse_double4 *const *force,
                      pse_double4 *const *vel, const unsigned int *group_members, unsigned int N, int parts);
int pse_team_brownian_velocity(pse_team *team, const pse_double4 *const *pos, const pse_double4 *const *force,
                               pse_double4 *const *vel, const unsigned int *group_members, unsigned int N,
                               double kT, double dt, unsigned int timestep, int *lanczos_m);
int pse_team_step(pse_team *team, pse_double4 *const *pos, pse_double4 *const *vel, pse_double3 *const *accel,
                  pse_int3 *const *image, const pse_double4 *const *net_force, const unsigned int *group_members,
                  unsigned int N, double kT, double dt, unsigned int timestep, double shear_rate, int *lanczos_m);

/* -- owned-particle teams (round 5) ----------------------------------------------------------------------------------------
 * The calls above replicate the particle state: every rank passes all N particles, bins all of them, and takes part in an
 * all-gather of the velocities every step.  Here a rank passes ONLY THE PARTICLES IT OWNS -- those of its x slab of the box, as
 * HOOMD's domain decomposition hands them to a plugin (the reference is single-GPU, PSEv1/Stokes.cc:104; per-step data flow
 * PSEv1/Stokes.cc:433-514) -- and the engine does what HOOMD's Communicator would: particles that have left the slab migrate to the
 * neighbour, the ghost layers the near field, the spreading and the two-step Lanczos blocks need arrive from both neighbours,
 * all in ONE exchange of fixed-size messages at the start of the step.  No rank touches the other N (G - 1) / G particles, there
 * is no all-gather, and NOTHING is read back inside a step: row counts and ranges live in device memory, the Lanczos decision
 * is taken on the device (as with pse_set_async), every exchange has host-known sizes (capacities).
 *
 * Handles: pse_params.local_rows = 1, n_slabs = G >= 2, n_max = row capacity (pse_local_layout tells how it is divided).  Needs
 * >= 3 cell layers per rank along x (>= 4 with two ranks), the pair list and the real-space table in LDS.
 * Arrays (per member, device): rows [0, *n_local) of pos / vel / accel / image / net_force / tag are the particles the rank owns
 * (capacity: rows_own of pse_local_layout); tag = the particle's global index (keys the particle noise, PSEv1/Brownian.cu:117;
 * identifies it across ranks); vel.w = mass.  On entry a particle may have left the slab by less than a slab width (the last
 * step moved it).  On return the arrays hold the particles the rank owns NOW, in the engine's cell order (pos, vel, accel,
 * image, tag rewritten; net_force is an input: the caller recomputes it for the new order), *n_local their number (a device
 * word: the host learns it when it asks).  integrate = 0: velocities only, positions unchanged (but reordered likewise).
 * kT = 0: deterministic.  *lanczos_m as for queue-only calls (pse_set_async).  Errors that show on the device only (a capacity
 * exceeded, a particle that moved further than a neighbour) are sticky: pse_team_local_status reads them (synchronises), and
 * the next call refuses to start.
 * Shear: the slabs are slabs of the FRACTIONAL x coordinate, so between two calls of pse_set_box that follow the strain
 * continuously an affinely advected particle keeps its slab.  A Lees-Edwards FLIP of the tilt (xy + 0.5 -> - 0.5,
 * PSEv1/VariantShearFunction.cc:34-43) re-maps the fractional x of every particle by its fractional y: the owner of the particle
 * data redistributes them before the next call (what HOOMD's domain decomposition does at a flip): pse_team_redistribute_local
 * below -- a step cannot follow it (flag 8). */
int pse_team_step_local(pse_team *team, pse_double4 *const *pos, pse_double4 *const *vel, pse_double3 *const *accel,
                        pse_int3 *const *image, const pse_double4 *const *net_force, unsigned int *const *tag,
                        unsigned int *const *n_local, double kT, double dt, unsigned int timestep, double shear_rate,
                        int integrate, int *lanczos_m);
/* The Lees-Edwards flip for an owned-particle team: after pse_set_box has taken the tilt of EVERY member through the flip, one call
 * re-owns every particle by its fractional x under the new box -- any particle may go to any rank -- through the team's own transfer
 * list (count rows first, then exactly the records that move, in the wire format of the step's first exchange).  Arrays as for
 * pse_team_step_local (net_force is rewritten too: the rows have a new order; vel.xyz and accel come back zero, vel.w = mass kept);
 * on return -- the work is queued on the members' streams -- rows [0, *n_local) hold what the rank owns now.  The call waits for the
 * streams twice (the host sizes the second exchange): it runs once per unit of strain.  If some rank's arrays could not hold what it
 * would own, NOTHING is moved and every rank returns PSE_ERR_INVALID (every rank sees every count row).
 * HOOMD call site: where the reference's box-tilt updater wraps the strain (PSEv1/VariantShearFunction.cc:34-43). */
int pse_team_redistribute_local(pse_team *team, pse_double4 *const *pos, pse_double4 *const *vel, pse_double3 *const *accel,
                                pse_int3 *const *image, pse_double4 *const *net_force, unsigned int *const *tag,
                                unsigned int *const *n_local);
/* Iterations an owned-particle step queues beyond its starting count *lanczos_m, in blocks of two, every kernel of them gated on
 * the device-side decision (default -1: the members' PSE_LANCZOS_EXTRA, 2).  A time-stepping loop whose last steps all ended
 * at their starting count with pse_info.lanczos_status 0 can set 0: the gated block -- one more exchange, seven launches that
 * leave at once -- is then not queued at all (~ 45 us of a 0.65 ms rank step at the metric point); a step whose count then does
 * not suffice says so (lanczos_status 1, the result uses the last size) and the caller goes back to the default and a larger
 * count.  The same value on every rank of the team (it decides how many exchanges a step has): derive it from numbers every rank
 * holds -- pse_info after a synchronisation is one: all ranks take the same decisions from the same sums.
 * Between processes *lanczos_m of pse_team_step_local comes back UNCHANGED (within one process: the most recent m that has
 * reached the host): read pse_info.lanczos_m after a synchronisation and pass the same count on every rank. */
int pse_team_set_lanczos_extra(pse_team *team, int extra);
/* the same for the queue-only calls of a single-GPU handle (pse_set_async): iterations queued beyond the starting count, each gated on
 * the device-side decision (default -1: PSE_LANCZOS_EXTRA, 2).  With 0 a step whose starting count suffices queues no gated iteration at
 * all (ten launches that would leave at once: ~ 25 us of a 3 ms step at the metric point); pse_info.lanczos_status = 1 /
 * lanczos_open_calls say when it did not.  The reference iterates until the step norm passes (PSEv1/Brownian.cu:606-724). */
int pse_set_lanczos_extra(pse_handle *h, int extra);
/* The near-field operator inside the Lanczos iteration of M_real^{1/2} psi (pse_brownian_velocity, pse_brownian_velocity_part, pse_step,
 * pse_sqrt_mreal, the team calls).  PSE_LANCZOS_RECORDS16 (default): the pair coefficients from the 16-byte records of the per-step pair
 * list, rounded to single-precision accuracy, and (single GPU) the neighbours' rows from their 16-byte mirror -- see the precision note
 * at the top; tolerances below about 1e-6 are not honoured.  PSE_LANCZOS_FP64: the exact fp64 operator everywhere the iteration applies
 * it -- a 32-byte plane of fp64 coefficients beside the records (allocated by the first call that selects it, here on the host, and
 * counted in pse_info.device_bytes: 32 bytes per pair-list slot), the rows gathered as doubles, the square root in double; each
 * mat-vec streams about three times the bytes.  The environment variable PSE_LANCZOS_OP=fp64, read in pse_create, sets the starting
 * mode.  Calls already queued keep the mode they were queued with; a graph captured before a switch keeps its mode and must be
 * captured again.  In-process team calls refuse members whose modes differ (PSE_ERR_INVALID); the ranks of a process team must all
 * set the same mode.  The deterministic U = M.F and the far field are fp64 in either mode.  Other values, a null handle or pointer:
 * PSE_ERR_INVALID. */
enum pse_lanczos_operator { PSE_LANCZOS_RECORDS16 = 0, PSE_LANCZOS_FP64 = 1 };
int pse_set_lanczos_operator(pse_handle *h, int op);
int pse_get_lanczos_operator(pse_handle *h, int *op);
/* row capacities of an owned-particle handle: own rows (= capacity the caller's arrays need), ghost rows per side, records per
 * neighbour message of the first exchange; cell layers along x in all and per rank (any pointer may be null) */
int pse_local_layout(pse_handle *h, int *rows_own, int *rows_ghost, int *records, int *layers, int *layers_per_rank);
/* waits for the team's streams; flags[member] = 0 or a combination of 1 own rows exceeded, 2 ghost rows exceeded, 4 message
 * capacity exceeded, 8 a particle moved beyond the neighbour's slab, 16 *n_local above the capacity; returns PSE_ERR_INVALID if any */
int pse_team_local_status(pse_team *team, int *flags);

/* -- self-diagnosis of a team call (for the first run on a multi-GPU node: one number would say nothing about where the time went)
 * With it on, every exchange of a call is bracketed by two events on the stream of the lane that issues it, and the spans of
 * the two lanes are taken the same way; pse_team_get_diag waits for the call and reads them.  kind: 0 the first exchange of an
 * owned-particle step (migrants + ghosts), 1 Lanczos (ghost rows of the mat-vec results + the ranks' partial sums), 2 all-to-all
 * of the far-field transpose, 3 plane halo of the gather, 4 velocity all-gather (replicated-state calls), 5 other ghost rows. */
#define PSE_DIAG_MAX 48
typedef struct pse_team_diag {
    int n_exchanges;
    int kind[PSE_DIAG_MAX];
    int lane[PSE_DIAG_MAX];                   /* 0 main lane (sort, near field, Lanczos, update), 1 far-field lane */
    double device_us[PSE_DIAG_MAX];           /* between the two events: for RCCL the hand-over to the communication stream, the
                                                 transfers and the hand-over back; host-staged transport: incl. the host's part */
    double host_us[PSE_DIAG_MAX];             /* host time spent issuing it (host-staged transport: the whole staged exchange) */
    unsigned long long bytes[PSE_DIAG_MAX];   /* sent by this rank */
    double main_lane_ms, side_lane_ms;        /* first to last event of the lane's stream inside the call (side: fork to join; 0: one lane) */
    double critical_path_ms;                  /* = main_lane_ms: the main lane joins the far-field lane before it ends */
} pse_team_diag;
int pse_team_set_diag(pse_team *team, int enabled);
int pse_team_get_diag(pse_team *team, pse_team_diag *out);

/* Developer switch for an IN-PROCESS team (measurement, not a result): from now on the team queues the work of the one member
 * with this slab rank only -- its kernels on both lanes and the copies that stand for what it receives; the other members'
 * buffers keep what the last full call left there.  The wall time of a call is then that rank's critical path with a GPU to
 * itself, lanes overlapping as they would (tools/perf_team.py --solo); the numbers it returns are not meaningful.  Call with the
 * same positions as the last full call and do not integrate; slab_rank < 0 switches it off. */
int pse_team_debug_solo(pse_team *team, int slab_rank);

/* host-only: t = T^{1/2} e_1 of the Lanczos tridiagonal (alpha[0..m), beta[1..m)); replaces LAPACKE_spteqr +
 * the host loops at PSEv1/Brownian.cu:540-582. Exposed so the eigen-solver can be tested without a GPU. */
int pse_host_lanczos_sqrt_e1(int m, const double *alpha, const double *beta, double *t);
/* host-only: the Lanczos decision of the host-checked Brownian calls (lz_decide_host: what ends the iteration of every call that is not
 * queue-only) on GIVEN coefficients -- the arguments, the structs, the initial state of NaN bytes and the outcome per decision of
 * pse_debug_lz_decide, with the five mirror values kept as the device's decision would leave them, and no device.  A decision may
 * check any number of sizes (the host drivers' batches grow): PSE_ERR_INVALID for a null array, n_dec outside [1, 40], a first
 * decision without `first`, anything but 1 <= m_lo <= m_hi <= done_iters <= 100, pending_beta outside [0, m_hi], m_max > 100.  A
 * non-finite coefficient or a failed eigen-solve is status 2 in the outcome, not an error of this call. */
int pse_host_lz_decide(const double *scal_host, int n_dec, const pse_debug_lz_decision *dec, double open0, pse_debug_lz_outcome *out);
/* host-only: the real-space table a handle of (xi, rcut) holds on the device (build_realspace_table, pse_params.cpp), without creating
 * one.  n_intervals = ceil(8 rcut) + 1 intervals of width 1/8; interval k is 20 doubles at coef[20 k]: ten coefficients of f_w and ten
 * of g_w in powers of t = 2 (8 r - k) - 1, lowest first (the smooth parts: f = f_RPY - f_w, g = g_RPY - g_w).  *n_intervals is set
 * whenever xi and rcut are valid, so a first call with cap = 0 sizes the array.  PSE_ERR_INVALID: xi or rcut not positive,
 * 8 rcut >= 1e6, a null pointer, cap (in doubles) below 20 n_intervals. */
int pse_host_realspace_table(double xi, double rcut, int cap, double *coef, int *n_intervals);
/* host-only: the parameter rule of Stokes::setParams (PSEv1/Stokes.cc:129-236,319) without creating a handle */
int pse_host_select_params(const pse_params *params, pse_info *info);
/* host-only: the per-particle rows a pse_bonds object stores (pse_bonds_create calls this after validating).  A CSR over the n
 * particles: row i is entries[2 row_off[i]] .. entries[2 row_off[i + 1]), one (partner, type) pair of unsigned per bond end; every
 * bond appears in both endpoints' rows (duplicates as often as they are listed), each row sorted by (partner, type), so the rows
 * are a function of the bond SET, not of the list order or of the order of a bond's endpoints.  types == NULL: all type 0.
 * PSE_ERR_INVALID: a null array, n == 0, nbonds == 0 or > 2^30, an endpoint >= n, a bond with i == j. */
int pse_host_bond_rows(unsigned n, unsigned nbonds, const unsigned *pairs, const unsigned *types /* or NULL */,
                       int *row_off /* n + 1 */, unsigned *entries /* 2 nbonds x 2: partner, type */);
/* host-only: the per-particle rows a pse_angles object stores (pse_angles_create calls this after validating).  A CSR over the n
 * particles: row p is entries[4 row_off[p]] .. entries[4 row_off[p + 1]), one (i, j, k, type) quadruple of unsigned -- 16 bytes -- per
 * angle p takes part in, j the vertex and the ends swapped where needed so that i < k; p is one of i, j, k, which is its role.  Every
 * angle appears in the rows of all three of its particles (duplicates as often as they are listed), each row sorted by
 * (i, j, k, type), so the rows are a function of the angle SET, not of the list order or of which end is written first.
 * types == NULL: all type 0.  PSE_ERR_INVALID: a null array, n == 0, nangles == 0 or > 2^28 (3 nangles must fit the int
 * offsets), an index >= n, an angle with two equal members. */
int pse_host_angle_rows(unsigned n, unsigned nangles, const unsigned *triples, const unsigned *types /* or NULL */,
                        int *row_off /* n + 1 */, unsigned *entries /* 3 nangles x 4: i, j, k, type */);
/* host-only: the per-particle rows a pse_dihedrals object stores (pse_dihedrals_create calls this after validating).  A CSR over
 * the n particles, row p = entries row_off[p] .. row_off[p + 1) of TWO parallel sections of `entries`: the first holds one
 * (i, j, k, l) quadruple of unsigned -- 16 bytes, entry e at entries[4 e] -- per dihedral p takes part in, the second, which starts
 * at entries[16 ndihedrals], that entry's type at [e].  That is the 20 bytes of information per entry and no more: one aligned
 * 16-byte load and one 4-byte load, both consecutive along a row, and no bits of an index are given up to the type.  A quadruple is
 * stored as (l, k, j, i) where l < i, so that its first member is the smaller end; p is one of the four, which is its role.  Every
 * dihedral appears in the rows of all four of its particles (duplicates as often as they are listed), each row sorted by
 * (i, j, k, l, type), so the rows are a function of the dihedral SET, not of the list order or of the direction a quadruple is
 * written in.  types == NULL: all type 0.  PSE_ERR_INVALID: a null array, n == 0, ndihedrals == 0 or > 2^28 (4 ndihedrals must fit
 * the int offsets), an index >= n, a quadruple with two equal members. */
int pse_host_dihedral_rows(unsigned n, unsigned ndihedrals, const unsigned *quads, const unsigned *types /* or NULL */,
                           int *row_off /* n + 1 */, unsigned *entries /* 4 ndihedrals x 4: i, j, k, l; then 4 ndihedrals types */);
/* host-only: the per-particle rows a pse_exclusions object stores (pse_exclusions_create calls this after validating).  A CSR over
 * the n particles: row i is entries[row_off[i]] .. entries[row_off[i + 1]), the indices excluded from i, one unsigned each, sorted
 * ascending.  An exclusion is a set: a pair listed several times, in either order, is kept once; every pair appears in both members'
 * rows; row_off[n] is the number of entries kept (twice the number of distinct pairs, at most 2 npairs).  The rows are a function of
 * the pair SET, not of the list order or of the order of a pair's members.  PSE_ERR_INVALID: a null array, n == 0, npairs == 0 or
 * > 2^30, an index >= n, a pair with i == j. */
int pse_host_exclusion_rows(unsigned n, unsigned npairs, const unsigned *pairs, int *row_off /* n + 1 */,
                            unsigned *entries /* room for 2 npairs */);
/* host-only: where the tables of a typed pair table lie and what the kernel uses of each (pse_typed_table_create calls this).  For
 * the npt = ntypes (ntypes + 1)/2 pair types in the order p(a, b) of pse_typed_table_create: base[p] = the offset of table p in the
 * concatenated stage = the sum of the widths before it (an off pair type takes no room), scale[p] = (double)(width - 1)/(rmax - rmin)
 * -- the expression of pse_pair_table --, rmax2[p] = rmax rmax; scale and rmax2 are 0 for an off pair type (width 0), whose rmin and
 * rmax are not looked at.  *total = the sum of the widths.  PSE_ERR_INVALID: a null array, ntypes outside [1, 8], a width of 1, a
 * negative width or a width > 2048, all widths zero, a sum of widths > 3584, and for a pair type that is on: rmin or rmax not finite,
 * rmin < 0, rmax <= rmin.  Nothing is written after a refusal. */
int pse_host_typed_table_layout(int ntypes, const int *width, const double *rmin, const double *rmax,
                                int *base /* npt */, double *scale /* npt */, double *rmax2 /* npt */, int *total);
/* host-only: the layout a pse_molecules object stores (pse_molecules_create calls this after validating).  The MOLECULES are the
 * connected components of the bond graph with at least two particles, numbered by their smallest member, which is the ROOT;
 * mol_of[i] = the molecule of particle i, or -1 for a particle without a bond.  Per molecule a breadth-first SPANNING TREE from the root,
 * the neighbours visited in ascending index: `members` holds the caller indices of molecule after molecule in breadth-first order,
 * molecule mol at members[mol_off[mol]] .. members[mol_off[mol + 1]); parent[s] = the breadth-first POSITION (0 .. m - 1) of the parent
 * of the member in slot s, always smaller than its own position, the root being its own parent; depth[s] = its distance from the root
 * in tree edges.  Bonds that close rings are not tree edges: nring[mol] counts them, they are otherwise ignored.  A molecule is
 * LINEAR if it is a tree with exactly two members of degree 1 and all others of degree 2 (a dimer is): ends[2 mol], ends[2 mol + 1] =
 * the positions of the two, the one with the lower caller index first; 0xffffffff twice for any other molecule.  TILES: the molecules
 * are packed in order into tiles of at most PSE_MOL_TILE members, a molecule never straddles a tile and a tile is closed when the next
 * molecule does not fit: tile t holds the molecules tile_mol[t] .. tile_mol[t + 1), and tile_rounds[t] = ceil(log2(its largest depth + 1))
 * rounds of pointer jumping.  counts = (nmol, members in all, ntiles).  The layout is a function of the bond SET.
 * PSE_ERR_INVALID, in this order: a null array, n == 0, nbonds == 0 (no molecule at all) or > 2^30, in the order of the list an endpoint
 * >= n or a bond (i, i), a bond listed twice in either order, a molecule of more than PSE_MOL_TILE members. */
int pse_host_molecule_rows(unsigned n, unsigned nbonds, const unsigned *pairs, int *mol_of /* n */, unsigned *members /* n */,
                           unsigned *parent /* n */, unsigned *depth /* n */, unsigned *mol_off /* n / 2 + 1 */, unsigned *ends /* 2 (n / 2) */,
                           unsigned *nring /* n / 2 */, unsigned *tile_mol /* n / 2 + 1 */, unsigned *tile_rounds /* n / 2 */,
                           unsigned *counts /* 3 */);
/* The chain rank of every member slot of that layout (parent, mol_off and ends as pse_host_molecule_rows wrote them, nmol = counts[0]):
 * for a LINEAR molecule rank[slot] = the index 0 .. m - 1 along the chain, counted from ends[2 mol], the end with the lower caller
 * index; for any other molecule the breadth-first position.  A function of the bond SET.  PSE_ERR_INVALID: a null array. */
int pse_host_chain_order(unsigned nmol, const unsigned *parent, const unsigned *mol_off /* nmol + 1 */, const unsigned *ends /* 2 nmol */,
                         unsigned *rank /* one per member slot */);
/* host-only: the weights of pse_chain_modes_create for a linear chain of m members, nmodes rows of m doubles, row-major.  Row 0 is the
 * end-to-end functional (-1, 0, ..., 0, +1); rows p = 1 .. nmodes - 1 are the Rouse modes w_{p,q} = cos(pi p (2 q + 1) / (2 m)) / m.
 * The argument is reduced IN INTEGERS: j = p (2 q + 1) mod 4 m, the angle pi j / (2 m), folded into the first quadrant (j > 2 m:
 * j = 4 m - j; j > m: j = 2 m - j and the sign flips) before the one cos call; j == m gives exactly 0.  So w_{p,m-1-q} = -w_{p,q} bit
 * for bit for odd p and = w_{p,q} for even p.  PSE_ERR_INVALID, in this order: a null out, m < 2, nmodes outside [1,
 * PSE_CHAIN_MODES_MAX], nmodes - 1 >= m. */
int pse_host_rouse_weights(unsigned m, int nmodes, double *out /* nmodes x m */);

#ifdef __cplusplus
}
#endif
#endif /* PSE_AMD_H */
