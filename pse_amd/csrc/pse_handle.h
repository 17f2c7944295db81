// What the units of the C-ABI share (pse_engine.hip: the handle's life cycle; pse_capi.hip: the step driver and the teams;
// pse_objects.hip: the device objects and their passes): the handle, the owners of what it acquires, the error macros, the few
// functions that two units call and the base of the device objects.  Internal to those three units.
#pragma once
#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <type_traits>
#include <vector>

#include "../../include/pse_amd.h"
#include "pse_err.h"
#include "pse_host.h"
#include "pse_kernels.h"
#include "pse_farfield.h"
#include "pse_fft.h"
#include "pse_vectors.h"
#include "pse_local.h"

using namespace pse;

#define HIPCHK(x)                                                                                      \
    do {                                                                                               \
        hipError_t e_ = (x);                                                                           \
        if (e_ != hipSuccess) return fail(PSE_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define TRY(x)              \
    do {                    \
        int r_ = (x);       \
        if (r_) return r_;  \
    } while (0)

#define FFTCHK(x)                                                                                      \
    do {                                                                                               \
        rocfft_status s_ = (x);                                                                        \
        if (s_ != rocfft_status_success) return fail(PSE_ERR_FFT, "%s failed: rocfft status %d (%s:%d)", #x, (int)s_, __FILE__, __LINE__); \
    } while (0)

// The owners of what a handle, a team or a device object acquires, one per kind of resource.  A resource is registered where it is
// made, by the owner's make function, and released with the owner -- by release() or by the destructor, however far a create got.
struct DeviceArrays {
    DeviceArrays() = default;
    DeviceArrays(const DeviceArrays &) = delete;
    ~DeviceArrays() { release(); }
    hipError_t make(void **p, size_t bytes) {
        *p = nullptr;
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) v.push_back(*p);
        return e;
    }
    void replace(void *was, void *now) {   // `now` is owned in place of `was`, which goes back to the caller (place_grids)
        for (void *&q : v) if (q == was) q = now;
    }
    void release() { for (void *p : v) (void)hipFree(p); v.clear(); }
private:
    std::vector<void *> v;
};
struct PinnedBuffers {
    PinnedBuffers() = default;
    PinnedBuffers(const PinnedBuffers &) = delete;
    ~PinnedBuffers() { for (void *p : v) (void)hipHostFree(p); }
    hipError_t make(void **p, size_t bytes, unsigned flags = hipHostMallocDefault) {
        *p = nullptr;
        const hipError_t e = hipHostMalloc(p, bytes, flags);
        if (e == hipSuccess) v.push_back(*p);
        return e;
    }
    void drop(void *p) {   // one buffer ahead of the rest (a staging buffer that was outgrown); null: nothing
        for (size_t k = 0; k < v.size(); ++k) if (v[k] == p) { (void)hipHostFree(p); v.erase(v.begin() + k); return; }
    }
private:
    std::vector<void *> v;
};
struct Events {
    Events() = default;
    Events(const Events &) = delete;
    ~Events() { for (hipEvent_t e : v) (void)hipEventDestroy(e); }
    hipError_t make(hipEvent_t *ev, unsigned flags = hipEventDefault) {
        *ev = nullptr;
        const hipError_t e = hipEventCreateWithFlags(ev, flags);
        if (e == hipSuccess) v.push_back(*ev);
        return e;
    }
private:
    std::vector<hipEvent_t> v;
};
struct Streams {
    Streams() = default;
    Streams(const Streams &) = delete;
    ~Streams() { for (hipStream_t s : v) (void)hipStreamDestroy(s); }
    hipError_t make(hipStream_t *s, unsigned flags, const int *priority = nullptr) {   // priority null: the default one
        *s = nullptr;
        const hipError_t e = priority ? hipStreamCreateWithPriority(s, flags, *priority) : hipStreamCreateWithFlags(s, flags);
        if (e == hipSuccess) v.push_back(*s);
        return e;
    }
    void synchronize() { for (hipStream_t s : v) (void)hipStreamSynchronize(s); }
private:
    std::vector<hipStream_t> v;
};
struct FftPlans {   // rocFFT plans (double precision) and execution infos
    FftPlans() = default;
    FftPlans(const FftPlans &) = delete;
    ~FftPlans() { release(); }
    rocfft_status plan(rocfft_plan *p, rocfft_result_placement placement, rocfft_transform_type type, size_t dims, const size_t *len, size_t batch,
                       rocfft_plan_description desc) {
        *p = nullptr;
        const rocfft_status s = rocfft_plan_create(p, placement, type, rocfft_precision_double, dims, len, batch, desc);
        if (s == rocfft_status_success) plans.push_back(*p);
        return s;
    }
    rocfft_status info(rocfft_execution_info *i) {
        *i = nullptr;
        const rocfft_status s = rocfft_execution_info_create(i);
        if (s == rocfft_status_success) infos.push_back(*i);
        return s;
    }
    void release() {
        for (rocfft_plan p : plans) rocfft_plan_destroy(p);
        for (rocfft_execution_info i : infos) rocfft_execution_info_destroy(i);
        plans.clear(); infos.clear();
    }
private:
    std::vector<rocfft_plan> plans;
    std::vector<rocfft_execution_info> infos;
};

constexpr int PH_COUNT_ = 13;   // timed phases (enum PH_* below)

struct Phase {
    hipEvent_t a = nullptr, b = nullptr;
};
struct DeviceObject;

struct pse_handle {
    pse_params par;
    Derived d;
    Box box;
    DBox dbox;
    DGrid G;
    DCells nc;
    double cell_gamma;  // tilt bound the cell grid was sized for
    int device = 0;
    hipStream_t stream = nullptr;    // main chain: sort, near field, Lanczos, update (caller-visible ordering)
    hipStream_t wstream = nullptr;   // wave-space chain; == stream unless the two chains overlap (single GPU)
    hipStream_t side = nullptr;      // non-blocking stream behind wstream (an in-process team shares one among its members)
    hipStream_t side_owned = nullptr; // the one this handle made (streams)
    int *bounds_host = nullptr;      // pinned: slab row boundaries on their way back from the device
    hipEvent_t ev_bounds = nullptr;
    bool bounds_pending = false;
    // developer switches, read from the environment ONCE, in pse_create (nothing on the call path consults the environment)
    struct Tuning {
        int cell_bz = 6;          // PSE_CELL_BZ: height of the z blocks of the cell storage order (0: plain x, y, z order)
        double skin = 0.4;        // PSE_SKIN: r_buff of the neighbour list kept across calls (0: off)
        int overlap = 1;          // PSE_OVERLAP: 1 (default since round 6) two chains for every call, 0 only for kT = 0, -1 never
        bool no_xfuse = false;    // PSE_NO_XFUSE: rocFFT for the x pass
        int own_y_pow2 = 1;       // PSE_OWN_Y_POW2=0: rocFFT's 2-D transforms at Ny = 256 instead of its 1-D z pass + k_yfft_regs (A/B)
        int own_y = 1;            // PSE_OWN_Y=0: rocFFT's 2-D (y, z) transforms also where the own y pass applies
        int own_z = 1;            // PSE_OWN_Z=0: rocFFT's 1-D z transforms also where k_zfft_rows applies (A/B)
        int yslab_regs = 1;       // PSE_YSLAB_REGS=0: a slab rank's y pass at Ny = 256, 512 by k_fft_cols instead of k_yfft_regs (A/B)
        int yfft_kb = 4;          // PSE_YFFT_KB: kz columns per workgroup of the own y pass (2, 4, 8)
        int wave_mode = 0;        // PSE_WAVE_MODE: 0 automatic, 1 slab, 2 replicated
        int spread_tz = 0, spread_nw = 0;   // PSE_SPREAD_TZ, PSE_SPREAD_NW
        int gather_bz = 0;        // PSE_GATHER_BZ=1|2: bins along z per gather workgroup (0: by the particles per bin)
        int xmix_runtime = 0;     // PSE_XMIX=1: runtime radix plan of the mixed x pass also where a compile-time plan exists
        int xfft_small_wide = 0;  // PSE_XFFT_SMALL_KB=8: the eight-column x pass also on small grids
        bool verbose = false;     // PSE_VERBOSE
        bool team_sstep = true;      // PSE_TEAM_SSTEP=0: teams run one Lanczos iteration per exchange (default: two, see lanczos_team)
        int team_sched[3] = {1, 2, 3};   // PSE_TEAM_SCHED=a,b,c: far-field exchange k of a team step is issued before Lanczos exchange sched[k]
        int vq = 1;                  // PSE_VQ=0: the pair-list mat-vec gathers the neighbours' rows as doubles (two gathers per pair) (A/B)
        int place_trials = 10;       // PSE_PLACE_TRIALS=K: the two grids are allocated up to K times and the pair the x + inverse y + z passes run fastest on is kept (0, 1: off)
        int lz_extra = 2;            // PSE_LANCZOS_EXTRA: iterations a queue-only Brownian call queues beyond the starting count (gated on the device-side decision)
        int lz_op = PSE_LANCZOS_RECORDS16;   // PSE_LANCZOS_OP=fp64: the handle starts with the fp64 Lanczos operator (pse_set_lanczos_operator)
        int rows24 = 1;              // PSE_ROWS24=0: the Lanczos basis and the pair-list mat-vec results of a single GPU stay double4 (tests, bisecting)
    } tun;
    DCells bidx_nc = {0, 0, 0};      // cell grid the boundary-cell indices on the device belong to
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool overlap_all = false;   // fork also for Brownian steps (PSE_OVERLAP=1)
    bool side_on = false;       // this call runs the wave chain on the side stream
    hipEvent_t ev_scal = nullptr;   // the Lanczos scalars have reached the pinned host buffer
    int n_max = 0, n_pad = 0;
    // sorted particle state
    unsigned *keys = nullptr, *keys_s = nullptr, *vals = nullptr, *perm = nullptr, *tag_s = nullptr;
    void *sort_tmp = nullptr;
    int *cell_cnt = nullptr;
    size_t sort_tmp_bytes = 0;
    int *cell_off = nullptr;
    double *pv_rows = nullptr;   // pse_pair_repulsion_virial: one row of eight partial sums per workgroup of its cell pass
    std::vector<DeviceObject *> topologies;   // the bond, angle and dihedral objects created on this handle and still alive (pse_destroy frees them)
    // what the handle has acquired, at create or later (the fp64 plane of the pair list, the buffers of the redistribution): every
    // device array (dmalloc), pinned buffer, event, stream, rocFFT plan and execution info named below belongs to one of these
    DeviceArrays arrays;
    FftPlans fft;
    PinnedBuffers pinned;
    Streams streams;
    Events events;
    int *cnt_block = nullptr; // [far-field bin counts | the two flags of the kept neighbour list | cell counts]: zeroed by ONE memset per call
    size_t cnt_bins = 0;      // ints of the bin counts (incl. the sentinel)
    SpreadWork sw = {};       // far-field bins and the bin-ordered particle records (origins, prefac * force, separable weights)
    NbList nb = {};              // nb.c64 = nb64 while the fp64 Lanczos operator is selected, else null
    double4 *nb64 = nullptr;     // the fp64 plane of the pair list (allocated when the mode is first selected)
    int lz_op = PSE_LANCZOS_RECORDS16;
    bool nb_valid = false;   // the pair list matches the current sorted positions
    bool lz_last_queued = false;   // the most recent Brownian call took its Lanczos decision on the device (pse_get_info then reads the host mirror)
    // neighbour list kept across steps (HOOMD's NeighborList with r_buff and a distance check every step, PSEv1/integrate.py:60,79)
    double skin = 0.0;           // r_buff; 0: cell walk every step
    double skin_max = 0.0;       // what the cell grid and the list capacity were sized for
    VerletList vl = {};
    double4 *pos_build = nullptr;   // sorted positions at the build
    int *flags_host = nullptr;      // pinned copy of vl.flags
    bool vl_valid = false;       // the list on the device belongs to the current order (perm) and box
    bool vl_use = false;         // this call runs on the kept list (no sort, no cell walk)
    bool vl_pending = false;     // this call's first cell pass writes the list
    int vl_N = 0; const unsigned *vl_group = nullptr; Box vl_box = {};
    bool nc_wide = false;        // the cell grid in use is the one sized for rcut + skin_max
    unsigned long long nlist_builds = 0, nlist_reuses = 0;
    // A list that is never reused costs a wider cell grid and its own writes at every build: after two builds in a row whose
    // list failed its first distance check (particles diffuse more than r_buff / 2 per call) the list is suspended for a while
    // -- builds then run exactly as with r_buff = 0 -- and tried again, with the pause doubling while it keeps failing.
    // Kept per kind of call -- [1]: integrating steps (pse_step), [0]: evaluations (pse_mobility, pse_brownian_velocity, ...): a
    // time-stepping loop that outruns the skin must not switch the list off for evaluations repeated at fixed positions.
    int vl_reused_since_build = 0, vl_misses[2] = {0, 0}, vl_suspend_left[2] = {0, 0}, vl_suspend_len[2] = {32, 32};
    int vl_kind = 0;             // kind of the call being prepared
    bool pv_is_f = false;        // the vector half of pv mirrors f_s (as the permute wrote it)
    bool w_is_mpsi = false;  // w_s already holds M_real psi_s (delivered by the pass that built the pair list)
    bool sums0_done = false; // ... and scal[LZ_TMP ..] the sums psi.psi, psi.M psi of Lanczos iteration 0
    CombineSink sink = {};   // where the final Lanczos combination of this call sends its rows (velocity() sets it; off: ub_s)
    bool tail_done = false;  // ... and it did: the sum of the three contributions has reached its destination
    bool async_mode = false; // pse_set_async: deterministic evaluations queue their work and return -- no flag read-back, capturable
    bool gated = false;      // this call decides between the kept list and a rebuild ON THE DEVICE: both chains are queued (gate_word)
    int *gate_word = nullptr;   // (cnt_block): flags[0] | flags[1] of this call, read by the kernels of both chains
    size_t n_cells_alloc = 0;
    float4 *posf_s = nullptr;   // single-precision copy of pos_s (cutoff pre-filter of the near field)
    double2 *pv = nullptr;      // [N][3] packed (position, force) records gathered by the drain of the near-field passes
    double4 *pos_s = nullptr, *f_s = nullptr, *uw_s = nullptr, *ur_s = nullptr, *ub_s = nullptr, *psi_s = nullptr, *w_s = nullptr;
    // real-space table
    double *coef = nullptr;
    int n_intervals = 0;
    // grids
    double *rgrid = nullptr;     // [3][nxl][Ny][Nz]
    double2 *cgrid = nullptr;    // [3][nxl][Ny][Nzh]
    rocfft_plan plan_fwd = nullptr, plan_inv = nullptr;      // single GPU: 3-D real transforms, batch 3
    rocfft_plan plan_x_fwd = nullptr, plan_x_inv = nullptr;  // slab mode: 1-D complex transforms along x (strided, in place)
    rocfft_execution_info info_fwd = nullptr, info_inv = nullptr;
    // slab decomposition (n_slabs > 1): x planes [x0, x0+nxl) of the real grid, y rows [y0, y0+nyl) of the transposed spectrum
    int n_slabs = 1, slab_rank = 0, nyl = 0, y0 = 0;
    double2 *sendbuf = nullptr, *recvbuf = nullptr;          // [3][n_slabs][nxl][nyl][Nzh] each
    int *d_bidx = nullptr, *d_bounds = nullptr;              // slab mode: cell indices / row offsets of the cell-slab boundaries
    std::vector<int> row_lo, first_end, last_begin;          // per rank: own rows [row_lo[r], row_lo[r+1]), first / last cell layer
    std::vector<int> first2_end, last2_begin;                // ... and its first / last TWO cell layers (two-step Lanczos of a team)
    double4 *w2_s = nullptr, *u_s = nullptr;                 // two-step Lanczos: w2 = M M v_j, u = M v_{j-1}
    double *sums_all = nullptr;                              // [n_slabs][LZ_NGRAM]: every rank's partial Lanczos sums (they travel with the ghost rows)
    double4 *utot_s = nullptr;                               // slab mode: summed velocity of the own rows, all-gathered
    bool xfuse = false;                                      // power-of-two Nx: fused x pass (k_xfft_scale)
    bool own_y = false;                                      // y transforms by k_fft_cols, rocFFT does the z transforms only
    bool own_y_slab = false;                                 // ... on a slab rank, with the all-to-all block layout as its output / input
    int lz_extra = -1;           // pse_set_lanczos_extra: gated iterations a queue-only call queues beyond its starting count (-1: PSE_LANCZOS_EXTRA)
    void *vq = nullptr;          // [n] 16-byte mirror of the newest Lanczos vector (single GPU; k_lz_update writes it, the pair-list mat-vec gathers from it)
    int place_tried = 0; float place_ms_first = 0, place_ms_kept = 0;   // place_grids: pairs tried, the probe's time on the first and on the kept one
    bool own_z = false;                                      // z transforms by k_zfft_rows (Nz = 256, 512): rocFFT is then off the path
    double2 *twiddle_z = nullptr;                            // [Nz] exp(-2 pi i m / Nz) (== twiddle when Nz == Nx)
    double2 *twiddle_y = nullptr;                            // [Ny] exp(-2 pi i m / Ny) (== twiddle when Ny == Nx)
    int grid_slabs = 1;   // slabs the far-field grid is cut into: n_slabs, or 1 when every rank keeps the whole grid
    double2 *twiddle = nullptr;                              // [Nx] exp(-2 pi i m / Nx)
    void *fft_work = nullptr;
    size_t fft_work_bytes = 0;
    // Lanczos
    double4 *V = nullptr;        // [M_MAX + 1][n_max] double4 rows -- or, rows24, as many rows of three doubles (lz_vec in pse_capi.hip knows)
    // Decided once, in pse_create: single GPU, a pair list, the records operator at create, PSE_ROWS24 != 0.  Then V[j >= 1] and w24 hold
    // 24-byte rows (pse_device.h): only k_lz_update, k_mreal_list and k_basis_combine touch them, each told the layout per pointer.
    bool rows24 = false;
    double *w24 = nullptr;       // rows24: [n_max][3], the results of the pair-list mat-vecs of the iteration, in the basis' unused slot 0 (the
                                 // build pass's M psi stays in w_s)
    double *scal = nullptr, *partials = nullptr;
    double *lz_sums = nullptr;   // [2][LZ_NPART] partial sums of x_{j+1}.x_{j+1}, x_{j+1}.x_j a k_lz_update leaves for iteration j + 1 (pse_vectors.h)
    double *sc_host = nullptr;   // pinned host copy of scal, mapped: the Lanczos kernels write alpha, beta, the norm there as well
    double *sc_host_dev = nullptr;   // its device address
    int *bounds_host_dev = nullptr;  // device address of bounds_host (mapped pinned): k_pick writes the row boundaries straight to the host
    int npart_cap = 0;
    // owned-particle rank (pse_params.local_rows; pse_local.h): geometry, capacities and the buffers of the step's first exchange
    struct LocalPlan {
        bool on = false;
        LocalGeom g{};
        int rows_cap = 0;                    // c_own + 2 c_g
        double *send[2] = {nullptr, nullptr}, *recv[2] = {nullptr, nullptr};   // [left, right] messages: LOCAL_HDR + LOCAL_REC * c_x doubles
        size_t msg = 0;                      // doubles per message
        double4 *stage_w1 = nullptr, *stage_w2 = nullptr;   // the last layers of w1, w2 on their way to the right neighbour (c_g rows each)
        double4 *porig_s = nullptr; double *mass_s = nullptr; int3 *image_s = nullptr;
        LocalRows *rows = nullptr;           // device
        int *counters = nullptr;             // (inside cnt_block: zeroed with the cell counts)
        int *layer_cnt = nullptr;            // (likewise) kept particles per x layer of the cell grid: LOCAL_MAX_LAYERS ints
        size_t zero_ints = 0;                // ints of cnt_block a step starts from zero
        bool zeroed = false;                 // the last step's k_local_finish has cleared them (else: a memset in front of the step)
        int *err = nullptr, *err_host = nullptr;   // error word: device, and a pinned word the status call copies it to
        // pse_team_redistribute_local (allocated at its first call): records out / in (c_own each), the destination of every particle,
        // the ranks' count rows [G][row] (row = G counts, the rank's capacity, its particle count; an even number of ints), send offsets + fill counters
        double *rd_send = nullptr, *rd_recv = nullptr;
        int *rd_rows = nullptr, *rd_off = nullptr, *rd_host = nullptr;
    } loc;
    LzState *lz_state = nullptr;     // the device-side Lanczos decision of queue-only Brownian calls (pse_set_async)
    unsigned long long lz_seq = 0;   // calls that queued one (the decision kernel stamps the host mirror with it)
    const uint32_t *ts_off = nullptr;   // pse_set_timestep_offset: the noise of a Brownian call is drawn at timestep + *ts_off
    // bookkeeping
    pse_info info;
    bool timing = false;
    Phase ph[PH_COUNT_];
    unsigned long long bytes = 0;
    int sorted_N = 0;
    bool matvec_timed = false;
};

// *p = a device array of n T (n = 0: of one) that the handle owns and counts in its bytes
template <class T>
int dmalloc(pse_handle *h, T **p, size_t n) {
    if (n == 0) n = 1;
    const hipError_t e = h->arrays.make((void **)p, n * sizeof(T));
    if (e != hipSuccess) return fail(PSE_ERR_HIP, "hipMalloc((void **)p, n * sizeof(T)) failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
    h->bytes += n * sizeof(T);
    return 0;
}
// pse_engine.hip, called by the driver too: the cell grid of a box, and the rocFFT execution infos bound to h->wstream
int cells_for(const Box &box, double rc, double gamma, int n_slabs, int bz_want, DCells &out, int xpad = 0);
int bind_wave_stream(pse_handle *h);
// pse_capi.hip, called by pse_create too
ScaleArgs scale_args(pse_handle *h, bool noise, double kT, double dt, unsigned timestep, double xi = 0.0, double eta = 0.0);
bool team_sstep(const pse_handle *h);
void roctx_lookup();   // PSE_ROCTX, read once per process
// The sort, the cell list and the sorted copies of a call's arrays (pse_capi.hip, which also holds the default arguments)
struct PrepExtra { bool psi; unsigned timestep; };   // psi: the pass also draws the particle noise of this step into psi_s
int prepare(pse_handle *h, const double4 *pos, const double4 *vec, const unsigned *group, int N, bool defer_bounds, bool need_cells, PrepExtra px,
            bool with_real);


// A device object of the C-ABI (pse_objects.hip).  It belongs to the handle it was created on, which deletes what is still alive in
// pse_destroy, and it owns the device arrays that put() made: they are freed with it, however far a create got.
struct DeviceObject {
    pse_handle *h = nullptr;
    hipError_t err = hipSuccess;   // the first failure of a put()
    size_t bytes = 0;              // asked for so far
    bool zeroed = false;           // a put() zeroed memory (hipMemset on the null stream, which may return early)
    DeviceObject() = default;
    virtual ~DeviceObject() = default;
    // *dst = a device array of n T: a copy of the host's `src`; src null: zeroed with `zero`, else as allocated.  Returns the first
    // failure of this object: once one put() has failed, the later ones do nothing.
    template <class T>
    hipError_t put(T **dst, const std::remove_const_t<T> *src, size_t n, bool zero = false) {
        *dst = nullptr;
        if (err != hipSuccess) return err;
        void *p = nullptr;
        bytes += n * sizeof(T);
        if ((err = arrays.make(&p, n * sizeof(T))) != hipSuccess) return err;
        *dst = (T *)p;
        if (src) err = hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
        else if (zero) { err = hipMemset(p, 0, n * sizeof(T)); zeroed = true; }
        return err;
    }
private:
    DeviceArrays arrays;
};
