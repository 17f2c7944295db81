// C-ABI of the PSE engine (include/pse_amd.h): the step driver that replaces
// gpu_stokes_step_one / gpu_stokes_CombinedMobilityBrownian_wrap / gpu_stokes_BrealLanczos_wrap
// (PSEv1/Stokes.cu:234-365, PSEv1/Brownian.cu:772-923, PSEv1/Brownian.cu:357-765).
//
// Differences from the reference driver that are deliberate: all workspaces are allocated once
// in pse_create (the reference cudaMalloc/cudaFree's ~109 N Scalar4 every step); Lanczos scalars stay on the
// device and the host is consulted only at convergence checks; wave vectors are computed inside the scaling
// kernel; failures are returned, never exit()ed.  The handle's life cycle (pse_create ... pse_destroy) is in pse_engine.hip, the
// device objects (bonds ... cluster links) and the entry points of their passes are in pse_objects.hip; the handle, which the
// three units see, is in pse_handle.h.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocfft/rocfft.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/pse_amd.h"
#include "pse_err.h"
#include "pse_host.h"
#include "pse_kernels.h"
#include "pse_farfield.h"
#include "pse_fft.h"
#include "pse_vectors.h"
#include "pse_forces.h"
#include "pse_handle.h"

using namespace pse;

// the 16-byte mirror of the Lanczos vector, where the mat-vec reads it (records mode; the fp64 operator gathers the rows as doubles)
static void *vq_of(const pse_handle *h) { return h->nb.c64 ? nullptr : h->vq; }

enum { PH_SORT, PH_SPREAD, PH_FFTF, PH_SCALE, PH_FFTI, PH_GATHER, PH_REAL, PH_LANCZOS, PH_INTEG, PH_COMM, PH_TOTAL, PH_MATVEC, PH_RECORDS, PH_COUNT };
// Phase ranges for rocprofv3 --marker-trace (PSE_ROCTX=1): host-side roctx ranges around the launches of each phase (the
// reference has one HOOMD Profiler push/pop around the whole step, PSEv1/Stokes.cc:450-451,519-521).  libroctx64 is
// looked up at run time: no link dependency, nothing happens unless the switch is set.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        const char *e = getenv("PSE_ROCTX");
        if (!e || !atoi(e)) return;
        void *lib = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) return;
        push = (int (*)(const char *))dlsym(lib, "roctxRangePushA");
        pop = (int (*)())dlsym(lib, "roctxRangePop");
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
static const Roctx &roctx() { static Roctx r; return r; }
void roctx_lookup() { (void)roctx(); }
static_assert(PH_COUNT == PH_COUNT_, "phase table");
static const char *const PH_NAME[PH_COUNT] = {"pse:sort", "pse:spread", "pse:fft_forward", "pse:kspace_scale", "pse:fft_inverse", "pse:gather",
                                              "pse:near_field", "pse:lanczos", "pse:integrate", "pse:exchange", "pse:total", "pse:matvec",
                                              "pse:far_records"};
static void range_push(int p) { if (roctx().push) roctx().push(PH_NAME[p]); }
static void range_pop() { if (roctx().pop) roctx().pop(); }
static int ts(pse_handle *h, int p) { range_push(p); if (h->timing) HIPCHK(hipEventRecord(h->ph[p].a, h->stream)); return 0; }
static int te(pse_handle *h, int p) { if (h->timing) HIPCHK(hipEventRecord(h->ph[p].b, h->stream)); range_pop(); return 0; }
static int tsw(pse_handle *h, int p) { range_push(p); if (h->timing) HIPCHK(hipEventRecord(h->ph[p].a, h->wstream)); return 0; }
static int tew(pse_handle *h, int p) { if (h->timing) HIPCHK(hipEventRecord(h->ph[p].b, h->wstream)); range_pop(); return 0; }

static int collect_times(pse_handle *h, unsigned mask) {
    if (!h->timing) return 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->side) HIPCHK(hipStreamSynchronize(h->side));
    double *dst[PH_COUNT] = {&h->info.t_sort, &h->info.t_spread, &h->info.t_fft_fwd, &h->info.t_scale, &h->info.t_fft_inv,
                             &h->info.t_gather, &h->info.t_real, &h->info.t_lanczos, &h->info.t_integrate, &h->info.t_comm,
                             &h->info.t_total, &h->info.t_matvec, &h->info.t_records};
    for (int p = 0; p < PH_COUNT; ++p) {
        *dst[p] = 0.0;
        if (mask & (1u << p)) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, h->ph[p].a, h->ph[p].b) == hipSuccess) *dst[p] = ms;
        }
    }
    return 0;
}

extern "C" int pse_debug_last_gate(pse_handle *h, int *gate) {
    if (!h || !gate) return fail(PSE_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    *gate = -1;
    if (h->gated) HIPCHK(hipMemcpy(gate, h->gate_word, sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

// ---- team: the SPMD driver ---------------------------------------------------------------------------------------
// A team is the set of slab ranks this process drives.  Production multi-GPU: one rank per process, team of one
// member, data moved between processes by RCCL on the member's stream.  In-process loopback: all n_slabs ranks are
// members of one team on one device (used to test the decomposition on a single GPU); the "collectives" are device
// copies.  A single GPU is a team of one with n_slabs = 1 and no communication.  Every phase below runs for all local
// members, then the exchange; the phase code is identical in the three cases.
struct pse_team {
    PinnedBuffers pinned;        // what the team has acquired (pse_handle.h); released with it: events, then the stream, then the staging
    Streams streams;
    Events events;
    std::vector<pse_handle *> m;
    int G = 1;                   // ranks in the decomposition
    ncclComm_t nccl = nullptr;   // set when members.size() == 1 and G > 1: ONE communicator for every exchange of the team
    // ... and ONE stream all its RCCL calls are issued on, in program order -- the same order on every rank (SPMD code, host-side
    // decisions taken from identical all-reduced numbers).  The two compute lanes (main: sort, near field, Lanczos, update; side:
    // the far-field chain) hand their buffers to it and take them back through events, so the lanes overlap while no two
    // collectives of one communicator are ever in flight in an order that could differ between ranks.
    hipStream_t comm = nullptr;
    std::vector<hipEvent_t> evs; // ring of events for those hand-overs
    size_t ev_next = 0;
    pse_transport cb = {};       // or: a transport supplied by the host program (host-staged; pse_team_create_transport)
    bool has_cb = false;
    double *stage = nullptr;     // pinned staging of the callback transport
    size_t stage_n = 0;
    // developer switch (pse_team_debug_solo): an in-process team queues the work of ONE member only -- its kernels on both lanes,
    // the copies that stand for what it receives -- so that the wall time of a call is that rank's critical path on a GPU of its
    // own (the other members' buffers keep what the last full call left there: the numbers are not meaningful, the timing is)
    int solo = -1;
    std::vector<pse_handle *> solo_m;
    bool lanes = true;           // two compute lanes (PSE_TEAM_LANES=0: one stream for everything, also the RCCL calls)
    int lz_extra = -1;           // pse_team_set_lanczos_extra: iterations an owned-particle step queues beyond its starting count (-1: the members' PSE_LANCZOS_EXTRA)
    bool debug_sync = getenv("PSE_DEBUG_SYNC") != nullptr;   // (read once, when the team is created)
    // self-diagnosis (pse_team_set_diag): every exchange of a call bracketed by events on the lane that issues it, the lanes'
    // spans, the host time the transport's callback took -- read after the call by pse_team_get_diag
    struct Diag {
        bool on = false;
        std::vector<hipEvent_t> ev;          // 2 per exchange slot + 4 for the lanes
        int n = 0;                           // exchanges of the last call
        int kind[PSE_DIAG_MAX]; int lane[PSE_DIAG_MAX]; double host_us[PSE_DIAG_MAX]; unsigned long long bytes[PSE_DIAG_MAX];
        bool side_used = false;
    } diag;
};
enum { DIAG_FIRST = 0, DIAG_LANCZOS = 1, DIAG_ALL_TO_ALL = 2, DIAG_HALO = 3, DIAG_ALL_GATHER = 4, DIAG_GHOST = 5 };
// brackets one exchange with two events on the stream of the lane that issues it (and measures the host time in between)
struct DiagScope {
    pse_team &T; int slot = -1; hipStream_t s; std::chrono::steady_clock::time_point t0;
    DiagScope(pse_team &team, int kind, bool wave_lane, unsigned long long bytes) : T(team) {
        if (!T.diag.on || T.diag.n >= PSE_DIAG_MAX || T.G == 1) return;
        pse_handle *h = T.solo >= 0 ? T.solo_m[0] : T.m[0];
        s = wave_lane ? h->wstream : h->stream;
        slot = T.diag.n++;
        T.diag.kind[slot] = kind; T.diag.lane[slot] = wave_lane ? 1 : 0; T.diag.bytes[slot] = bytes; T.diag.host_us[slot] = 0.0;
        (void)hipEventRecord(T.diag.ev[2 * slot], s);
        t0 = std::chrono::steady_clock::now();
    }
    ~DiagScope() {
        if (slot < 0) return;
        T.diag.host_us[slot] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        (void)hipEventRecord(T.diag.ev[2 * slot + 1], s);
    }
};
static const std::vector<pse_handle *> &act(const pse_team &T) { return T.solo >= 0 ? T.solo_m : T.m; }
#define NCCLCHK(x)                                                                                              \
    do {                                                                                                        \
        ncclResult_t r_ = (x);                                                                                  \
        if (r_ != ncclSuccess) return fail(PSE_ERR_COMM, "%s failed: %s (%s:%d)", #x, ncclGetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

static bool loopback(const pse_team &T) { return T.G > 1 && !T.nccl && !T.has_cb; }
static bool remote(const pse_team &T) { return T.nccl || T.has_cb; }   // one member per process
static hipEvent_t team_event(pse_team &T) { hipEvent_t e = T.evs[T.ev_next]; T.ev_next = (T.ev_next + 1) % T.evs.size(); return e; }

static void diag_mark(pse_team &T, int which, hipStream_t s) {   // 0 / 1 main lane begin / end, 2 / 3 far-field lane begin / end
    if (T.diag.on) (void)hipEventRecord(T.diag.ev[2 * PSE_DIAG_MAX + which], s);
    if (T.diag.on && which == 2) T.diag.side_used = true;
}
static void diag_begin(pse_team &T) {
    if (!T.diag.on) return;
    T.diag.n = 0; T.diag.side_used = false;
    diag_mark(T, 0, (T.solo >= 0 ? T.solo_m[0] : T.m[0])->stream);
}
// One exchange of a process-per-rank team: a list of point-to-point transfers (counts in doubles; 0 = none) -- ONE RCCL group, or one
// call of the host program's transport.  Every exchange of the team goes through here -- also the partial sums of the Lanczos
// iteration, which travel as small blocks to every rank in the group of the ghost rows (no collective of another kind is ever
// posted) -- so what the RCCL path sends (buffers, counts, peers, order) is exactly what the callback transport sends -- and that
// one runs between real processes in the tests (two ranks cannot share a GPU under RCCL).
struct Xfer { const double *send; size_t ns; int to; double *recv; size_t nr; int from; };
static int team_exchange(pse_team &T, const std::vector<Xfer> &ops, bool wave_lane) {
    pse_handle *h = T.m[0];
    hipStream_t s = wave_lane ? h->wstream : h->stream;
    const int me = h->slab_rank;
    // a rank's sends to itself and its receives from itself pair up in order (the all-to-all's diagonal block): local copies in
    // every transport (nothing of the exchange depends on how a library treats a send to the calling rank)
    std::vector<const Xfer *> self_send, self_recv;
    for (const Xfer &x : ops) {
        if (x.ns && x.to == me) self_send.push_back(&x);
        if (x.nr && x.from == me) self_recv.push_back(&x);
    }
    if (self_send.size() != self_recv.size()) return fail(PSE_ERR_COMM, "unpaired self transfer");
    for (size_t q = 0; q < self_send.size(); ++q) {
        if (self_send[q]->ns != self_recv[q]->nr) return fail(PSE_ERR_COMM, "self transfer of unequal sizes");
        if (self_recv[q]->recv != self_send[q]->send)
            HIPCHK(hipMemcpyAsync(self_recv[q]->recv, self_send[q]->send, self_send[q]->ns * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    bool any = false;
    for (const Xfer &x : ops) any = any || (x.ns && x.to != me) || (x.nr && x.from != me);
    if (!any) return 0;
    if (T.nccl) {
        ncclComm_t comm = T.nccl;
        // hand-over lane -> communication stream (what the lane has queued so far produces the buffers) ...
        hipStream_t cs = T.comm ? T.comm : s;
        if (T.comm) { hipEvent_t e = team_event(T); HIPCHK(hipEventRecord(e, s)); HIPCHK(hipStreamWaitEvent(T.comm, e, 0)); }
        NCCLCHK(ncclGroupStart());
        ncclResult_t bad = ncclSuccess;   // a failing call must not leave the library inside an open group
        for (const Xfer &x : ops) if (bad == ncclSuccess && x.ns && x.to != me) bad = ncclSend(x.send, x.ns, ncclDouble, x.to, comm, cs);
        for (const Xfer &x : ops) if (bad == ncclSuccess && x.nr && x.from != me) bad = ncclRecv(x.recv, x.nr, ncclDouble, x.from, comm, cs);
        const ncclResult_t end = ncclGroupEnd();
        if (bad != ncclSuccess || end != ncclSuccess)
            return fail(PSE_ERR_COMM, "RCCL exchange failed: %s", ncclGetErrorString(bad != ncclSuccess ? bad : end));
        // ... and back: the lane goes on when the exchange has completed
        if (T.comm) { hipEvent_t e = team_event(T); HIPCHK(hipEventRecord(e, T.comm)); HIPCHK(hipStreamWaitEvent(s, e, 0)); }
        return 0;
    }
    // host-staged transport: device -> pinned host, the host program moves the bytes, pinned host -> device
    size_t need = 0;
    for (const Xfer &x : ops) need += (x.to == me ? 0 : x.ns) + (x.from == me ? 0 : x.nr);
    if (need > T.stage_n) {
        T.pinned.drop(T.stage);
        T.stage = nullptr; T.stage_n = 0;
        HIPCHK(T.pinned.make((void **)&T.stage, (need + 1024) * sizeof(double)));
        T.stage_n = need + 1024;
    }
    std::vector<pse_host_xfer> hx;
    size_t off = 0;
    std::vector<std::pair<double *, const double *>> back;   // (device destination, host source) of what arrives
    std::vector<size_t> back_n;
    for (const Xfer &x : ops) {
        pse_host_xfer e{};
        if (x.ns && x.to != me) { e.send = T.stage + off; e.send_count = x.ns; e.send_to = x.to; HIPCHK(hipMemcpyAsync(T.stage + off, x.send, x.ns * sizeof(double), hipMemcpyDeviceToHost, s)); off += x.ns; }
        if (x.nr && x.from != me) { e.recv = T.stage + off; e.recv_count = x.nr; e.recv_from = x.from; back.push_back({x.recv, T.stage + off}); back_n.push_back(x.nr); off += x.nr; }
        if (e.send_count || e.recv_count) {
            if (!e.send_count) e.send_to = -1;
            if (!e.recv_count) e.recv_from = -1;
            hx.push_back(e);
        }
    }
    HIPCHK(hipStreamSynchronize(s));
    if (!hx.empty() && T.cb.exchange(T.cb.user, (int)hx.size(), hx.data())) return fail(PSE_ERR_COMM, "transport: exchange failed");
    for (size_t q = 0; q < back.size(); ++q)
        HIPCHK(hipMemcpyAsync(back[q].first, back[q].second, back_n[q] * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // the staging buffer is reused by the next exchange
    return 0;
}

// the device copies of an in-process exchange, batched into as few launches as the argument space allows
struct CopyBatch {
    CopyList l{};
    hipStream_t s;
    explicit CopyBatch(hipStream_t st) : s(st) { l.n = 0; }
    void add(double *dst, const double *src, size_t n) {
        if (!n || dst == src) return;
        while (n) {   // counts are 32-bit
            const size_t c = std::min<size_t>(n, 0x40000000u);
            l.src[l.n] = src; l.dst[l.n] = dst; l.cnt[l.n] = (unsigned)c;
            if (++l.n == 40) flush();
            src += c; dst += c; n -= c;
        }
    }
    void flush() { if (l.n) launch_copy_list(l, s); l.n = 0; }
    ~CopyBatch() { flush(); }
};

// all-to-all of equal blocks, nset sets at once (one group): member r sends block q of set c of send(r) to rank q,
// which stores it as block r of set c of recv(q); sets are set_stride doubles apart
template <class FS, class FR>
static int team_all_to_all(pse_team &T, FS send, FR recv, size_t blk_doubles, int nset, size_t set_stride) {
    if (T.G == 1) return 0;
    DiagScope dg(T, DIAG_ALL_TO_ALL, true, (unsigned long long)nset * (T.G - 1) * blk_doubles * sizeof(double));
    if (remote(T)) {
        pse_handle *h = T.m[0];
        std::vector<Xfer> ops;
        for (int c = 0; c < nset; ++c)
            for (int q = 0; q < T.G; ++q)
                ops.push_back(Xfer{send(h) + c * set_stride + (size_t)q * blk_doubles, blk_doubles, q,
                                   recv(h) + c * set_stride + (size_t)q * blk_doubles, blk_doubles, q});
        return team_exchange(T, ops, true);
    }
    CopyBatch cb(act(T)[0]->wstream);   // an in-process team shares one stream per lane
    for (int c = 0; c < nset; ++c)
        for (pse_handle *src : T.m)
            for (pse_handle *dst : act(T))
                cb.add(recv(dst) + c * set_stride + (size_t)src->slab_rank * blk_doubles,
                       send(src) + c * set_stride + (size_t)dst->slab_rank * blk_doubles, blk_doubles);
    return 0;
}
// gather halo: every rank stores copies of its left neighbour's last hl planes below its slab and of its right
// neighbour's first nhalo planes above it
static int team_halo_exchange(pse_team &T) {
    if (T.G == 1) return 0;
    DiagScope dg(T, DIAG_HALO, true, (unsigned long long)3 * (T.m[0]->G.hl + T.m[0]->G.nhalo) * T.m[0]->G.Ny * T.m[0]->G.Nz * sizeof(double));
    auto comp = [](pse_handle *h, int c) { return h->rgrid + (size_t)c * (h->G.nxl + h->G.hl + h->G.nhalo) * h->G.Ny * h->G.Nz; };
    if (remote(T)) {
        pse_handle *h = T.m[0];
        const DGrid &G = h->G;
        const size_t plane = (size_t)G.Ny * G.Nz;
        const int left = (h->slab_rank + T.G - 1) % T.G, right = (h->slab_rank + 1) % T.G;
        std::vector<Xfer> ops;
        for (int c = 0; c < 3; ++c) {
            double *own = comp(h, c) + plane * G.hl;
            // my first planes go left and arrive above the left neighbour's slab; my last planes go right and arrive below the right one's
            ops.push_back(Xfer{own, plane * G.nhalo, left, own + plane * G.nxl, plane * G.nhalo, right});
            ops.push_back(Xfer{own + plane * (G.nxl - G.hl), plane * G.hl, right, comp(h, c), plane * G.hl, left});
        }
        return team_exchange(T, ops, true);
    }
    auto member = [&](int r) { for (pse_handle *h : T.m) if (h->slab_rank == r) return h; return (pse_handle *)nullptr; };
    CopyBatch cb(act(T)[0]->wstream);
    for (pse_handle *dst : act(T)) {
        const DGrid &G = dst->G;
        const size_t plane = (size_t)G.Ny * G.Nz;
        pse_handle *L = member((dst->slab_rank + T.G - 1) % T.G), *R = member((dst->slab_rank + 1) % T.G);
        for (int c = 0; c < 3; ++c) {
            cb.add(comp(dst, c) + plane * (G.hl + G.nxl), comp(R, c) + plane * G.hl, plane * G.nhalo);
            cb.add(comp(dst, c), comp(L, c) + plane * (G.hl + G.nxl - G.hl), plane * G.hl);
        }
    }
    return 0;
}

// ghost rows of distributed vectors: for every buffer, a rank receives its right neighbour's first `depth` cell layers and its left
// neighbour's last `depth` layers (the near-field mat-vec of the own rows reads one layer besides the own rows; the two-step
// Lanczos block keeps two).  Row numbers are global, so a block lands at the position it was sent from.
static std::vector<Xfer> ghost_ops(const pse_handle *h, int G, std::initializer_list<double *> bufs, int depth = 1) {
    const std::vector<int> &lo = h->row_lo;
    const std::vector<int> &fe = depth == 1 ? h->first_end : h->first2_end, &lb = depth == 1 ? h->last_begin : h->last2_begin;
    auto cnt = [](int a, int b) { return (size_t)std::max(0, b - a) * 4; };
    const int r = h->slab_rank, L = (r + G - 1) % G, R = (r + 1) % G;
    std::vector<Xfer> ops;
    for (double *buf : bufs) {
        if (!buf) continue;
        // my first layers go left (the left neighbour's right ghost), my last layers go right
        ops.push_back(Xfer{buf + (size_t)lo[r] * 4, cnt(lo[r], fe[r]), L, buf + (size_t)lo[R] * 4, cnt(lo[R], fe[R]), R});
        ops.push_back(Xfer{buf + (size_t)lb[r] * 4, cnt(lb[r], lo[r + 1]), R, buf + (size_t)lb[L] * 4, cnt(lb[L], lo[L + 1]), L});
    }
    return ops;
}
// The partial Lanczos sums of a rank (n numbers at scal[LZ_TMP ..]) go to every rank -- point-to-point blocks in the SAME group as the
// ghost rows (round 4: no separate all-reduce collective; the kernels that consume the sums add the ranks' blocks in rank order)
static void sum_ops(const pse_handle *h, int G, int n, std::vector<Xfer> &ops) {
    for (int q = 0; q < G; ++q)
        ops.push_back(Xfer{h->scal + LZ_TMP, (size_t)n, q, h->sums_all + (size_t)q * LZ_NGRAM, (size_t)n, q});
}
// An exchange given as one transfer list per rank (+ an optional sum over the ranks), in any of the three transports.  In-process
// teams execute the receives as device copies: the k-th receive of dst from src pairs with the k-th send of src to dst -- the
// matching rule of the message transports.
template <class FOPS>
static int team_run_exchange(pse_team &T, FOPS make_ops, bool wave_lane, int kind = DIAG_GHOST) {
    if (T.G == 1) return 0;
    unsigned long long bytes = 0;
    if (T.diag.on) for (const Xfer &x : make_ops(T.solo >= 0 ? T.solo_m[0] : T.m[0])) bytes += (unsigned long long)x.ns * sizeof(double);
    DiagScope dg(T, kind, wave_lane, bytes);
    if (remote(T)) return team_exchange(T, make_ops(T.m[0]), wave_lane);
    std::vector<std::vector<Xfer>> all(T.G);
    for (pse_handle *h : T.m) all[h->slab_rank] = make_ops(h);
    CopyBatch cb(wave_lane ? act(T)[0]->wstream : act(T)[0]->stream);
    for (pse_handle *dst : act(T)) {
        const int d = dst->slab_rank;
        std::vector<size_t> taken(T.G, 0);   // sends of each source already paired with a receive of dst
        for (const Xfer &rx : all[d]) {
            if (!rx.nr) continue;
            const std::vector<Xfer> &so = all[rx.from];
            size_t &k = taken[rx.from];
            while (k < so.size() && !(so[k].ns && so[k].to == d)) ++k;
            if (k == so.size() || so[k].ns != rx.nr) return fail(PSE_ERR_COMM, "in-process exchange: unmatched transfer");
            cb.add(rx.recv, so[k].send, rx.nr);
            ++k;
        }
    }
    return 0;
}
template <class FB>
static int team_ghost_exchange(pse_team &T, FB buf) {
    return team_run_exchange(T, [&](pse_handle *h) { return ghost_ops(h, T.G, {buf(h)}); }, false);
}

// One exchange per Lanczos iteration: the three partial sums (all-reduce) and the ghost rows of y = M x (every rank receives its
// right neighbour's first cell layer and its left neighbour's last one) travel in ONE group.
template <class FB>
static int team_lanczos_exchange(pse_team &T, FB buf) {
    return team_run_exchange(T, [&](pse_handle *h) { auto ops = ghost_ops(h, T.G, {buf(h)}); sum_ops(h, T.G, 3, ops); return ops; }, false, DIAG_LANCZOS);
}

// every rank's own rows [row_lo[r], row_lo[r+1]) of buf become visible on every rank (blocks of different sizes)
template <class FB>
static int team_all_gather_rows(pse_team &T, FB buf) {
    if (T.G == 1) return 0;
    const std::vector<int> &lo = T.m[0]->row_lo;
    DiagScope dg(T, DIAG_ALL_GATHER, false, (unsigned long long)(T.G - 1) * (lo[T.m[0]->slab_rank + 1] - lo[T.m[0]->slab_rank]) * 32ull);
    if (remote(T)) {
        pse_handle *h = T.m[0];
        const int r = h->slab_rank;
        std::vector<Xfer> ops;
        for (int q = 0; q < T.G; ++q)
            if (q != r)
                ops.push_back(Xfer{buf(h) + (size_t)lo[r] * 4, (size_t)(lo[r + 1] - lo[r]) * 4, q,
                                   buf(h) + (size_t)lo[q] * 4, (size_t)(lo[q + 1] - lo[q]) * 4, q});
        return team_exchange(T, ops, false);
    }
    CopyBatch cb(act(T)[0]->stream);
    for (pse_handle *src : T.m)
        for (pse_handle *dst : act(T))
            if (src != dst) {
                const int r = src->slab_rank;
                cb.add(buf(dst) + (size_t)lo[r] * 4, buf(src) + (size_t)lo[r] * 4, (size_t)(lo[r + 1] - lo[r]) * 4);
            }
    return 0;
}

// ---- phases ---------------------------------------------------------------------------------------------------
static int check_n(pse_handle *h, unsigned N) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    if (N == 0 || (int)N > h->n_max) return fail(PSE_ERR_INVALID, "N = %u outside (0, n_max = %d]", N, h->n_max);
    HIPCHK(hipSetDevice(h->device));
    return 0;
}

// rows of the particle arrays this rank owns: the particles of its cell slab (contiguous in the cell-sorted order)
static void row_range(const pse_handle *h, int N, int &lo, int &hi) {
    if (h->n_slabs == 1) { lo = 0; hi = N; return; }
    lo = h->row_lo[h->slab_rank]; hi = h->row_lo[h->slab_rank + 1];
}

// after the sort: where the cell slabs begin in the sorted arrays (3G+1 ints; identical on every rank because the particle
// arrays are replicated).  The copy back is issued here and awaited only where the host first needs the numbers -- after the
// far-field chain has been queued, so the GPU does not idle meanwhile.
static int slab_bounds_issue(pse_handle *h) {
    const int G = h->n_slabs;
    if (G == 1) return 0;
    const int layer = h->nc.nzb * h->nc.ny * h->nc.bz, per = h->nc.nx / G;   // storage cells of one x layer
    std::vector<int> idx(5 * G + 1);
    for (int r = 0; r <= G; ++r) idx[r] = r * per * layer;
    for (int r = 0; r < G; ++r) {
        idx[G + 1 + r] = (r * per + 1) * layer;                       // end of the first layer, begin of the last
        idx[2 * G + 1 + r] = ((r + 1) * per - 1) * layer;
        idx[3 * G + 1 + r] = (r * per + std::min(2, per)) * layer;    // ... of the first / last two layers
        idx[4 * G + 1 + r] = ((r + 1) * per - std::min(2, per)) * layer;
    }
    if (h->bidx_nc.nx != h->nc.nx || h->bidx_nc.ny != h->nc.ny || h->bidx_nc.nz != h->nc.nz) {   // once per cell grid
        HIPCHK(hipStreamSynchronize(h->stream));
        HIPCHK(hipMemcpy(h->d_bidx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
        h->bidx_nc = h->nc;
    }
    launch_pick(h->cell_off, h->d_bidx, (int)idx.size(), h->bounds_host_dev, h->stream);   // straight into the mapped host buffer: no copy to queue
    HIPCHK(hipEventRecord(h->ev_bounds, h->stream));
    h->bounds_pending = true;
    return 0;
}
static int slab_bounds_wait(pse_handle *h, int N) {
    if (!h->bounds_pending) return 0;
    h->bounds_pending = false;
    const int G = h->n_slabs;
    HIPCHK(hipEventSynchronize(h->ev_bounds));
    const int *out = h->bounds_host;
    h->row_lo.assign(out, out + G + 1);
    h->first_end.assign(out + G + 1, out + 2 * G + 1);
    h->last_begin.assign(out + 2 * G + 1, out + 3 * G + 1);
    h->first2_end.assign(out + 3 * G + 1, out + 4 * G + 1);
    h->last2_begin.assign(out + 4 * G + 1, out + 5 * G + 1);
    if (h->row_lo[0] != 0 || h->row_lo[G] != N) return fail(PSE_ERR_NUMERIC, "inconsistent cell offsets after the sort");
    return 0;
}

// Two Lanczos iterations per exchange (lanczos_team): needs the pair list, the table in LDS (the pass that builds the list then
// delivers M psi with it), at least two cell layers per rank and two ghost layers on either side that are not the rank's own.
bool team_sstep(const pse_handle *h) {
    const int G = h->n_slabs, per = h->nc.nx / std::max(1, G);
    return G > 1 && h->tun.team_sstep && h->w2_s && h->nb.cap > 0 && mreal_table_in_lds(h->n_intervals * 2 * RS_NCOEF) && per >= 2 &&
           h->nc.nx >= per + 4;
}

// What a slab rank orders, gathers into cell order and keeps particle data for: its own cell layers and one ghost layer on either
// side (CellRanges in pse_kernels.h).  Everything, when the far field is replicated on every rank, when the slab and its ghosts
// cover all layers anyway, or when a support could reach further than a ghost layer is wide (a particle beyond the ghost layer
// must not touch the slab's planes: (P/2 + 1) node planes against the width of a cell layer).
static CellRanges slab_need(const pse_handle *h) {
    CellRanges r{};
    const int G = h->n_slabs, nx = h->nc.nx;
    if (G == 1 || h->grid_slabs == 1) return r;
    const int per = nx / G, layer = h->nc.nzb * h->nc.ny * h->nc.bz;
    const int depth = team_sstep(h) ? 2 : 1;   // ghost layers kept on either side
    if (per + 2 * depth >= nx) return r;
    if ((h->G.P / 2 + 1.0) / h->G.Nx > 1.0 / nx) return r;
    const int start = ((h->slab_rank * per - depth) % nx + nx) % nx, len = per + 2 * depth;
    if (start + len <= nx) { r.n = 1; r.c0[0] = start * layer; r.c1[0] = (start + len) * layer; }
    else { r.n = 2; r.c0[0] = start * layer; r.c1[0] = nx * layer; r.c0[1] = 0; r.c1[1] = (start + len - nx) * layer; }
    return r;
}

// bin + sort + gather into cell order (positions change every step, so this runs every call; every rank COUNTS all particles
// -- the state is replicated and the row offsets are global -- but orders and gathers only what slab_need() says)
// need_cells: the caller walks the cell list itself (pair repulsion): sort even if the neighbour list could be kept.
//
// With a neighbour skin the sort and the cell walk run only when the distance check says so (the reference keeps HOOMD's
// NeighborList with r_buff = 0.4 and setEvery(1, dist_check), PSEv1/integrate.py:60,79, and calls m_nlist->compute every
// step, Stokes.cc:433): the particles are gathered into the order of the last sort, every one is compared with where it
// was at the build, and one flag comes back to the host.  Kept: perm, the neighbour list; rebuilt as before: the far-field
// records, the per-step (f, h) pair list.
int prepare(pse_handle *h, const double4 *pos, const double4 *vec, const unsigned *group, int N, bool defer_bounds = false,
            bool need_cells = false, PrepExtra px = PrepExtra{false, 0}, bool with_real = true) {
    TRY(ts(h, PH_SORT));
    const FarBinArgs far = far_bin_args(h->G, h->sw);
    double4 *psi_out = px.psi ? h->psi_s : nullptr;
    h->nb_valid = false;
    h->w_is_mpsi = false; h->sums0_done = false;
    h->vl_use = false;
    h->vl_pending = false;
    h->pv_is_f = vec != nullptr && h->pv != nullptr;
    const bool same_box = h->vl_box.Lx == h->box.Lx && h->vl_box.Ly == h->box.Ly && h->vl_box.Lz == h->box.Lz && h->vl_box.xy == h->box.xy;
    h->gated = false;
    // (only when the call has a near-field part: the rebuild chain's list and build positions are written by real(); a far-field-only
    // call that took it would leave a list in the OLD order marked valid -- such a call rebuilds, ungated)
    if (h->async_mode && with_real && !px.psi && h->skin > 0.0 && h->vl_valid && !need_cells && h->vl_N == N && h->vl_group == group && same_box &&
        h->sorted_N == N && h->nc_wide && h->n_slabs == 1) {
        // Asynchronous mode, a deterministic evaluation, a kept list exists: the decision "reuse or rebuild" is taken on the device and
        // BOTH chains are queued -- the kernels of the chain not taken read the gate word and leave at once.  No read-back, nothing
        // host-side depends on the outcome, so the call can be captured into a hipGraph and replayed with any positions.
        //   ungated: gather into the order of the last build + distance check -> flags; decide -> gate word
        //   rebuild chain (gate != 0): zero the bin and cell counts, cell sort, gather into the new order, [real(): cell pass that
        //                              writes the list, positions of the build]
        //   reuse chain (gate == 0):   [real(): the kept-list pass]
        const int ncell = cells_total(h->nc);
        HIPCHK(hipMemsetAsync(h->cnt_block, 0, h->cnt_bins * sizeof(int), h->stream));   // bin counts + flags[0]
        launch_permute(pos, vec, group, h->perm, N, h->dbox, h->pos_s, h->posf_s, h->pv, h->f_s, h->tag_s, h->stream,
                       h->pos_build, 0.25 * h->skin * h->skin, h->vl.flags, CellRanges{}, nullptr, &far, nullptr, 0, 0);
        launch_gate_decide(h->vl.flags, h->gate_word, h->stream);
        const Gate rb{h->gate_word, 1};
        launch_gate_zero(rb, h->cnt_block, h->cnt_bins - 1, h->cell_cnt, (size_t)ncell + 1, h->stream);   // (not the flags)
        HIPCHK(cell_sort(pos, group, N, h->dbox, h->nc, h->keys, h->vals, h->keys_s, h->cell_cnt, ncell, h->sort_tmp, h->sort_tmp_bytes,
                         h->cell_off, h->perm, h->stream, CellRanges{}, SlabBook{}, true, rb));
        launch_permute(pos, vec, group, h->perm, N, h->dbox, h->pos_s, h->posf_s, h->pv, h->f_s, h->tag_s, h->stream, nullptr, 0.0, nullptr,
                       CellRanges{}, h->cell_off, &far, nullptr, 0, 0, rb);
        h->gated = true;
        h->vl.rskin = h->d.rcut + h->skin;
        h->sw.need = CellRanges{}; h->sw.cell_off = h->cell_off;
        ++h->nlist_builds;   // (counted as a build: which chain ran is known on the device only)
        TRY(te(h, PH_SORT));
        HIPCHK(hipGetLastError());
        return 0;
    }
    if (h->skin > 0.0 && !h->async_mode && h->vl_valid && !need_cells && h->vl_N == N && h->vl_group == group && same_box && h->sorted_N == N) {
        HIPCHK(hipMemsetAsync(h->cnt_block, 0, h->cnt_bins * sizeof(int), h->stream));   // bin counts + flags[0] ([1] is the build's overflow mark)
        launch_permute(pos, vec, group, h->perm, N, h->dbox, h->pos_s, h->posf_s, h->pv, h->f_s, h->tag_s, h->stream,
                       h->pos_build, 0.25 * h->skin * h->skin, h->vl.flags, CellRanges{}, nullptr, &far, psi_out, h->par.seed, px.timestep, Gate{}, h->ts_off);
        HIPCHK(hipMemcpyAsync(h->flags_host, h->vl.flags, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->flags_host[0] == 0 && h->flags_host[1] == 0) {
            h->vl_use = true;
            ++h->nlist_reuses;
            ++h->vl_reused_since_build;
            h->vl_misses[h->vl_kind] = 0; h->vl_suspend_len[h->vl_kind] = 32;
            TRY(te(h, PH_SORT));
            return 0;
        }
        const int q = h->vl_kind;
        if (h->vl_reused_since_build == 0 && ++h->vl_misses[q] >= 2) {   // built twice for nothing: pause
            h->vl_suspend_left[q] = h->vl_suspend_len[q];
            h->vl_suspend_len[q] = std::min(2 * h->vl_suspend_len[q], 4096);
            h->vl_misses[q] = 1;                                     // one more miss after the pause suspends again
        }
    }
    h->vl_valid = false;
    ++h->nlist_builds;
    // (asynchronous mode: no host-side feedback, hence no suspension logic -- deterministic evaluations always keep the list, for the
    // device-side decision of the next call; Brownian calls, which cannot take that path, do not)
    const bool with_list = h->skin > 0.0 && (h->async_mode ? !px.psi : h->vl_suspend_left[h->vl_kind] == 0);
    if (h->skin > 0.0 && !h->async_mode && !with_list) --h->vl_suspend_left[h->vl_kind];
    if (h->skin_max > 0.0) {   // cells as wide as this build reaches: rcut + r_buff with the list, rcut without
        const bool wide = h->nc_wide;
        if (wide != with_list) {
            DCells nc;
            TRY(cells_for(h->box, h->d.rcut + (with_list ? h->skin_max : 0.0), h->cell_gamma, h->n_slabs, h->tun.cell_bz, nc));
            h->nc = nc; h->nc_wide = with_list;
            h->info.ncell_x = nc.nx; h->info.ncell_y = nc.ny; h->info.ncell_z = nc.nz;
        }
    }
    const int ncell = cells_total(h->nc);
    if ((size_t)ncell > h->n_cells_alloc)   // pse_create and pse_set_box check both cell grids: cannot happen, must not pass silently
        return fail(PSE_ERR_INVALID, "cell grid %d x %d x %d exceeds the capacity sized at creation", h->nc.nx, h->nc.ny, h->nc.nz);
    const CellRanges need = slab_need(h);
    h->sw.need = need; h->sw.cell_off = h->cell_off;
    SlabBook sb{};
    if (need.n > 0 && h->n_slabs <= 64) {   // where the particles of the layers this rank does not keep are counted (cell_sort)
        auto kept = [&](int c) { for (int q = 0; q < need.n; ++q) if (c >= need.c0[q] && c < need.c1[q]) return true; return false; };
        const int layer = h->nc.nzb * h->nc.ny * h->nc.bz, per = h->nc.nx / h->n_slabs;
        sb.n = h->n_slabs; sb.cells_per_slab = per * layer; sb.spread = std::max(1, std::min(1024, layer));
        for (int q = 0; q < h->n_slabs; ++q) {
            sb.book[q] = q * per * layer;   // (a slab kept whole has no foreign particles: never used)
            for (int l = 0; l < per; ++l)
                if (!kept((q * per + l) * layer)) { sb.book[q] = (q * per + l) * layer; break; }
        }
    }
    // one memset: the bin counts, both flags of the kept list, the cell counts (+ the sentinel)
    HIPCHK(hipMemsetAsync(h->cnt_block, 0, ((h->cnt_bins + 4 + (size_t)ncell + 1 + 3) & ~(size_t)3) * sizeof(int), h->stream));   // (rounded up into the padding)
    HIPCHK(cell_sort(pos, group, N, h->dbox, h->nc, h->keys, h->vals, h->keys_s, h->cell_cnt, ncell, h->sort_tmp, h->sort_tmp_bytes,
                     h->cell_off, h->perm, h->stream, need, sb, true));
    launch_permute(pos, vec, group, h->perm, N, h->dbox, h->pos_s, h->posf_s, h->pv, h->f_s, h->tag_s, h->stream, nullptr, 0.0, nullptr,
                   need, h->cell_off, &far, psi_out, h->par.seed, px.timestep, Gate{}, h->ts_off);
    h->sorted_N = N;
    if (with_list) {   // the first cell pass of this call writes the list (real())
        h->vl_pending = true; h->vl_N = N; h->vl_group = group;
        h->vl.rskin = h->d.rcut + h->skin;
        h->vl_reused_since_build = 0;
    }
    TRY(slab_bounds_issue(h));
    if (!defer_bounds) TRY(slab_bounds_wait(h, N));
    TRY(te(h, PH_SORT));
    HIPCHK(hipGetLastError());
    return 0;
}

// xi, eta > 0: the operator with these in place of the handle's own (pse_debug_wave_grid; a step never passes them)
ScaleArgs scale_args(pse_handle *h, bool noise, double kT, double dt, unsigned timestep, double xi, double eta) {
    ScaleArgs a;
    const DGrid &G = h->G;
    a.xi = xi > 0.0 ? xi : h->d.xi; a.eta = eta > 0.0 ? eta : h->d.eta; a.noise = noise ? 1 : 0;
    a.noise_fac = noise ? std::sqrt(2.0 * kT / dt / (G.hx * G.hy * G.hz)) : 0.0;   // PSEv1/Brownian.cu:197
    a.seed = h->par.seed; a.timestep = timestep; a.ts_off = h->ts_off;
    a.transposed = h->grid_slabs > 1 ? 1 : 0; a.y0 = h->y0; a.nyl = h->grid_slabs > 1 ? h->nyl : G.Ny;
    a.runtime_plan = h->tun.xmix_runtime; a.wide_small = h->tun.xfft_small_wide;
    return a;
}

// wave-space part: spread -> FFT -> scale (+ noise) -> inverse FFT -> gather  (PSEv1/Brownian.cu:836-872), cut where a
// slab-decomposed team exchanges data: compute part k, exchange k, compute part k + 1, ...
//   part 0  records, spread, 2-D forward transforms (+ pack)         exchange 0  all-to-all (y rows of every x plane -> their rank)
//   part 1  x transforms + k-space scaling (+ noise)                 exchange 1  all-to-all back
//   part 2  (unpack +) 2-D inverse transforms                        exchange 2  plane halo of the gather
//   part 3  gather
// A single GPU, or a team that keeps the whole grid on every rank, has no exchanges: the parts simply follow one another.
struct WaveArgs { int N; bool noise; double kT, dt; unsigned timestep; double xi = 0.0, eta = 0.0; /* > 0: operator overrides (debug) */ };
// the forward transforms of part 0 (+ a slab rank's pack): real grids -> half spectra, z and y (single GPU with rocFFT's 3-D plan: x too)
static int wave_forward_transforms(pse_handle *h, int GS) {
    const DGrid &G = h->G;
    const size_t nr = (size_t)(G.nxl + G.hl + G.nhalo) * G.Ny * G.Nz, ncx = (size_t)G.nxl * G.Ny * G.Nzp;
    TRY(tsw(h, PH_FFTF));
    double *zr[3]; double2 *zs[3];   // the rows of the own planes of each component
    for (int c = 0; c < 3; ++c) { zr[c] = h->rgrid + c * nr + (size_t)G.hl * G.Ny * G.Nz; zs[c] = h->cgrid + c * ncx; }
    if (GS == 1) {
        if (h->own_z) launch_zfft(zr, zs, G.Nx * G.Ny, G.Nz, G.Nzp, false, h->twiddle_z, h->wstream);
        else {
            void *in[1] = {h->rgrid}, *out[1] = {h->cgrid};
            FFTCHK(rocfft_execute(h->plan_fwd, in, out, h->info_fwd));
        }
        if (h->own_y) launch_yfft(h->cgrid, G, false, h->twiddle_y, h->wstream, h->tun.yfft_kb);
    } else {
        if (h->own_z) launch_zfft(zr, zs, G.nxl * G.Ny, G.Nz, G.Nzp, false, h->twiddle_z, h->wstream);
        else for (int c = 0; c < 3; ++c) {   // 2-D (y,z) transforms of the local planes, one component at a time
            void *in[1] = {h->rgrid + c * nr + (size_t)G.hl * G.Ny * G.Nz}, *out[1] = {h->cgrid + c * ncx};
            FFTCHK(rocfft_execute(h->plan_fwd, in, out, h->info_fwd));
        }
        if (h->own_y_slab) launch_yfft_slab(h->cgrid, h->sendbuf, G, h->nyl, false, h->twiddle_y, h->wstream, h->tun.yslab_regs > 0);
        else launch_slab_pack(h->cgrid, h->sendbuf, G.nxl, G.Ny, G.Nzp, h->nyl, 0, h->wstream);
    }
    TRY(tew(h, PH_FFTF));
    return 0;
}
static int wave_compute(pse_team &T, const WaveArgs &a, int part) {
    const int GS = T.m[0]->grid_slabs;   // 1: every rank transforms the whole grid (single GPU, or a team that replicates it)
    for (pse_handle *h : act(T)) {
        const DGrid &G = h->G;
        const size_t nr = (size_t)(G.nxl + G.hl + G.nhalo) * G.Ny * G.Nz, ncx = (size_t)G.nxl * G.Ny * G.Nzp;
        if (part == 0) {
            double *gx = h->rgrid, *gy = h->rgrid + nr, *gz = h->rgrid + 2 * nr;
            TRY(tsw(h, PH_RECORDS));
            HIPCHK(launch_far_records(h->pos_s, h->f_s, a.N, G, h->dbox, h->sw, h->wstream));
            TRY(tew(h, PH_RECORDS));
            TRY(tsw(h, PH_SPREAD));
            if (spread_needs_zero(G)) HIPCHK(hipMemsetAsync(h->rgrid, 0, 3 * nr * sizeof(double), h->wstream));
            HIPCHK(launch_spread(h->pos_s, h->f_s, a.N, gx, gy, gz, G, h->dbox, h->sw, h->wstream));
            TRY(tew(h, PH_SPREAD));
            TRY(wave_forward_transforms(h, GS));
        } else if (part == 1) {
            double2 *sp = GS == 1 ? h->cgrid : h->recvbuf;   // [3][Nx][nyl][Nzh] after the transpose
            TRY(tsw(h, PH_SCALE));
            const ScaleArgs sa = scale_args(h, a.noise, a.kT, a.dt, a.timestep, a.xi, a.eta);
            if (h->xfuse) {
                launch_xfft_scale(sp, sp + ncx, sp + 2 * ncx, G, h->dbox, sa, h->twiddle, h->wstream);
            } else {
                if (GS > 1)
                    for (int c = 0; c < 3; ++c) { void *io[1] = {sp + c * ncx}; FFTCHK(rocfft_execute(h->plan_x_fwd, io, nullptr, h->info_fwd)); }
                launch_scale(sp, sp + ncx, sp + 2 * ncx, G, h->dbox, sa, h->wstream);
                if (GS > 1)
                    for (int c = 0; c < 3; ++c) { void *io[1] = {sp + c * ncx}; FFTCHK(rocfft_execute(h->plan_x_inv, io, nullptr, h->info_inv)); }
            }
            TRY(tew(h, PH_SCALE));
        } else if (part == 2) {
            TRY(tsw(h, PH_FFTI));
            double *zr[3]; double2 *zs[3];
            for (int c = 0; c < 3; ++c) { zr[c] = h->rgrid + c * nr + (size_t)G.hl * G.Ny * G.Nz; zs[c] = h->cgrid + c * ncx; }
            if (GS == 1) {
                if (h->own_y) launch_yfft(h->cgrid, G, true, h->twiddle_y, h->wstream, h->tun.yfft_kb);
                if (h->own_z) launch_zfft(zr, zs, G.Nx * G.Ny, G.Nz, G.Nzp, true, h->twiddle_z, h->wstream);
                else {
                    void *in[1] = {h->cgrid}, *out[1] = {h->rgrid};
                    FFTCHK(rocfft_execute(h->plan_inv, in, out, h->info_inv));
                }
            } else {
                if (h->own_y_slab) launch_yfft_slab(h->cgrid, h->sendbuf, G, h->nyl, true, h->twiddle_y, h->wstream, h->tun.yslab_regs > 0);
                else launch_slab_pack(h->cgrid, h->sendbuf, G.nxl, G.Ny, G.Nzp, h->nyl, 1, h->wstream);
                if (h->own_z) launch_zfft(zr, zs, G.nxl * G.Ny, G.Nz, G.Nzp, true, h->twiddle_z, h->wstream);
                else for (int c = 0; c < 3; ++c) {
                    void *in[1] = {h->cgrid + c * ncx}, *out[1] = {h->rgrid + c * nr + (size_t)G.hl * G.Ny * G.Nz};
                    FFTCHK(rocfft_execute(h->plan_inv, in, out, h->info_inv));
                }
            }
            TRY(tew(h, PH_FFTI));
        } else {
            TRY(tsw(h, PH_GATHER));
            HIPCHK(launch_gather(h->pos_s, h->sw, a.N, h->rgrid, h->rgrid + nr, h->rgrid + 2 * nr, G, h->dbox, h->uw_s, h->wstream));
            TRY(tew(h, PH_GATHER));
            // every particle was gathered by the rank that owns its row (zeros elsewhere)
        }
    }
    return 0;
}
static int wave_exchange(pse_team &T, int k) {
    pse_handle *h0 = T.m[0];
    if (h0->grid_slabs == 1) return 0;
    const size_t blk = (size_t)h0->G.nxl * h0->nyl * h0->G.Nzp * 2, comp = blk * h0->grid_slabs;
    if (k == 0) {
        for (pse_handle *h : act(T)) TRY(tsw(h, PH_COMM));
        TRY(team_all_to_all(T, [&](pse_handle *h) { return (double *)h->sendbuf; }, [&](pse_handle *h) { return (double *)h->recvbuf; }, blk, 3, comp));
        for (pse_handle *h : act(T)) TRY(tew(h, PH_COMM));
        return 0;
    }
    if (k == 1)
        return team_all_to_all(T, [&](pse_handle *h) { return (double *)h->recvbuf; }, [&](pse_handle *h) { return (double *)h->sendbuf; }, blk, 3, comp);
    return team_halo_exchange(T);
}
// The far-field chain as the main lane's driver sees it: compute parts are queued as early as the data allows, exchange k of the
// chain is ISSUED when the driver reaches its slot -- just before Lanczos exchange number slot[k] -- so that the order of the
// collectives on the team's one communication stream is a fixed interleaving of the two lanes, the same on every rank.
struct WavePump {
    pse_team *T = nullptr;
    WaveArgs a{};
    int next = 4;                   // next compute part to queue (4: the chain is complete, or not part of this call)
    int slot[3] = {0, 0, 0};
    unsigned *mask = nullptr;
    bool forked = false;
    // the side lane may start from here (the sorted arrays exist); what the caller queues on the main lane afterwards runs NEXT to the chain
    int fork(pse_team &team) {
        for (pse_handle *h : act(team))
            if (h->side_on) {
                HIPCHK(hipEventRecord(h->ev_fork, h->stream));
                HIPCHK(hipStreamWaitEvent(h->side, h->ev_fork, 0));
                if (h == act(team)[0]) diag_mark(team, 2, h->side);
            }
        forked = true;
        return 0;
    }
    int start(pse_team &team, const WaveArgs &args, const int sched[3], unsigned *m) {
        T = &team; a = args; mask = m;
        for (int k = 0; k < 3; ++k) slot[k] = sched[k];
        if (!forked) TRY(fork(team));
        *mask |= (1u << PH_SPREAD) | (1u << PH_FFTF) | (1u << PH_SCALE) | (1u << PH_FFTI) | (1u << PH_GATHER) | (1u << PH_RECORDS);
        if (T->m[0]->grid_slabs > 1) *mask |= 1u << PH_COMM;
        TRY(wave_compute(*T, a, 0));
        next = 1;
        if (T->m[0]->grid_slabs == 1) return upto(1 << 30);   // no exchanges: the whole chain is queued at once
        return 0;
    }
    // called before Lanczos exchange e is issued (and with a huge e to finish the chain)
    int upto(int e) {
        while (T && next <= 3 && slot[next - 1] <= e) {
            TRY(wave_exchange(*T, next - 1));
            TRY(wave_compute(*T, a, next));
            ++next;
        }
        return 0;
    }
    int drain() { return upto(1 << 30); }
};

// rows of a rank with `depth` ghost cell layers on either side: its own rows first, then its left neighbour's last layers and its
// right neighbour's first layers (duplicates dropped: with two ranks and one layer each, both ghosts are the same rows)
static int row_ranges(const pse_handle *h, int N, int depth, int rg[3][2]) {
    if (h->n_slabs == 1) { rg[0][0] = 0; rg[0][1] = N; return 1; }
    const int G = h->n_slabs, r = h->slab_rank, L = (r + G - 1) % G, R = (r + 1) % G;
    int n = 0;
    auto add = [&](int a, int b) {
        if (b <= a) return;
        for (int q = 0; q < n; ++q) if (rg[q][0] == a && rg[q][1] == b) return;
        rg[n][0] = a; rg[n][1] = b; ++n;
    };
    rg[0][0] = h->row_lo[r]; rg[0][1] = h->row_lo[r + 1]; n = 1;   // the own rows are range 0 even when empty (list rows start there)
    if (depth >= 1) {
        add((depth == 1 ? h->last_begin : h->last2_begin)[L], h->row_lo[L + 1]);
        add(h->row_lo[R], (depth == 1 ? h->first_end : h->first2_end)[R]);
    }
    return n;
}
static RowMap rank_rows(const pse_handle *h, int N, int depth) {
    int rg[3][2];
    const int n = row_ranges(h, N, depth, rg);
    return row_map(rg, n);
}

// near-field mat-vec out = M_real vec (PSEv1/Mobility.cu:594-687) on the rows this rank owns (+ `depth` ghost layers); vec must be
// valid on those rows and on the cell layer beyond them.  build_list: also record the pair list for later mat-vecs of this step.
static int real(pse_team &T, double4 *pse_handle::*vec, double4 *pse_handle::*out, size_t vec_off, size_t out_off, int N,
                bool build_list, bool with_psi = false, int depth = 0) {
    for (pse_handle *h : act(T)) {
        h->w_is_mpsi = false;
        int mode = MREAL_CELLS;
        if (h->nb.cap > 0) {
            if (h->nb_valid) mode = MREAL_USE_LIST;
            else if (build_list) mode = MREAL_BUILD_LIST;
        }
        // the kept neighbour list: used when this call runs on it, written by the first cell pass after a sort
        int vlm = VL_NONE;
        if (h->vl_use) vlm = VL_USE;
        else if (h->vl_pending && mode != MREAL_USE_LIST) vlm = VL_WRITE;
        const double4 *v = h->*vec + vec_off;
        if (h->gated && mode == MREAL_CELLS) {   // both chains, gated on the device-side decision of prepare()
            const RowMap rows = rank_rows(h, N, 0);
            const int nco = h->n_intervals * 2 * RS_NCOEF;
            const Gate rb{h->gate_word, 1}, ru{h->gate_word, 0};
            launch_mreal(h->pos_s, h->posf_s, v, h->*out + out_off, rows, h->cell_off, h->dbox, h->nc, h->d.rcut, h->d.self, h->coef, nco,
                         h->nb, MREAL_CELLS, h->stream, nullptr, nullptr, h->vl, VL_WRITE, nullptr, nullptr, 0, nullptr, rb);
            launch_gate_copy(rb, h->pos_build, h->pos_s, (size_t)N, h->stream);
            launch_mreal(h->pos_s, h->posf_s, v, h->*out + out_off, rows, h->cell_off, h->dbox, h->nc, h->d.rcut, h->d.self, h->coef, nco,
                         h->nb, MREAL_CELLS, h->stream, nullptr, nullptr, h->vl, VL_USE,
                         v == h->f_s && h->pv_is_f ? h->pv : nullptr, nullptr, 0, nullptr, ru);
            h->vl_valid = true; h->vl_box = h->box;
            continue;
        }
        const bool psi = with_psi && mode == MREAL_BUILD_LIST;
        launch_mreal(h->pos_s, h->posf_s, v, h->*out + out_off, rank_rows(h, N, mode == MREAL_BUILD_LIST ? depth : 0), h->cell_off, h->dbox,
                     h->nc, h->d.rcut, h->d.self, h->coef, h->n_intervals * 2 * RS_NCOEF, h->nb, mode, h->stream,
                     psi ? h->psi_s : nullptr, h->w_s, h->vl, vlm,
                     v == h->f_s && h->pv_is_f && (vlm == VL_USE || mode != MREAL_USE_LIST) ? h->pv : nullptr,   // packed (position, F) records
                     psi && h->n_slabs == 1 ? h->partials : nullptr, h->npart_cap, h->scal);   // single GPU: + the sums of Lanczos iteration 0
        h->sums0_done = psi && h->n_slabs == 1 && vlm != VL_USE && mreal_table_in_lds(h->n_intervals * 2 * RS_NCOEF);
        if (vlm == VL_WRITE) {   // the list now matches perm, pos_s and the box of this call
            HIPCHK(hipMemcpyAsync(h->pos_build, h->pos_s, (size_t)N * sizeof(double4), hipMemcpyDeviceToDevice, h->stream));
            h->vl_pending = false; h->vl_valid = true; h->vl_box = h->box;
        }
        if (mode == MREAL_BUILD_LIST) { h->nb_valid = true; h->w_is_mpsi = with_psi && (vlm == VL_USE || mreal_table_in_lds(h->n_intervals * 2 * RS_NCOEF)); }
    }
    return 0;
}

// rows a rank updates in a Lanczos iteration: its own and the ghost layers its next mat-vec reads
static int update_ranges(const pse_handle *h, int N, int rg[3][2]) { return row_ranges(h, N, 1, rg); }

// ---- what the four Lanczos drivers below share ------------------------------------------------------------------------------------
// Lanczos vector q of a handle: psi for q = 0, else parked in V[q] (the members of a team have one n_pad); none for q < 0.  THE place
// that knows the layout of the basis: psi is double4 always, V[q >= 1] rows of three doubles on a rows24 handle (pse_handle.h).
static VecOut lz_vec(const pse_handle *h, int q) {
    if (q < 0) return VecOut(nullptr);
    if (q == 0) return VecOut(h->psi_s);
    if (h->rows24) return VecOut(reinterpret_cast<double *>(h->V) + (size_t)3 * q * h->n_pad, 1);
    return VecOut(h->V + (size_t)q * h->n_pad);
}
// ... as a double4 array: the drivers of a team, whose kernels (k_lz_block, the Gram sums) read nothing else; never a rows24 handle
static double4 *lz_vec4(const pse_handle *h, int q) { return reinterpret_cast<double4 *>(lz_vec(h, q).p); }
// the whole basis for the final combination (row q * n_pad + i in either layout)
static VecIn lz_basis(const pse_handle *h) { return VecIn(reinterpret_cast<const double *>(h->V), h->rows24 ? 1 : 0); }
// where a pair-list mat-vec of the iteration leaves y = M x_j: the packed buffer of a rows24 handle, else w_s (where the build pass
// and real() leave theirs on every handle)
static VecOut lz_y(const pse_handle *h, bool from_list) { return from_list && h->rows24 ? VecOut(h->w24, 1) : VecOut(h->w_s); }
// A mat-vec through real() reads its vector as double4 (k_mreal_cells gathers neighbours' rows from it): on a rows24 handle only psi
// may go that way.  With a pair list (the condition of rows24) the drivers reach real() at iteration 0 alone -- it builds the list,
// and every later iteration runs on it -- unless a call between the build and the iteration invalidated the list while M psi was
// kept (pse_set_lanczos_operator): that iteration is refused before anything is read.
static int lz_real_ok(const pse_handle *h, int j) {
    if (j > 0 && h->rows24)
        return fail(PSE_ERR_INVALID, "Lanczos iteration %d would walk the cells on a basis in 24-byte rows: the pair list of this call is "
                    "no longer valid (was the Lanczos operator changed after the list was built?); repeat the call", j);
    return 0;
}
// the two-step block that starts at iteration j (full), or the single step j
static LzBlockArgs lz_block_args(const pse_handle *h, int j, bool full) {
    LzBlockArgs a{};
    a.q = lz_vec4(h, j); a.p = lz_vec4(h, j - 1); a.w1 = h->w_s; a.w2 = full ? h->w2_s : nullptr;
    a.u = h->u_s; a.v1 = lz_vec4(h, j + 1); a.v2 = full ? lz_vec4(h, j + 2) : nullptr;
    a.j = j;
    return a;
}
// the starting count of a call; its first convergence check is at max(m_in, 2) (Brownian.cu:465-466,606)
static int lz_m_in(const int *m_io) { return std::min(std::max(m_io ? *m_io : 2, 1), M_MAX); }
// the gated iterations a queue-only single-GPU call queues behind them (pse_set_lanczos_extra counts)
static int lz_queued_extra(const pse_handle *h, int m_in) {
    return std::max(0, std::min(h->lz_extra >= 0 ? h->lz_extra : h->tun.lz_extra, M_MAX - std::max(m_in, 2)));
}

// ---- ... and the two host-checked ones: a batch of iterations, its scalars read back, ONE decision (lz_decide_host) ---------------
// (alpha, beta and the norm are already on their way: the update kernels write them to the mapped host buffer as well)
static int lz_wait_scalars(pse_team &T, bool &hook_done, const std::function<int()> &before_first_wait) {
    pse_handle *h0 = T.m[0];
    HIPCHK(hipEventRecord(h0->ev_scal, h0->stream));
    if (!hook_done) {   // independent work queued behind the read-back keeps the GPU busy while the host decides
        hook_done = true;
        for (pse_handle *h : act(T)) TRY(te(h, PH_LANCZOS));
        if (before_first_wait) TRY(before_first_wait());
    }
    HIPCHK(hipEventSynchronize(h0->ev_scal));
    return 0;
}
// The decision on the batch that ends at iteration `done`: the sizes not yet checked, from m_in - 1 on.  d, built anew for every batch,
// brings `first` and what differs between the drivers (pending_beta; have_last_beta, normalised); the rest is filled in here.  The host
// mirror of the queue-only calls (LZ_HOST_M ..) is not written: pse_get_info reads it only after such a call, and its count of open
// calls is sticky.
static int lz_decide_batch(LzDecide d, int m_in, int done, double tol, const double *sc, LzState &st) {
    d.m_lo = std::max((d.first ? 0 : st.checked) + 1, std::max(m_in - 1, 1)); d.m_hi = d.done_iters = done; d.m_max = M_MAX; d.tol = tol;
    int at = 0;
    const LzFailure f = lz_decide_host(d, sc, st, &at);
    if (f == LZ_NONFINITE) return fail(PSE_ERR_NUMERIC, "Lanczos produced a non-finite coefficient at iteration %d", at);
    if (f == LZ_EIGEN_FAILED) return fail(PSE_ERR_NUMERIC, "tridiagonal eigen-solve failed at m = %d", at);
    return 0;
}
// psi == 0 -> result 0 (the decision's m_final = 0)
static int lz_zero_result(pse_team &T, int N, int matvecs) {
    for (pse_handle *h : act(T)) {
        HIPCHK(hipMemsetAsync(h->ub_s, 0, (size_t)N * sizeof(double4), h->stream));
        h->info.lanczos_m = 0; h->info.lanczos_matvecs = matvecs; h->info.lanczos_stepnorm = 0.0;
    }
    return 0;
}
// the final combination on every member's own rows, with the coefficients of the decision (Brownian.cu:716,739)
static void lz_combine(pse_team &T, int N, double scale, const LzState &st, int matvecs, int exchanges) {
    BasisCoef tc{};
    std::copy(st.coef, st.coef + st.m_final, tc.t);
    for (pse_handle *h : act(T)) {
        int lo, hi;
        row_range(h, N, lo, hi);
        launch_basis_combine(h->psi_s, lz_basis(h), h->n_pad, tc, st.m_final, h->scal, scale, 1, h->ub_s, lo, hi, h->stream, h->sink);
        h->tail_done = h->sink.on;
        h->info.lanczos_m = st.m_final; h->info.lanczos_matvecs = matvecs; h->info.lanczos_stepnorm = st.stepnorm;
        h->info.lanczos_exchanges = exchanges;
    }
}

// Queue-only Lanczos of a single GPU (pse_set_async): the iterations of the starting count are queued as the host-driven loop
// below queues them; then ONE launch takes the decision the host would take (k_lz_decide: the tridiagonal square roots of the two
// sizes m_in - 1 and m_in, the step norm), and `extra` more iterations follow, each with its own decision, every kernel of them
// gated on the outcome so far -- the reference iterates until the step norm passes (PSEv1/Brownian.cu:606-724); here whatever is
// not needed leaves at once.  The final combination takes m and its coefficients from the device.  Nothing is read back: the
// call can be captured into a hipGraph; m of a call reaches the host lazily (pse_get_info after a synchronisation, or the
// lanczos_m of the next call).  If the queue runs out before the step norm passes, the result uses the last size and
// pse_info.lanczos_status says 1.
static int lanczos_queued(pse_team &T, int N, double tol, double scale, int *m_io, const std::function<int()> &before_first_wait,
                          const std::function<int()> &before_combine) {
    pse_handle *h = T.m[0];
    const int m_in = lz_m_in(m_io), target = std::max(m_in, 2), extra = lz_queued_extra(h, m_in);
    const int *stop = &h->lz_state->done;
    const double seq = (double)++h->lz_seq;
    h->lz_last_queued = true;
    int rg[3][2];
    const int nrg_all = update_ranges(h, N, rg);
    // the vector part of iteration j: x_{j+1} from the sums that are still in place
    VecOut y = lz_y(h, false);   // where y = M x_j of the iteration in hand lies (a deferred vector part belongs to an iteration j >= 1: the list's)
    auto vector_part = [&](int j, const int *gate) {
        launch_lz_update(lz_vec(h, j), y, lz_vec(h, j - 1), lz_vec(h, j + 1), j, h->scal, rg, nrg_all, h->stream,
                         nullptr, 0, h->sc_host_dev, gate, vq_of(h), h->lz_sums);   // (+ the mirror of x_{j+1}: the next mat-vec's gathers, and two of its sums)
    };
    auto iteration = [&](int j, bool scalars_only, const int *gate) -> int {
        const bool have_y = j == 0 && h->w_is_mpsi;
        const bool fused = !have_y && h->nb.cap > 0 && h->nb_valid;
        if (!fused && !have_y) {
            if (gate) return fail(PSE_ERR_NUMERIC, "queued Lanczos: a gated iteration needs the pair list");
            TRY(lz_real_ok(h, j));
            TRY(real(T, j == 0 ? &pse_handle::psi_s : &pse_handle::V, &pse_handle::w_s, (size_t)j * h->n_pad, 0, N, true));
        }
        y = lz_y(h, fused);
        const double4 *vjm1 = lz_vec4(h, j - 1);   // for the kernels that read double4 alone: the mat-vec of iteration 0 (none) and k_lz_dots (iteration 0 on a rows24 handle: lz_real_ok)
        // from iteration 1 on the mat-vec sums x_j.y alone: x_j.x_j and x_j.x_{j-1} are what the update that wrote x_j left in lz_sums
        const bool split = fused && j > 0;
        if (fused)
            launch_mreal_lanczos(h->pos_s, lz_vec(h, j), y, row_map(0, N), h->cell_off, h->dbox, h->nc, h->d.rcut, h->d.self, h->coef, h->nb,
                                 LzFuse{split ? nullptr : vjm1, h->partials, h->npart_cap, nullptr, nullptr, nullptr, h->lz_sums, lz_update_grid(N)}, h->scal, nullptr, nullptr, h->stream,
                                 h->vl_use ? h->vl : VerletList{}, split ? 4 : 1, gate, DevRowArgs{}, j > 0 ? vq_of(h) : nullptr);
        else if (!(j == 0 && h->sums0_done))
            launch_lz_dots(lz_vec4(h, j), h->w_s, vjm1, 0, N, h->partials, h->npart_cap, h->scal, h->stream);
        h->w_is_mpsi = false; h->sums0_done = false;
        if (scalars_only) launch_lz_update(lz_vec(h, j), y, lz_vec(h, j - 1), lz_vec(h, j + 1), j, h->scal, rg, 0, h->stream, nullptr, 0,
                                           h->sc_host_dev, gate);
        else vector_part(j, gate);
        return 0;
    };
    for (int j = 0; j < target; ++j) TRY(iteration(j, j == target - 1, nullptr));
    LzDecide d{};
    d.m_lo = std::max(m_in - 1, 1); d.m_hi = target; d.done_iters = target; d.first = 1; d.last = extra == 0 ? 1 : 0; d.m_max = M_MAX; d.tol = tol;
    launch_lz_decide(d, h->scal, h->lz_state, h->sc_host_dev, seq, h->stream);
    int done = target;
    for (int x = 0; x < extra; ++x) {
        vector_part(done - 1, stop);
        TRY(iteration(done, true, stop));
        d.m_lo = d.m_hi = done + 1; d.done_iters = done + 1; d.pending_beta = done; d.first = 0; d.last = x == extra - 1 ? 1 : 0;
        launch_lz_decide(d, h->scal, h->lz_state, h->sc_host_dev, seq, h->stream);
        ++done;
    }
    TRY(te(h, PH_LANCZOS));
    if (before_first_wait) TRY(before_first_wait());
    if (before_combine) TRY(before_combine());
    launch_basis_combine(h->psi_s, lz_basis(h), h->n_pad, BasisCoef{}, 0, h->scal, scale, 1, h->ub_s, 0, N, h->stream, h->sink, h->lz_state);
    h->tail_done = h->sink.on;
    h->info.lanczos_matvecs = done; h->info.lanczos_exchanges = 0;
    // m of this call is known on the device only; what the host hands back is the most recent one that has reached it
    if (m_io) *m_io = h->sc_host[LZ_HOST_SEQ] > 0.0 && h->sc_host[LZ_HOST_M] >= 1.0 ? (int)h->sc_host[LZ_HOST_M] : m_in;
    HIPCHK(hipGetLastError());
    return 0;
}

// M_real^{1/2} psi by Lanczos (PSEv1/Brownian.cu:357-765): psi_s (sorted order, replicated on every rank) ->
// ub_s = scale |psi| V t on the rows this rank owns.  Scalars are replicated; vectors are valid on the own rows (+ the
// neighbouring cell layers for the vector the next mat-vec reads).
static int lanczos(pse_team &T, int N, double tol, double scale, int *m_io, const std::function<int()> &before_first_wait = nullptr,
                   WavePump *pump = nullptr, const std::function<int()> &before_combine = nullptr) {
    pse_handle *h0 = T.m[0];
    const int m_in = lz_m_in(m_io);
    if (h0->async_mode && T.G == 1 && T.solo < 0 && h0->nb.cap > 0 && !h0->timing &&
        lz_decide_supported(std::max(m_in, 2) + lz_queued_extra(h0, m_in)))
        return lanczos_queued(T, N, tol, scale, m_io, before_first_wait, before_combine);
    for (pse_handle *h : act(T)) h->lz_last_queued = false;
    const double *sc = h0->sc_host;   // pinned: the read-back of the device scalars is one DMA, no staging copy
    int done = 0, n_exchanges = 0;    // iterations launched so far
    int target = std::max(m_in, 2);
    int pending_beta = 0;             // beta_done = |x_done| does not exist when a batch is decided: it arrives with the next one
    LzState st{0, 0, 0, 0, 1.0, {}, {}};   // as a decision under `first` resets it
    bool hook_done = false;
    bool y_from_list = false;   // y = M x_j of the iteration in hand came from a pair-list mat-vec (lz_y; a deferred vector part is of an iteration j >= 1)
    // the update of iteration j: alpha_j, beta_j from the sums in place and, unless scalars_only, x_{j+1} on the own and the ghost rows
    auto update = [&](int j, bool scalars_only) {
        for (pse_handle *h : act(T)) {
            int rg[3][2];
            const int nrg = scalars_only ? 0 : update_ranges(h, N, rg);
            launch_lz_update(lz_vec(h, j), lz_y(h, y_from_list), lz_vec(h, j - 1), lz_vec(h, j + 1), j, h->scal, rg, nrg, h->stream, h->sums_all, T.G > 1 ? T.G : 0,
                             h == h0 ? h->sc_host_dev : nullptr, nullptr, T.G <= 1 ? vq_of(h) : nullptr, T.G <= 1 ? h->lz_sums : nullptr);
        }
    };
    while (true) {
        for (; done < target; ++done) {
            // iteration j = done on the unnormalised x_j (psi for j = 0, else parked in V[j]); see k_lz_update
            const bool have_y = done == 0 && h0->w_is_mpsi;      // M psi came with the pass that built the pair list
            const bool fused = !have_y && h0->nb.cap > 0 && h0->nb_valid;   // sums fused into the pair-list mat-vec
            const bool timed = done == 1 && fused;               // one pair-list mat-vec kernel per call is timed on its own
            if (!fused && !have_y) {
                TRY(lz_real_ok(h0, done));
                TRY(real(T, done == 0 ? &pse_handle::psi_s : &pse_handle::V, &pse_handle::w_s, (size_t)done * h0->n_pad, 0, N, true));
            }
            y_from_list = fused;
            for (pse_handle *h : act(T)) {
                int lo, hi;
                row_range(h, N, lo, hi);
                // x_{j-1}, unnormalised, for the kernels that read double4 alone: the mat-vec of iteration 0 (none), of a team, and k_lz_dots
                // (iteration 0 on a rows24 handle: lz_real_ok)
                const double4 *vjm1 = lz_vec4(h, done - 1);
                if (fused) {
                    const bool ev = timed && h->timing;
                    // a single GPU, from iteration 1 on: the mat-vec sums x_j.y alone; x_j.x_j and x_j.x_{j-1} are what the update that
                    // wrote x_j left in lz_sums.  Teams keep the three sums of the mat-vec: they travel with the exchange.
                    const bool split = done > 0 && T.G <= 1;
                    launch_mreal_lanczos(h->pos_s, lz_vec(h, done), lz_y(h, true), row_map(lo, hi), h->cell_off, h->dbox, h->nc, h->d.rcut, h->d.self, h->coef,
                                         h->nb, LzFuse{split ? nullptr : vjm1, h->partials, h->npart_cap, nullptr, nullptr, nullptr, h->lz_sums, lz_update_grid(N)}, h->scal,
                                         ev ? h->ph[PH_MATVEC].a : nullptr, ev ? h->ph[PH_MATVEC].b : nullptr, h->stream,
                                         h->vl_use ? h->vl : VerletList{}, split ? 4 : 1, nullptr, DevRowArgs{}, done > 0 && T.G <= 1 ? vq_of(h) : nullptr);
                    if (timed) h->matvec_timed = true;
                } else if (!(done == 0 && h->sums0_done)) {   // (iteration 0: the sums came with the pass that built the pair list)
                    launch_lz_dots(lz_vec4(h, done), h->w_s, vjm1, lo, hi, h->partials, h->npart_cap, h->scal, h->stream);
                }
                h->w_is_mpsi = false; h->sums0_done = false;
            }
            // the partial sums and the ghost rows of y = M x_j in one exchange; every rank then updates its own rows AND its ghost
            // rows (it holds x_j and x_{j-1} there from the previous iteration), so x_{j+1} needs no exchange of its own
            if (pump) TRY(pump->upto(n_exchanges));   // the far-field exchanges whose slot has come go first
            ++n_exchanges;
            TRY(team_lanczos_exchange(T, [](pse_handle *h) { return (double *)h->w_s; }));
            // The LAST iteration of a batch only derives its scalars (alpha_j, beta_j): whether x_{j+1} is needed at all is what the
            // check below decides -- in the steady state of a time-stepping loop (m_in = m) it is not, and the step saves one vector
            // pass and the reduction of |x_{j+1}| (0.04 ms at the metric point).  If the iteration goes on, the vector part follows.
            update(done, done == target - 1);
        }
        TRY(lz_wait_scalars(T, hook_done, before_first_wait));
        if (T.solo >= 0) { st.m_final = done; break; }   // timing only (pse_team_debug_solo): coefficients zero
        // alpha_0 .. alpha_{done-1}, beta_1 .. beta_{done-1} have arrived
        LzDecide d{};
        d.first = pending_beta == 0; d.pending_beta = pending_beta;
        TRY(lz_decide_batch(d, m_in, done, tol, sc, st));
        if (st.done) break;   // (always at done = M_MAX: the walk reaches that size, where m >= m_max ends it)
        // not converged: the vector part of the last iteration (its sums are still in place), then the next batch; an x_done that
        // vanishes (invariant subspace) shows in the first sums of that batch
        update(done - 1, false);
        pending_beta = done;
        target = std::min(M_MAX, done + std::max(2, done / 4));
    }
    if (st.m_final == 0) {
        if (m_io) *m_io = m_in;
        return lz_zero_result(T, N, done);
    }
    if (before_combine) TRY(before_combine());   // (the far-field velocities must be in place if the combination adds them)
    // the basis holds the unnormalised x_q: v_q = x_q / |x_q|, |x_0| = the norm of psi, |x_q| = beta_q -- normalised = 0
    lz_combine(T, N, scale, st, done, T.G > 1 ? n_exchanges : 0);
    if (m_io) *m_io = st.m_final;
    return 0;
}

// M_real^{1/2} psi for a team, TWO Lanczos iterations per exchange (k_lz_block in pse_kernels.hip has the algebra).  Per block:
// w1 = M v_j on the own rows + one ghost layer, w2 = M w1 on the own rows with the Gram sums fused in, ONE exchange (all-reduce
// of the sums + two ghost layers of w1 and w2 to either neighbour), then every rank forms v_{j+1}, v_{j+2} and M v_{j+1} on its own
// and its ghost rows.  An odd tail is a single step (scalars only unless the iteration goes on).  The alpha, beta the host checks
// are the reference's (PSEv1/Brownian.cu:440-521) to rounding, so m is -- the tests hold it to the port's.  The first w1 = M psi
// comes with the pass that built the pair list.  Exchanges per step at m = 7: 4 (one-step driver: 7).
static int lanczos_team(pse_team &T, int N, double tol, double scale, int *m_io, const std::function<int()> &before_first_wait,
                        WavePump *pump, const std::function<int()> &before_combine = nullptr) {
    pse_handle *h0 = T.m[0];
    for (pse_handle *h : act(T)) h->lz_last_queued = false;
    const int m_in = lz_m_in(m_io);
    const double *sc = h0->sc_host;
    int done = 0, target = std::max(m_in, 2), n_exchanges = 0, matvecs = 0;
    int half_pending = -1;                // j of a single step whose vectors have not been formed yet
    bool first = true;
    LzState st{0, 0, 0, 0, 1.0, {}, {}};   // as a decision under `first` resets it
    bool hook_done = false;
    while (true) {
        while (done < target) {
            if (half_pending >= 0) {      // the iteration goes on past a single step: its vector part (w1 is there on two ghost layers)
                for (pse_handle *h : act(T)) {
                    int rg[3][2];
                    const int nrg = row_ranges(h, N, 2, rg);
                    launch_lz_block(lz_block_args(h, half_pending, false), false, h->scal, rg, nrg, h->stream, h->sums_all, T.G, h == h0 ? h->sc_host_dev : nullptr);
                }
                half_pending = -1;
            }
            const int j = done;
            const bool full = target - done >= 2 && j + 2 <= M_MAX;
            for (pse_handle *h : act(T)) {
                const LzFuse lz{nullptr, h->partials, h->npart_cap, lz_vec4(h, j), lz_vec4(h, j - 1), j > 0 ? h->u_s : nullptr};
                if (j == 0 && !h->w_is_mpsi) return fail(PSE_ERR_NUMERIC, "two-step Lanczos: M psi did not come with the pair list");
                if (!(j == 0 && h->w_is_mpsi)) {   // w1 = M v_j: own rows + one ghost layer for a block, own rows for a single step
                    launch_mreal_lanczos(h->pos_s, lz_vec(h, j), h->w_s, rank_rows(h, N, full ? 1 : 0), h->cell_off, h->dbox, h->nc, h->d.rcut,
                                         h->d.self, h->coef, h->nb, lz, h->scal, nullptr, nullptr, h->stream, VerletList{}, full ? 0 : 3);
                    ++matvecs;
                } else if (!full) {
                    return fail(PSE_ERR_NUMERIC, "two-step Lanczos: a single step cannot start at j = 0");
                }
                h->w_is_mpsi = false;
                if (full) {                        // w2 = M w1 on the own rows, Gram sums fused
                    launch_mreal_lanczos(h->pos_s, h->w_s, h->w2_s, rank_rows(h, N, 0), h->cell_off, h->dbox, h->nc, h->d.rcut, h->d.self,
                                         h->coef, h->nb, lz, h->scal, nullptr, nullptr, h->stream, VerletList{}, 2);
                    ++matvecs;
                }
            }
            if (pump) TRY(pump->upto(n_exchanges));
            ++n_exchanges;
            TRY(team_run_exchange(T, [&](pse_handle *h) {
                                      auto ops = ghost_ops(h, T.G, {(double *)h->w_s, full ? (double *)h->w2_s : nullptr}, 2);
                                      sum_ops(h, T.G, LZ_NGRAM, ops);
                                      return ops; },
                                  false, DIAG_LANCZOS));
            for (pse_handle *h : act(T)) {
                int rg[3][2];
                const int nrg = full ? row_ranges(h, N, 2, rg) : 0;   // a single step derives its scalars only, for now
                launch_lz_block(lz_block_args(h, j, full), full, h->scal, rg, nrg, h->stream, h->sums_all, T.G, h == h0 ? h->sc_host_dev : nullptr);
            }
            if (full) done += 2; else { done += 1; half_pending = j; }
        }
        TRY(lz_wait_scalars(T, hook_done, before_first_wait));
        if (T.solo >= 0) { st.m_final = done; break; }   // timing only (pse_team_debug_solo): coefficients zero
        // alpha_0 .. alpha_{done-1}, beta_1 .. beta_done have arrived
        LzDecide d{};                     // beta_done arrives with its batch, and the basis holds NORMALISED v_q, except v_0 = psi / |psi|
        d.first = first; d.have_last_beta = d.normalised = 1;
        TRY(lz_decide_batch(d, m_in, done, tol, sc, st));
        if (st.done) break;   // (always at done = M_MAX: the walk reaches that size, where m >= m_max ends it)
        first = false;
        target = std::min(M_MAX, done + std::max(2, done / 4));
    }
    if (st.m_final == 0) {
        if (m_io) *m_io = m_in;
        return lz_zero_result(T, N, matvecs);
    }
    if (half_pending >= 0 && st.m_final > half_pending + 1) return fail(PSE_ERR_NUMERIC, "two-step Lanczos: basis vector %d was never formed", half_pending + 1);
    if (before_combine) TRY(before_combine());   // (the far-field velocities must be in place if the combination adds them)
    lz_combine(T, N, scale, st, matvecs, n_exchanges);
    if (m_io) *m_io = st.m_final;
    return 0;
}

// per-member argument pointers of a team call
struct Args {
    const double4 *pos; const double4 *force; double4 *vel;
};

// what pse_step does after the velocity is known (K15 gpu_stokes_step_one_kernel, PSEv1/Stokes.cu:137-192): handed to velocity()
// so that the final un-sort and the Euler update are one pass over the particles
struct StepArgs {
    double4 *pos; double4 *vel; double3 *accel; int3 *image; const double4 *force;
};
struct StepTail { const std::vector<StepArgs> *sa; double dt, shear_rate; };

static int velocity(pse_team &T, const std::vector<Args> &a, const unsigned *group, int N, int parts, double kT, double dt,
                    unsigned timestep, int *m_io, unsigned *mask, const StepTail *tail = nullptr) {
    for (pse_handle *h : T.m)
        if (h->loc.on) return fail(PSE_ERR_INVALID, "this handle is an owned-particle rank (pse_params.local_rows): drive it through pse_team_step_local");
    // tail_done says that THIS call's Lanczos combination wrote the summed rows.  A call with noise but without the real-space half
    // (parts = 2, kT > 0: no Lanczos iteration) must not read what an earlier Brownian call on the same handle left there -- it would
    // skip its own sum and never write vel.  The reset here and the lz guards below each prevent that alone; both are kept.
    for (pse_handle *h : T.m) h->tail_done = false;
    diag_begin(T);
    for (size_t r = 0; r < T.m.size(); ++r)
        if (T.solo < 0 || T.m[r]->slab_rank == T.solo)   // psi rides with the gather into cell order: the near-field pass that
            TRY(prepare(T.m[r], a[r].pos, a[r].force, group, N, true, false, PrepExtra{kT > 0.0, timestep}, (parts & 1) != 0));   // builds the pair list applies M_real to F and psi together
    *mask |= 1u << PH_SORT;
    const bool noise = kT > 0.0;
    const bool sstep = T.G > 1 && noise && (parts & 1) && team_sstep(T.m[0]);   // two Lanczos iterations per exchange
    for (pse_handle *h : act(T)) {   // where the wave chain of this call runs
        // The two chains share the chip whenever nothing is timed per kernel (with phase timing on, every kernel runs alone on one
        // stream: those durations are the roofline evidence).  A single GPU forks for deterministic evaluations only (Brownian
        // steps gain nothing there); a TEAM always forks: at 1 / G of the rows no kernel fills the chip, and the
        // far-field exchanges travel while the Lanczos iterations compute (one communicator, one communication stream: pse_team).
        const bool on = h->side && parts == 3 && !h->timing && (T.G > 1 ? T.lanes : (h->overlap_all || !noise));
        if (on != h->side_on || h->wstream != (on ? h->side : h->stream)) {
            h->side_on = on;
            h->wstream = on ? h->side : h->stream;
            TRY(bind_wave_stream(h));
        }
    }
    WavePump pump;
    const WaveArgs wa{N, noise, kT, dt, timestep};
    auto wave_start = [&]() -> int { return pump.start(T, wa, T.m[0]->tun.team_sched, mask); };
    // With noise on one stream the wave chain is queued BEHIND the Lanczos iterations: the host has to read their scalars
    // back before it can finish the Brownian part, and meanwhile the GPU works through the far field instead of idling.
    const bool wave_behind = noise && (parts & 2) && (parts & 1) && !T.m[0]->side_on;
    // Two lanes and noise: the near field + Lanczos chain is the longer lane, so its first pass is queued BEFORE the far-field chain
    // (which forks here and follows at once); a deterministic evaluation has the far field as its longer lane and keeps it first.
    const bool near_first = noise && parts == 3 && T.m[0]->side_on;
    if (near_first) TRY(pump.fork(T));
    if ((parts & 2) && !wave_behind && !near_first) TRY(wave_start());
    // the slab row boundaries are needed from here on (a host round trip); the first part of the far-field chain is queued
    for (pse_handle *h : act(T)) TRY(slab_bounds_wait(h, N));
    if (parts & 1) {
        for (pse_handle *h : act(T)) TRY(ts(h, PH_REAL));
        TRY(real(T, &pse_handle::f_s, &pse_handle::ur_s, 0, 0, N, noise, noise, sstep ? 1 : 0));
        for (pse_handle *h : act(T)) TRY(te(h, PH_REAL));
        *mask |= 1u << PH_REAL;
    }
    if (near_first) TRY(wave_start());
    const bool lz = noise && (parts & 1);   // the particle noise M_real^{1/2} psi belongs to the real-space half (the k-space noise to the wave half)
    if (lz) {
        for (pse_handle *h : act(T)) TRY(ts(h, PH_LANCZOS));   // closed inside the Lanczos driver, after the first batch of iterations
        for (pse_handle *h : act(T)) h->matvec_timed = false;
        const std::function<int()> hook = [&]() -> int {    // before the host first waits for the Lanczos scalars: everything else is queued
            if (wave_behind) TRY(wave_start());
            return pump.drain();
        };
        const double tol = T.m[0]->d.error, scale = std::sqrt(2.0 * kT / dt);
        // The final combination of the Lanczos vectors adds the far-field and the near-field velocity of its row and sends the sum
        // where the step wants it: one pass and one launch less than combination -> ub_s -> sum / un-sort.
        for (size_t r = 0; r < T.m.size(); ++r) {
            pse_handle *h = T.m[r];
            h->tail_done = false;
            h->sink = CombineSink{};
            if (parts == 3) h->sink = CombineSink{true, h->uw_s, h->ur_s, h->tag_s, T.G == 1 ? a[r].vel : nullptr, T.G == 1 ? nullptr : h->utot_s};
        }
        const std::function<int()> join = [&]() -> int {   // the gathered far-field velocity is needed by the combination
            TRY(pump.drain());
            for (pse_handle *h : act(T))
                if (h->side_on && h->sink.on) {
                    if (h == act(T)[0]) diag_mark(T, 3, h->side);
                    HIPCHK(hipEventRecord(h->ev_join, h->side));
                    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_join, 0));
                }
            return 0;
        };
        if (sstep) TRY(lanczos_team(T, N, tol, scale, m_io, hook, &pump, join));
        else TRY(lanczos(T, N, tol, scale, m_io, hook, &pump, join));
        for (pse_handle *h : act(T)) h->sink = CombineSink{};
        *mask |= 1u << PH_LANCZOS;
        if (T.m[0]->matvec_timed) *mask |= 1u << PH_MATVEC;
    }
    TRY(pump.drain());   // (kT = 0: the exchanges of the far-field chain are issued here, one after the other)
    if (T.G > 1) {
        // every rank has all three contributions for the rows it owns: add them, exchange the row blocks once
        for (pse_handle *h : act(T))
            if ((parts & 2) && h->side_on) {   // join: the gathered far-field velocity is needed now
                if (h == act(T)[0] && !(lz && h->tail_done)) diag_mark(T, 3, h->side);
                HIPCHK(hipEventRecord(h->ev_join, h->side));
                HIPCHK(hipStreamWaitEvent(h->stream, h->ev_join, 0));
            }
        for (pse_handle *h : act(T)) {
            if (lz && h->tail_done) continue;   // the Lanczos combination has written the summed rows already
            int lo, hi;
            row_range(h, N, lo, hi);
            launch_sum_rows((parts & 2) ? h->uw_s : nullptr, (parts & 1) ? h->ur_s : nullptr, lz ? h->ub_s : nullptr,
                            h->utot_s, lo, hi, h->stream, h->tag_s);   // the tags travel with the rows: no rank orders foreign rows
        }
        TRY(team_all_gather_rows(T, [](pse_handle *h) { return (double *)h->utot_s; }));
    }
    for (size_t r = 0; r < T.m.size(); ++r) {
        pse_handle *h = T.m[r];
        if (T.solo >= 0 && h->slab_rank != T.solo) continue;
        if ((parts & 2) && h->side_on && T.G == 1) {   // join
            HIPCHK(hipEventRecord(h->ev_join, h->side));
            HIPCHK(hipStreamWaitEvent(h->stream, h->ev_join, 0));
        }
        const double4 *ua = T.G > 1 ? h->utot_s : ((parts & 2) ? h->uw_s : nullptr);
        const double4 *ub = T.G > 1 ? nullptr : ((parts & 1) ? h->ur_s : nullptr), *uc = T.G > 1 ? nullptr : (lz ? h->ub_s : nullptr);
        const unsigned *tags = T.G > 1 ? nullptr : h->tag_s;     // a team: the tag travels in the fourth component of its row
        if (!(T.G == 1 && lz && h->tail_done)) launch_scatter_sum(ua, ub, uc, tags, N, a[r].vel, h->stream);   // (single GPU: the Lanczos combination has un-sorted the sum)
        if (tail) {
            // The Euler update stays its own pass in the CALLER's order (replicated state: every rank updates every particle,
            // bit-identically).  Fused into the un-sort it ran over the sorted rows and made five arrays scattered instead of
            // one: 152 us against 29 + 35 per rank at the metric point (profiles/r04_team8_notes.txt).
            const StepArgs &x = (*tail->sa)[r];
            TRY(ts(h, PH_INTEG));
            launch_integrate(x.pos, x.vel, x.accel, x.image, x.force, group, N, h->dbox, tail->dt, tail->shear_rate, h->stream);
            TRY(te(h, PH_INTEG));
        }
        HIPCHK(hipGetLastError());
    }
    diag_mark(T, 1, act(T)[0]->stream);
    return 0;
}

static int team_of_one(pse_handle *h, pse_team &T) {
    if (h->n_slabs > 1) return fail(PSE_ERR_INVALID, "this handle is a slab rank: drive it through a pse_team");
    T.m = {h}; T.G = 1;
    return 0;
}

static int do_mobility(pse_team &T, const std::vector<Args> &a, const unsigned *group, unsigned N, int parts) {
    for (pse_handle *h : T.m) TRY(check_n(h, N));
    for (auto &x : a) if (!x.pos || !x.force || !x.vel) return fail(PSE_ERR_INVALID, "null array");
    if (!(parts & 3)) return fail(PSE_ERR_INVALID, "parts must select real (1), wave (2) or both (3)");
    unsigned mask = 1u << PH_TOTAL;
    for (pse_handle *h : act(T)) TRY(ts(h, PH_TOTAL));
    TRY(velocity(T, a, group, (int)N, parts, 0.0, 1.0, 0, nullptr, &mask));
    for (pse_handle *h : act(T)) { TRY(te(h, PH_TOTAL)); TRY(collect_times(h, mask)); }
    return 0;
}

static int do_brownian(pse_team &T, const std::vector<Args> &a, const unsigned *group, unsigned N, double kT, double dt,
                       unsigned timestep, int *lanczos_m, int parts = 3) {
    for (pse_handle *h : act(T)) TRY(check_n(h, N));
    for (auto &x : a) if (!x.pos || !x.force || !x.vel) return fail(PSE_ERR_INVALID, "null array");
    if (kT < 0 || !(dt > 0)) return fail(PSE_ERR_INVALID, "need kT >= 0 and dt > 0");
    unsigned mask = 1u << PH_TOTAL;
    for (pse_handle *h : act(T)) TRY(ts(h, PH_TOTAL));
    TRY(velocity(T, a, group, (int)N, parts, kT, dt, timestep, lanczos_m, &mask));
    for (pse_handle *h : act(T)) { TRY(te(h, PH_TOTAL)); TRY(collect_times(h, mask)); }
    return 0;
}

static int do_step(pse_team &T, const std::vector<StepArgs> &sa, const unsigned *group, unsigned N, double kT, double dt,
                   unsigned timestep, double shear_rate, int *lanczos_m) {
    for (pse_handle *h : act(T)) TRY(check_n(h, N));
    std::vector<Args> a;
    for (auto &x : sa) {
        if (!x.pos || !x.vel || !x.accel || !x.image || !x.force) return fail(PSE_ERR_INVALID, "null array");
        a.push_back(Args{x.pos, x.force, x.vel});
    }
    if (kT < 0 || !(dt > 0)) return fail(PSE_ERR_INVALID, "need kT >= 0 and dt > 0");
    unsigned mask = (1u << PH_TOTAL) | (1u << PH_INTEG);
    for (pse_handle *h : act(T)) TRY(ts(h, PH_TOTAL));
    for (pse_handle *h : act(T)) h->vl_kind = 1;   // an integrating step: its own neighbour-list suspension state
    const StepTail tail{&sa, dt, shear_rate};
    const int rc_v = velocity(T, a, group, (int)N, 3, kT, dt, timestep, lanczos_m, &mask, &tail);
    for (pse_handle *h : act(T)) h->vl_kind = 0;
    if (rc_v) return rc_v;
    for (pse_handle *h : act(T)) {
        TRY(te(h, PH_TOTAL));
        HIPCHK(hipGetLastError());
        TRY(collect_times(h, mask));
    }
    return 0;
}

// ---- owned-particle team step (pse_team_step_local; kernels in pse_local.hip) ---------------------------------------------------
// Everything below only QUEUES work: the row counts of a step never reach the host (LocalRows lives in device memory, every
// launch covers the capacity), every exchange has the fixed size of its capacity, the Lanczos decision is k_lz_decide's.
static LocalRegions local_regions(const pse_handle *h) {
    const LocalGeom &g = h->loc.g;
    const int lc = layer_cells(h->nc), nx = g.nx;
    auto wrap = [&](int l) { return ((l % nx) + nx) % nx; };
    LocalRegions r{};
    const int l_own = g.rank * g.per, l_gl = wrap(l_own - g.depth), l_gr = wrap(l_own + g.per);
    r.c0[0] = l_own * lc; r.c1[0] = (l_own + g.per) * lc; r.base[0] = 0; r.cap[0] = g.c_own;
    r.c0[1] = l_gl * lc; r.c1[1] = (l_gl + g.depth) * lc; r.base[1] = g.c_own; r.cap[1] = g.c_g;
    r.c0[2] = l_gr * lc; r.c1[2] = (l_gr + g.depth) * lc; r.base[2] = g.c_own + g.c_g; r.cap[2] = g.c_g;
    r.c_first_end = (l_own + g.depth) * lc - 1;            // the empty last cell of layer l_own + depth - 1
    r.c_last_begin = (l_own + g.per - g.depth) * lc;
    r.c_gl_adj = wrap(l_own - 1) * lc;
    r.c_gr_adj = (l_gr + 1) * lc - 1;                      // the empty last cell of layer l_gr
    return r;
}

// M_real^{1/2} psi of an owned-particle team: the two-step blocks of lanczos_team (k_lz_block has the algebra), queue-only.  Blocks for
// the starting count, ONE decision on the device (sizes m_in - 1 and m_in), then ceil(PSE_LANCZOS_EXTRA / 2) further blocks, each
// with its decision, their kernels gated on the outcome so far (the exchanges of a gated block still travel: they carry no
// meaning then, and every rank takes the same decisions from the same sums).  Ghost rows move by position: the first c_g rows of
// w1, w2 go left as they lie, the rows of the last layers were parked by the mat-vecs (stage_w1, stage_w2: their first row is known
// on the device only) and go right; they arrive in the ghost regions of the neighbours' w1, w2.
static int lanczos_local(pse_team &T, double tol, int *m_io, WavePump *pump) {
    pse_handle *h0 = T.m[0];
    const int m_in = lz_m_in(m_io), target = std::max(m_in, 2);
    const int extra_blocks = ((T.lz_extra >= 0 ? T.lz_extra : h0->tun.lz_extra) + 1) / 2;
    if (target + 2 * extra_blocks > M_MAX || !lz_decide_supported(target + 2 * extra_blocks))
        return fail(PSE_ERR_INVALID, "owned-particle step: starting count %d of the Lanczos iteration is beyond what the device-side decision takes", m_in);
    int n_exchanges = 0, matvecs = 0, done = 0, half_pending = -1;
    auto fuse = [&](pse_handle *h, int j) { return LzFuse{nullptr, h->partials, h->npart_cap, lz_vec4(h, j), lz_vec4(h, j - 1), j > 0 ? h->u_s : nullptr}; };
    auto exchange = [&](bool full) -> int {
        if (pump) TRY(pump->upto(n_exchanges));
        ++n_exchanges;
        return team_run_exchange(T, [&](pse_handle *h) {
            const LocalGeom &g = h->loc.g;
            const int L = (g.rank + g.G - 1) % g.G, R = (g.rank + 1) % g.G;
            const size_t cnt = (size_t)g.c_g * 4;
            std::vector<Xfer> ops;
            // my first layers go left and arrive as the left neighbour's right ghosts; my last layers (parked) go right
            ops.push_back(Xfer{(double *)h->w_s, cnt, L, (double *)(h->w_s + g.c_own + g.c_g), cnt, R});
            ops.push_back(Xfer{(double *)h->loc.stage_w1, cnt, R, (double *)(h->w_s + g.c_own), cnt, L});
            if (full) {
                ops.push_back(Xfer{(double *)h->w2_s, cnt, L, (double *)(h->w2_s + g.c_own + g.c_g), cnt, R});
                ops.push_back(Xfer{(double *)h->loc.stage_w2, cnt, R, (double *)(h->w2_s + g.c_own), cnt, L});
            }
            sum_ops(h, T.G, LZ_NGRAM, ops);
            return ops; }, false, DIAG_LANCZOS);
    };
    auto full_block = [&](int j, bool gated) -> int {
        for (pse_handle *h : act(T)) {
            const int *gate = gated ? &h->lz_state->done : nullptr;
            const LocalRows *R = h->loc.rows;
            if (j == 0) {
                if (!h->w_is_mpsi) return fail(PSE_ERR_NUMERIC, "owned-particle step: M psi did not come with the pair list");
            } else {   // w1 = M v_j on the own rows + the adjacent ghost layers
                launch_mreal_lanczos(h->pos_s, lz_vec(h, j), h->w_s, RowMap{}, h->cell_off, h->dbox, h->nc, h->d.rcut, h->d.self, h->coef, h->nb, fuse(h, j),
                                     h->scal, nullptr, nullptr, h->stream, VerletList{}, 0, gate,
                                     DevRowArgs{&R->own1, R, h->loc.stage_w1, h->loc.rows_cap, h->loc.g.c_g});
                ++matvecs;
            }
            h->w_is_mpsi = false;
            // w2 = M w1 on the own rows, Gram sums fused
            launch_mreal_lanczos(h->pos_s, h->w_s, h->w2_s, RowMap{}, h->cell_off, h->dbox, h->nc, h->d.rcut, h->d.self, h->coef, h->nb, fuse(h, j), h->scal,
                                 nullptr, nullptr, h->stream, VerletList{}, 2, gate, DevRowArgs{&R->own, R, h->loc.stage_w2, h->loc.g.c_own, h->loc.g.c_g});
            ++matvecs;
        }
        TRY(exchange(true));
        for (pse_handle *h : act(T))
            launch_lz_block(lz_block_args(h, j, true), true, h->scal, nullptr, 0, h->stream, h->sums_all, T.G, h->sc_host_dev, &h->loc.rows->all,
                            h->loc.rows_cap, false, gated ? &h->lz_state->done : nullptr);
        return 0;
    };
    auto single = [&](int j, bool gated) -> int {   // an odd starting count ends on one iteration: scalars now, vectors only if the iteration goes on
        for (pse_handle *h : act(T)) {
            const LocalRows *R = h->loc.rows;
            launch_mreal_lanczos(h->pos_s, lz_vec(h, j), h->w_s, RowMap{}, h->cell_off, h->dbox, h->nc, h->d.rcut, h->d.self, h->coef, h->nb, fuse(h, j), h->scal,
                                 nullptr, nullptr, h->stream, VerletList{}, 3, gated ? &h->lz_state->done : nullptr,
                                 DevRowArgs{&R->own, R, h->loc.stage_w1, h->loc.g.c_own, h->loc.g.c_g});
            ++matvecs;
        }
        TRY(exchange(false));
        for (pse_handle *h : act(T))
            launch_lz_block(lz_block_args(h, j, false), false, h->scal, nullptr, 0, h->stream, h->sums_all, T.G, h->sc_host_dev, &h->loc.rows->all,
                            h->loc.rows_cap, true, gated ? &h->lz_state->done : nullptr);
        half_pending = j;
        return 0;
    };
    auto decide = [&](int m_lo, int m_hi, int done_iters, bool first, bool last) {
        for (pse_handle *h : act(T)) {
            LzDecide d{};
            d.m_lo = m_lo; d.m_hi = m_hi; d.done_iters = done_iters; d.have_last_beta = 1; d.first = first ? 1 : 0; d.last = last ? 1 : 0;
            // (pse_team_debug_solo: the other ranks' sums are stale, the step norm means nothing -- the decision is made to pass at the
            // starting count, as it does in the steady state of a time-stepping loop, so the gated block is timed as what it then is)
            d.normalised = 1; d.m_max = M_MAX; d.tol = T.solo >= 0 ? 1e300 : tol;
            launch_lz_decide(d, h->scal, h->lz_state, h->sc_host_dev, (double)h->lz_seq, h->stream);
        }
    };
    for (pse_handle *h : act(T)) { ++h->lz_seq; h->lz_last_queued = true; }
    while (target - done >= 2) { TRY(full_block(done, false)); done += 2; }
    if (target - done == 1) { TRY(single(done, false)); done += 1; }
    decide(std::max(m_in - 1, 1), target, done, true, extra_blocks == 0);
    for (int x = 0; x < extra_blocks; ++x) {
        if (half_pending >= 0) {   // the vector part of the single step (its sums are still in place)
            for (pse_handle *h : act(T))
                launch_lz_block(lz_block_args(h, half_pending, false), false, h->scal, nullptr, 0, h->stream, h->sums_all, T.G, h->sc_host_dev,
                                &h->loc.rows->all, h->loc.rows_cap, false, &h->lz_state->done);
            half_pending = -1;
        }
        TRY(full_block(done, true));
        decide(done + 1, done + 2, done + 2, false, x == extra_blocks - 1);
        done += 2;
    }
    for (pse_handle *h : act(T)) { h->info.lanczos_matvecs = matvecs; h->info.lanczos_exchanges = n_exchanges; }
    // What the host hands back is the most recent m that has reached its mirror -- in ONE process only: between processes that
    // moment differs from rank to rank, and ranks that then start the next step from different counts queue different numbers of
    // exchanges (a hang).  A rank of a process team gets its starting count back unchanged; pse_get_info after a synchronisation
    // gives the m of the completed step -- the same on every rank, they all take the same decisions from the same sums.
    if (m_io) *m_io = !remote(T) && h0->sc_host[LZ_HOST_SEQ] > 0.0 && h0->sc_host[LZ_HOST_M] >= 1.0 ? (int)h0->sc_host[LZ_HOST_M] : m_in;
    return 0;
}

static int local_call(pse_team &T, const std::vector<LocalCaller> &ca, double kT, double dt, unsigned timestep, double shear_rate, int integrate,
                      int *m_io) {
    if (T.G < 2) return fail(PSE_ERR_INVALID, "pse_team_step_local needs a team of >= 2 ranks");
    for (size_t r = 0; r < T.m.size(); ++r) {
        pse_handle *h = T.m[r];
        if (!h->loc.on) return fail(PSE_ERR_INVALID, "pse_team_step_local: member %zu was not created with local_rows", r);
        if (h->loc.err_host[0]) return fail(PSE_ERR_INVALID, "owned-particle rank %d: an earlier step failed on the device (flags %d: 1 own rows, 2 ghost rows, "
                                            "4 message capacity exceeded, 8 a particle moved beyond the neighbour, 16 n_local above capacity)", h->slab_rank, h->loc.err_host[0]);
        const LocalCaller &c = ca[r];
        if (!c.pos || !c.vel || !c.accel || !c.image || !c.force || !c.tag || !c.n_local) return fail(PSE_ERR_INVALID, "null array");
        HIPCHK(hipSetDevice(h->device));
    }
    if (kT < 0 || !(dt > 0)) return fail(PSE_ERR_INVALID, "need kT >= 0 and dt > 0");
    const bool noise = kT > 0.0;
    unsigned mask = 0;
    auto stage = [&](const char *what) -> int {   // developer aid (PSE_DEBUG_SYNC, read when the team was created): wait and report after every stage
        if (!T.debug_sync) return 0;
        hipError_t e = hipDeviceSynchronize();
        fprintf(stderr, "pse local_call: %s: %s\n", what, hipGetErrorString(e));
        return e == hipSuccess ? 0 : fail(PSE_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    };
    diag_begin(T);
    for (pse_handle *h : act(T)) {   // two lanes: the far-field chain next to the near field / Lanczos chain
        const bool on = h->side && !h->timing && T.lanes;
        if (on != h->side_on || h->wstream != (on ? h->side : h->stream)) {
            h->side_on = on;
            h->wstream = on ? h->side : h->stream;
            TRY(bind_wave_stream(h));
        }
    }
    // (1) classification of the own particles + the messages for both neighbours
    for (size_t r = 0; r < T.m.size(); ++r) {
        pse_handle *h = T.m[r];
        if (T.solo >= 0 && h->slab_rank != T.solo) continue;
        // (the counters of a step -- bins, cells, layers, messages -- were cleared by the last step's k_local_finish; a first step, or
        // one after a call that did not reach its end, clears them here)
        if (!h->loc.zeroed) HIPCHK(hipMemsetAsync(h->cnt_block, 0, h->loc.zero_ints * sizeof(int), h->stream));
        h->loc.zeroed = false;
        const LocalPool pool{h->keys, h->keys_s, h->perm, h->cell_cnt};
        launch_local_classify(ca[r], h->loc.g, h->dbox, h->nc, pool, h->loc.send[0], h->loc.send[1], h->loc.counters, h->loc.err, h->loc.layer_cnt, h->stream);
    }
    TRY(stage("classify"));
    // (2) ONE exchange: my left message goes left, what arrives from the right is the right neighbour's left message
    TRY(team_run_exchange(T, [&](pse_handle *h) {
        const LocalGeom &g = h->loc.g;
        const int L = (g.rank + g.G - 1) % g.G, R = (g.rank + 1) % g.G;
        std::vector<Xfer> ops;
        const size_t body = h->loc.msg - LOCAL_HDR;
        // the records, and in front of them -- one more transfer, 8 bytes -- the sender's two record counters as they lie in its memory
        ops.push_back(Xfer{h->loc.send[0] + LOCAL_HDR, body, L, h->loc.recv[1] + LOCAL_HDR, body, R});
        ops.push_back(Xfer{h->loc.send[1] + LOCAL_HDR, body, R, h->loc.recv[0] + LOCAL_HDR, body, L});
        ops.push_back(Xfer{(const double *)h->loc.counters, 1, L, h->loc.recv[1], 1, R});
        ops.push_back(Xfer{(const double *)h->loc.counters, 1, R, h->loc.recv[0], 1, L});
        return ops; }, false, DIAG_FIRST));
    TRY(stage("first exchange"));
    // (3) cell sort of what the rank keeps: own particles that stayed, arrivals, ghosts
    for (size_t r = 0; r < T.m.size(); ++r) {
        pse_handle *h = T.m[r];
        if (T.solo >= 0 && h->slab_rank != T.solo) continue;
        const LocalPool pool{h->keys, h->keys_s, h->perm, h->cell_cnt};
        const int ncell = cells_total(h->nc);
        if ((size_t)ncell > h->n_cells_alloc) return fail(PSE_ERR_INVALID, "cell grid exceeds the capacity sized at creation");
        launch_local_bin_incoming(h->loc.recv[0], h->loc.recv[1], h->loc.g, h->dbox, h->nc, pool, h->loc.err, h->loc.layer_cnt, h->stream);
        const LocalRegions rg = local_regions(h);
        launch_local_offsets(h->cell_cnt, h->loc.layer_cnt, h->cell_off, h->loc.g, rg, layer_cells(h->nc), h->loc.rows, h->loc.err, h->stream);
        launch_local_scatter(h->cell_off, h->loc.g, pool, h->vals, h->loc.rows, h->stream);
        const FarBinArgs far = far_bin_args(h->G, h->sw);
        const LocalSorted out{h->pos_s, h->posf_s, h->pv, h->f_s, h->tag_s, h->loc.porig_s, h->loc.mass_s, h->loc.image_s, noise ? h->psi_s : nullptr};
        launch_local_permute(ca[r], h->loc.recv[0], h->loc.recv[1], h->loc.g, h->dbox, h->cell_off, pool, h->vals, h->loc.rows, out, &far, h->par.seed,
                             timestep, h->ts_off, h->stream);
        h->sorted_N = 0; h->nb_valid = false; h->vl_valid = false; h->w_is_mpsi = false; h->pv_is_f = true;
        CellRanges need{};   // (the generic far-field kernels: rows outside these hold no particle)
        need.n = 3;
        for (int q = 0; q < 3; ++q) { need.c0[q] = rg.c0[q]; need.c1[q] = rg.c1[q] - 1; }
        h->sw.need = need; h->sw.cell_off = h->cell_off; h->sw.rows_local = 1;
    }
    // (4) the far-field chain (side lane), the near field and the Lanczos blocks (main lane)
    TRY(stage("sort + permute"));
    // The side lane forks from the sort, but the main lane's pass is queued FIRST: the near field + Lanczos chain is the longer of the
    // two (the far-field lane ends ~250 us earlier at eight ranks), and a dispatch that reaches the device behind the spread waits
    // for the spread's workgroups to leave the CUs.
    WavePump pump;
    const WaveArgs wa{T.m[0]->loc.rows_cap, noise, kT, dt, timestep};
    TRY(pump.fork(T));
    for (pse_handle *h : act(T)) {
        const LocalRows *R = h->loc.rows;
        const int nco = h->n_intervals * 2 * RS_NCOEF;
        if (noise)   // the pass that builds the pair list applies M_real to F and psi together, on the own rows + the adjacent ghost layers
            launch_mreal(h->pos_s, h->posf_s, h->f_s, h->ur_s, RowMap{}, h->cell_off, h->dbox, h->nc, h->d.rcut, h->d.self, h->coef, nco, h->nb,
                         MREAL_BUILD_LIST, h->stream, h->psi_s, h->w_s, VerletList{}, VL_NONE, h->pv, nullptr, 0, nullptr, Gate{},
                         DevRowArgs{&R->own1, R, h->loc.stage_w1, h->loc.rows_cap, h->loc.g.c_g});
        else
            launch_mreal(h->pos_s, h->posf_s, h->f_s, h->ur_s, RowMap{}, h->cell_off, h->dbox, h->nc, h->d.rcut, h->d.self, h->coef, nco, h->nb,
                         MREAL_CELLS, h->stream, nullptr, nullptr, VerletList{}, VL_NONE, h->pv, nullptr, 0, nullptr, Gate{},
                         DevRowArgs{&R->own, R, nullptr, h->loc.g.c_own, 0});
        h->nb_valid = noise; h->w_is_mpsi = noise;
    }
    TRY(stage("near field"));
    TRY(pump.start(T, wa, T.m[0]->tun.team_sched, &mask));
    TRY(stage("records + spread + forward transforms"));
    if (noise) TRY(lanczos_local(T, T.m[0]->d.error, m_io, &pump));
    TRY(stage("lanczos"));
    TRY(pump.drain());
    TRY(stage("far field"));
    // (5) join the lanes; the end of the step on the own rows, written to the caller's arrays
    for (size_t r = 0; r < T.m.size(); ++r) {
        pse_handle *h = T.m[r];
        if (T.solo >= 0 && h->slab_rank != T.solo) continue;
        if (h->side_on) {
            if (h == act(T)[0]) diag_mark(T, 3, h->side);
            HIPCHK(hipEventRecord(h->ev_join, h->side));
            HIPCHK(hipStreamWaitEvent(h->stream, h->ev_join, 0));
        }
        LocalFinish f{};
        f.rows = h->loc.rows; f.st = noise ? h->lz_state : nullptr;
        f.zero = h->cnt_block; f.n_zero = (int)h->loc.zero_ints;
        f.psi_s = h->psi_s; f.V = h->V; f.stride = h->n_pad; f.scal = h->scal; f.scale = noise ? std::sqrt(2.0 * kT / dt) : 0.0;
        f.uw_s = h->uw_s; f.ur_s = h->ur_s;
        f.porig_s = h->loc.porig_s; f.f_s = h->f_s; f.mass_s = h->loc.mass_s; f.image_s = h->loc.image_s; f.tag_s = h->tag_s;
        f.integrate = integrate; f.dt = dt; f.shear_rate = shear_rate;
        launch_local_finish(f, ca[r], h->dbox, h->loc.g.c_own, h->stream);
        HIPCHK(hipMemcpyAsync(h->loc.err_host, h->loc.err, sizeof(int), hipMemcpyDeviceToHost, h->stream));   // (read by the NEXT call: nothing waits)
        HIPCHK(hipGetLastError());
        h->loc.zeroed = true;
    }
    diag_mark(T, 1, act(T)[0]->stream);
    return 0;
}

// ---- single-handle C-ABI -------------------------------------------------------------------------------------------
extern "C" int pse_mobility(pse_handle *h, const pse_double4 *pos, const pse_double4 *force, pse_double4 *vel,
                            const unsigned *group, unsigned N, int parts) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    pse_team T;
    TRY(team_of_one(h, T));
    return do_mobility(T, {Args{(const double4 *)pos, (const double4 *)force, (double4 *)vel}}, group, N, parts);
}

extern "C" int pse_brownian_velocity(pse_handle *h, const pse_double4 *pos, const pse_double4 *force, pse_double4 *vel,
                                     const unsigned *group, unsigned N, double kT, double dt, unsigned timestep,
                                     int *lanczos_m) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    pse_team T;
    TRY(team_of_one(h, T));
    return do_brownian(T, {Args{(const double4 *)pos, (const double4 *)force, (double4 *)vel}}, group, N, kT, dt, timestep,
                       lanczos_m);
}

// The two halves of a Brownian evaluation on their own (a FUNCTIONAL split for two GPUs): parts = 1 the real-space
// half M_real.F + sqrt(2kT/dt) M_real^{1/2} psi, parts = 2 the wave-space half M_wave.F + the k-space noise; the halves add up to
// what pse_brownian_velocity returns (the reference computes them in one call and shares its inverse FFT and gather between the
// deterministic and the stochastic wave part as this does, PSEv1/Brownian.cu:772-923).
extern "C" int pse_brownian_velocity_part(pse_handle *h, const pse_double4 *pos, const pse_double4 *force, pse_double4 *vel,
                                          const unsigned *group, unsigned N, double kT, double dt, unsigned timestep, int parts,
                                          int *lanczos_m) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    if (parts < 1 || parts > 3) return fail(PSE_ERR_INVALID, "parts must select real (1), wave (2) or both (3)");
    if (!pos || !force || !vel) return fail(PSE_ERR_INVALID, "null array");
    pse_team T;
    TRY(team_of_one(h, T));
    return do_brownian(T, {Args{(const double4 *)pos, (const double4 *)force, (double4 *)vel}}, group, N, kT, dt, timestep, lanczos_m, parts);
}

// K15 alone (gpu_stokes_step_one_kernel, PSEv1/Stokes.cu:137-192): the Euler update + wrap for velocities the caller has put together
extern "C" int pse_integrate(pse_handle *h, pse_double4 *pos, const pse_double4 *vel, pse_double3 *accel, pse_int3 *image,
                             const pse_double4 *net_force, const unsigned *group, unsigned N, double dt, double shear_rate) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    if (!pos || !vel || !accel || !image || !net_force) return fail(PSE_ERR_INVALID, "null array");
    if (!(dt > 0)) return fail(PSE_ERR_INVALID, "need dt > 0");
    TRY(check_n(h, N));
    HIPCHK(hipSetDevice(h->device));
    launch_integrate((double4 *)pos, (const double4 *)vel, (double3 *)accel, (int3 *)image, (const double4 *)net_force, group, (int)N, h->dbox, dt,
                     shear_rate, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int pse_step(pse_handle *h, pse_double4 *pos, pse_double4 *vel, pse_double3 *accel, pse_int3 *image,
                        const pse_double4 *net_force, const unsigned *group, unsigned N, double kT, double dt,
                        unsigned timestep, double shear_rate, int *lanczos_m) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    pse_team T;
    TRY(team_of_one(h, T));
    return do_step(T, {StepArgs{(double4 *)pos, (double4 *)vel, (double3 *)accel, (int3 *)image, (const double4 *)net_force}},
                   group, N, kT, dt, timestep, shear_rate, lanczos_m);
}

extern "C" int pse_sqrt_mreal(pse_handle *h, const pse_double4 *pos, const pse_double4 *psi, pse_double4 *out,
                              const unsigned *group, unsigned N, double tol, int *lanczos_m) {
    TRY(check_n(h, N));
    if (!pos || !psi || !out) return fail(PSE_ERR_INVALID, "null array");
    pse_team T;
    TRY(team_of_one(h, T));
    TRY(prepare(h, (const double4 *)pos, (const double4 *)psi, group, (int)N));   // f_s <- psi in sorted order
    HIPCHK(hipMemcpyAsync(h->psi_s, h->f_s, (size_t)N * sizeof(double4), hipMemcpyDeviceToDevice, h->stream));
    TRY(lanczos(T, (int)N, tol, 1.0, lanczos_m));
    launch_scatter_sum(h->ub_s, nullptr, nullptr, h->tag_s, (int)N, (double4 *)out, h->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int pse_random_psi(pse_handle *h, pse_double4 *psi, const unsigned *group, unsigned N, unsigned timestep) {
    TRY(check_n(h, N));
    if (!psi) return fail(PSE_ERR_INVALID, "null array");
    std::vector<unsigned> tags(N);
    if (group) HIPCHK(hipMemcpy(tags.data(), group, N * sizeof(unsigned), hipMemcpyDeviceToHost));
    else for (unsigned i = 0; i < N; ++i) tags[i] = i;
    HIPCHK(hipMemcpy(h->tag_s, tags.data(), N * sizeof(unsigned), hipMemcpyHostToDevice));
    launch_psi(h->psi_s, h->tag_s, (int)N, h->par.seed, timestep, h->stream);
    launch_scatter_sum(h->psi_s, nullptr, nullptr, h->tag_s, (int)N, (double4 *)psi, h->stream);
    HIPCHK(hipStreamSynchronize(h->stream));
    h->sorted_N = 0;
    return 0;
}

extern "C" int pse_eval_realspace(pse_handle *h, const double *r_host, int n, double *f_host, double *g_host) {
    if (!h || !r_host || !f_host || !g_host || n <= 0) return fail(PSE_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    // The kernel looks up r' = r^2 rsqrt(r^2), not r: three roundings, r' <= r (1 + 2^-51).  An r within that of the table's end could
    // index the interval behind the last one, so the end is refused with that margin (2^-50: the product below rounds once more).
    for (int i = 0; i < n; ++i)
        if (!(r_host[i] > 0.0) || r_host[i] * RS_PER_UNIT * (1.0 + 0x1p-50) >= h->n_intervals)
            return fail(PSE_ERR_INVALID, "r[%d] = %g outside the table range (0, %g)", i, r_host[i], (double)h->n_intervals / RS_PER_UNIT);
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, (size_t)3 * n * sizeof(double)));
    hipError_t e = hipMemcpy(buf, r_host, n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_eval_fg(buf, n, h->coef, buf + n, buf + 2 * n, h->stream);
        e = hipStreamSynchronize(h->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(f_host, buf + n, n * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(g_host, buf + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) return fail(PSE_ERR_HIP, "pse_eval_realspace: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int pse_debug_matvec_ms(pse_handle *h, int reps, float *ms_per_launch) {
    if (!h || !ms_per_launch || reps < 1) return fail(PSE_ERR_INVALID, "pse_debug_matvec_ms: bad argument");
    HIPCHK(hipSetDevice(h->device));
    if (h->n_slabs != 1 || !h->nb_valid || h->nb.cap <= 0 || h->sorted_N <= 0)
        return fail(PSE_ERR_INVALID, "pse_debug_matvec_ms: needs the pair list of a Brownian call on a single-GPU engine (call it right after one)");
    const int N = h->sorted_N;
    RowMap rm{};
    rm.n = 1; rm.lo[0] = 0; rm.hi[0] = N;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    auto run = [&](int n) {   // the launch of a Lanczos iteration j >= 1 (vector V[1], its mirror, the sums against V[0] = psi), the kernel alone
        for (int r = 0; r < n; ++r)
            launch_mreal_lanczos(h->pos_s, lz_vec(h, 1), lz_y(h, true), rm, h->cell_off, h->dbox, h->nc, h->d.rcut, h->d.self, h->coef, h->nb,
                                 LzFuse{h->psi_s, h->partials, h->npart_cap, nullptr, nullptr, nullptr}, h->scal, nullptr, nullptr, h->stream,
                                 VerletList{}, 1, nullptr, DevRowArgs{}, vq_of(h), true);   // (the mat-vec of the handle's current operator)
    };
    run(2);
    HIPCHK(hipEventRecord(e0, h->stream));
    run(reps);
    HIPCHK(hipEventRecord(e1, h->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    HIPCHK(hipGetLastError());
    *ms_per_launch = ms / (float)reps;
    return 0;
}
extern "C" int pse_debug_vq_roundtrip(int n, const double *rows_host, double *out_host) {
    if (n < 0 || (n > 0 && (!rows_host || !out_host))) return fail(PSE_ERR_INVALID, "pse_debug_vq_roundtrip: null argument");
    if (n == 0) return 0;
    double *d_in = nullptr, *d_out = nullptr;
    hipError_t e = hipMalloc((void **)&d_in, (size_t)3 * n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&d_out, (size_t)3 * n * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(d_in, rows_host, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) { launch_vq_roundtrip(d_in, d_out, n, nullptr); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpy(out_host, d_out, (size_t)3 * n * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(d_in); (void)hipFree(d_out);
    if (e != hipSuccess) return fail(PSE_ERR_HIP, "pse_debug_vq_roundtrip: %s", hipGetErrorString(e));
    return 0;
}
static_assert(PSE_DEBUG_LZ_NSCAL == LZ_NSCAL && LZ_HOST_OPEN == LZ_HOST_M + 4 && LZ_HOST_OPEN < LZ_NSCAL, "pse_debug_lz_decide: layout of the scalars");
extern "C" int pse_debug_lz_decide_supported(int m_hi) { return lz_decide_supported(m_hi) ? 1 : 0; }
extern "C" int pse_debug_lz_decide(const double *scal_host, int n_dec, const pse_debug_lz_decision *dec, double open0, pse_debug_lz_outcome *out) {
    if (int rc = lz_decisions_validate("pse_debug_lz_decide", scal_host, n_dec, dec, out)) return rc;
    // everything the kernel sizes its LDS and its loops by is checked HERE: no launch with more than the launcher asked for
    for (int k = 0; k < n_dec; ++k) {
        const pse_debug_lz_decision &d = dec[k];
        if (!lz_decide_supported(d.m_hi)) return fail(PSE_ERR_INVALID, "pse_debug_lz_decide: decision %d: m_hi = %d is not supported", k, d.m_hi);
        if (d.m_lo < d.m_hi - 1)
            return fail(PSE_ERR_INVALID, "pse_debug_lz_decide: decision %d: m_lo = %d is not m_hi or m_hi - 1 (m_hi = %d)", k, d.m_lo, d.m_hi);
    }
    double *scal = nullptr, *sch = nullptr;
    LzState *st = nullptr;
    std::vector<double> mirror(LZ_NSCAL, 0.0);
    mirror[LZ_HOST_OPEN] = open0;
    hipError_t e = hipMalloc((void **)&scal, LZ_NSCAL * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&sch, LZ_NSCAL * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void **)&st, sizeof(LzState));
    if (e == hipSuccess) e = hipMemcpy(scal, scal_host, LZ_NSCAL * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(sch, mirror.data(), LZ_NSCAL * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(st, 0xff, sizeof(LzState));   // NaN bytes: only the reset under `first` makes the state valid
    for (int k = 0; k < n_dec && e == hipSuccess; ++k) {
        launch_lz_decide(lz_decision(dec[k]), scal, st, sch, dec[k].seq, nullptr);
        e = hipGetLastError();
        LzState hs;
        if (e == hipSuccess) e = hipMemcpy(&hs, st, sizeof(LzState), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(out[k].mirror, sch + LZ_HOST_M, 5 * sizeof(double), hipMemcpyDeviceToHost);
        if (e != hipSuccess) break;
        lz_outcome(hs, &out[k]);
    }
    (void)hipFree(scal); (void)hipFree(sch); (void)hipFree(st);
    if (e != hipSuccess) return fail(PSE_ERR_HIP, "pse_debug_lz_decide: %s", hipGetErrorString(e));
    return 0;
}
extern "C" int pse_debug_grid_placement(pse_handle *h, int *tried, float *ms_first, float *ms_kept) {
    if (!h || !tried || !ms_first || !ms_kept) return fail(PSE_ERR_INVALID, "pse_debug_grid_placement: null argument");
    *tried = h->place_tried; *ms_first = h->place_ms_first; *ms_kept = h->place_ms_kept;
    return 0;
}
extern "C" int pse_debug_kvector(pse_handle *h, int n, const int *ijk_host, double *out_host) {
    if (!h || !ijk_host || !out_host || n <= 0) return fail(PSE_ERR_INVALID, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    for (int t = 0; t < n; ++t)
        if (ijk_host[3 * t] < 0 || ijk_host[3 * t] >= h->G.Nx || ijk_host[3 * t + 1] < 0 || ijk_host[3 * t + 1] >= h->G.Ny ||
            ijk_host[3 * t + 2] < 0 || ijk_host[3 * t + 2] >= h->G.Nz)
            return fail(PSE_ERR_INVALID, "node %d outside the %d x %d x %d grid", t, h->G.Nx, h->G.Ny, h->G.Nz);
    int *d_ijk = nullptr;
    double *d_out = nullptr;
    HIPCHK(hipMalloc((void **)&d_ijk, (size_t)3 * n * sizeof(int)));
    hipError_t e = hipMalloc((void **)&d_out, (size_t)5 * n * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(d_ijk, ijk_host, (size_t)3 * n * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_debug_kop(d_ijk, n, h->G, h->dbox, h->d.xi, h->d.eta, d_out, h->stream);
        e = hipStreamSynchronize(h->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(out_host, d_out, (size_t)5 * n * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(d_ijk);
    if (d_out) (void)hipFree(d_out);
    if (e != hipSuccess) return fail(PSE_ERR_HIP, "pse_debug_kvector: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int pse_debug_spread(pse_handle *h, const pse_double4 *pos, const pse_double4 *force, const unsigned *group, unsigned N) {
    TRY(check_n(h, N));
    if (!pos || !force) return fail(PSE_ERR_INVALID, "null array");
    if (h->n_slabs > 1) return fail(PSE_ERR_INVALID, "this handle is a slab rank: drive it through a pse_team");
    TRY(prepare(h, (const double4 *)pos, (const double4 *)force, group, (int)N));
    const DGrid &G = h->G;
    const size_t nr = (size_t)(G.nxl + G.hl + G.nhalo) * G.Ny * G.Nz;
    if (spread_needs_zero(G)) HIPCHK(hipMemsetAsync(h->rgrid, 0, 3 * nr * sizeof(double), h->stream));
    HIPCHK(launch_far_records(h->pos_s, h->f_s, (int)N, G, h->dbox, h->sw, h->stream));
    HIPCHK(launch_spread(h->pos_s, h->f_s, (int)N, h->rgrid, h->rgrid + nr, h->rgrid + 2 * nr, G, h->dbox, h->sw, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int pse_debug_gather(pse_handle *h, const pse_double4 *pos, const double *grid_host, const unsigned *group, unsigned N,
                                pse_double4 *vel_out) {
    TRY(check_n(h, N));
    if (!pos || !grid_host || !vel_out) return fail(PSE_ERR_INVALID, "null array");
    if (h->n_slabs > 1) return fail(PSE_ERR_INVALID, "this handle is a slab rank: drive it through a pse_team");
    TRY(prepare(h, (const double4 *)pos, nullptr, group, (int)N));   // (no vector: the records' force words are not read by the gather)
    const DGrid &G = h->G;
    const size_t nr = (size_t)(G.nxl + G.hl + G.nhalo) * G.Ny * G.Nz, plane = (size_t)G.Ny * G.Nz;
    HIPCHK(launch_far_records(h->pos_s, h->f_s, (int)N, G, h->dbox, h->sw, h->stream));
    for (int c = 0; c < 3; ++c)   // the layout pse_debug_copy_grid returns (a single GPU stores no halo planes: hl = nhalo = 0)
        HIPCHK(hipMemcpyAsync(h->rgrid + c * nr + plane * G.hl, grid_host + (size_t)c * plane * G.nxl, plane * G.nxl * sizeof(double),
                              hipMemcpyHostToDevice, h->stream));
    HIPCHK(launch_gather(h->pos_s, h->sw, (int)N, h->rgrid, h->rgrid + nr, h->rgrid + 2 * nr, G, h->dbox, h->uw_s, h->stream));
    launch_scatter_sum(h->uw_s, nullptr, nullptr, h->tag_s, (int)N, (double4 *)vel_out, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int pse_debug_far_path(pse_handle *h, unsigned N, int *out6) {
    TRY(check_n(h, N));
    if (!out6) return fail(PSE_ERR_INVALID, "null array");
    far_path(h->G, h->sw, (int)N, h->dbox.xy, out6);
    return 0;
}

// The wave-space stage of a step from grid to grid: parts 0 (its transforms), 1 and 2 of wave_compute as a step queues them.
extern "C" int pse_debug_wave_grid(pse_handle *h, const double *grid_in_host, double xi, double eta, int noise, double kT, double dt,
                                   unsigned timestep, int poison, double *grid_out_host) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    if (!grid_out_host) return fail(PSE_ERR_INVALID, "null array");
    if (noise && !(kT >= 0.0)) return fail(PSE_ERR_INVALID, "kT must be non-negative");
    if (noise && !(dt > 0.0)) return fail(PSE_ERR_INVALID, "dt must be positive");
    pse_team T;
    TRY(team_of_one(h, T));   // (refuses a slab rank)
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));   // whatever an earlier call left queued on either lane
    if (h->side) HIPCHK(hipStreamSynchronize(h->side));
    const DGrid &G = h->G;
    const size_t plane = (size_t)G.Ny * G.Nz, nr = plane * (G.nxl + G.hl + G.nhalo), ncx = (size_t)G.nxl * G.Ny * G.Nzp;
    if (poison) {   // NaN in every double of both grids: the pad columns of the spectrum rows included
        HIPCHK(hipMemsetAsync(h->rgrid, 0xFF, 3 * nr * sizeof(double), h->wstream));
        HIPCHK(hipMemsetAsync(h->cgrid, 0xFF, 3 * ncx * sizeof(double2), h->wstream));
    }
    for (int c = 0; c < 3; ++c) {   // the layout pse_debug_copy_grid returns
        double *dst = h->rgrid + c * nr + plane * G.hl;
        if (grid_in_host) HIPCHK(hipMemcpyAsync(dst, grid_in_host + (size_t)c * plane * G.nxl, plane * G.nxl * sizeof(double), hipMemcpyHostToDevice, h->wstream));
        else HIPCHK(hipMemsetAsync(dst, 0, plane * G.nxl * sizeof(double), h->wstream));
    }
    WaveArgs a{0, noise != 0, kT, dt, timestep};
    a.xi = xi; a.eta = eta;
    TRY(wave_forward_transforms(h, 1));
    TRY(wave_compute(T, a, 1));
    TRY(wave_compute(T, a, 2));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->wstream));
    for (int c = 0; c < 3; ++c)
        HIPCHK(hipMemcpy(grid_out_host + (size_t)c * plane * G.nxl, h->rgrid + c * nr + plane * G.hl, plane * G.nxl * sizeof(double),
                         hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int pse_debug_fft_path(pse_handle *h, int *out8) {
    if (!h || !out8) return fail(PSE_ERR_INVALID, "pse_debug_fft_path: null argument");
    const FftChoice none{FFT_ROCFFT, 0};
    const FftChoice x = h->xfuse ? xfft_choice(h->G, scale_args(h, false, 0.0, 1.0, 0)) : none;
    const FftChoice y = h->own_y ? yfft_choice(h->G, h->tun.yfft_kb) : none;   // (a slab rank's y pass, launch_yfft_slab, is not reported)
    const int out[8] = {h->xfuse, h->own_y, h->own_z, x.kernel, x.kb, y.kernel, y.kb, h->own_z ? zfft_choice(h->G.Nz) : FFT_ROCFFT};
    std::copy(out, out + 8, out8);
    return 0;
}

extern "C" int pse_debug_copy_grid(pse_handle *h, int stage, double *host_out) {
    if (!h || !host_out) return fail(PSE_ERR_INVALID, "bad argument");
    (void)stage;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->side) HIPCHK(hipStreamSynchronize(h->side));
    const size_t plane = (size_t)h->G.Ny * h->G.Nz, full = plane * (h->G.nxl + h->G.hl + h->G.nhalo);
    for (int c = 0; c < 3; ++c)   // the slab's own planes of each component (halo planes are not copied)
        HIPCHK(hipMemcpy(host_out + (size_t)c * plane * h->G.nxl, h->rgrid + c * full + plane * h->G.hl, plane * h->G.nxl * sizeof(double),
                         hipMemcpyDeviceToHost));
    return 0;
}

// ---- team C-ABI (multi-GPU) --------------------------------------------------------------------------------------
extern "C" int pse_team_unique_id(void *id128_host) {
    if (!id128_host) return fail(PSE_ERR_INVALID, "null argument");
    static_assert(sizeof(ncclUniqueId) == 128, "RCCL unique id is 128 bytes");
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    memcpy(id128_host, &id, sizeof id);
    return 0;
}

extern "C" int pse_team_destroy(pse_team *T);
// One double round the ring through the team's own exchange path (RCCL group or the host program's transport): every rank sends its
// number to the right neighbour and must receive the left neighbour's.  A transport that does not deliver -- a rank that never
// joined, crossed peers -- is reported here, at creation, not as a hang or as wrong physics in the first step.
static int team_ring_test(pse_team &T) {
    if (T.G < 2 || !remote(T)) return 0;
    pse_handle *h = T.m[0];
    HIPCHK(hipSetDevice(h->device));
    DeviceArrays scratch;   // (freed on every way out)
    double *buf = nullptr;
    HIPCHK(scratch.make((void **)&buf, 2 * sizeof(double)));
    const double mine = 1000.0 + h->slab_rank;
    double got = -1.0;
    int rc = 0;
    hipError_t e = hipMemcpy(buf, &mine, sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const int L = (h->slab_rank + T.G - 1) % T.G, R = (h->slab_rank + 1) % T.G;
        rc = team_exchange(T, {Xfer{buf, 1, R, buf + 1, 1, L}}, false);
        if (!rc) e = hipStreamSynchronize(h->stream);
        if (!rc && e == hipSuccess && T.comm) e = hipStreamSynchronize(T.comm);
        if (!rc && e == hipSuccess) e = hipMemcpy(&got, buf + 1, sizeof(double), hipMemcpyDeviceToHost);
        if (!rc && e == hipSuccess && got != 1000.0 + L)
            rc = fail(PSE_ERR_COMM, "team ring test: rank %d expected %g from its left neighbour %d and received %g -- the transport does not "
                      "connect the ranks as a ring of %d", h->slab_rank, 1000.0 + L, L, got, T.G);
    }
    if (e != hipSuccess && !rc) rc = fail(PSE_ERR_COMM, "team ring test failed: %s", hipGetErrorString(e));
    return rc;
}
// RCCL communicator of a one-member-per-process team (in-process teams have nothing to connect)
static int team_connect(pse_team *T, const void *id128_host) {
    if (T->m.size() != 1 || !id128_host) return 0;
    ncclUniqueId id;
    memcpy(&id, id128_host, sizeof id);
    HIPCHK(hipSetDevice(T->m[0]->device));
    {   // a rank that never joins leaves ncclCommInitRank waiting for ever: wait for it on a thread, with a deadline (PSE_TEAM_CONNECT_TIMEOUT, s)
        const char *te_ = getenv("PSE_TEAM_CONNECT_TIMEOUT");
        const int limit = te_ ? std::max(1, atoi(te_)) : 300;
        // The thread writes into a slot of its OWN (shared with this function): on a timeout the caller destroys the team, and a
        // peer that joins late -- or a bootstrap that fails later -- must not find freed memory behind the pointer.
        struct Slot { std::promise<ncclResult_t> done; ncclComm_t comm = nullptr; std::atomic<bool> abandoned{false}; };
        auto slot = std::make_shared<Slot>();
        std::future<ncclResult_t> fut = slot->done.get_future();
        const int G_ = T->G, r_ = T->m[0]->slab_rank, dev_ = T->m[0]->device;
        std::thread([slot, G_, id, r_, dev_]() {
            (void)hipSetDevice(dev_);
            const ncclResult_t r = ncclCommInitRank(&slot->comm, G_, id, r_);
            if (slot->abandoned.load() && r == ncclSuccess && slot->comm) { (void)ncclCommAbort(slot->comm); slot->comm = nullptr; }   // nobody will ever use it
            slot->done.set_value(r);
        }).detach();
        if (fut.wait_for(std::chrono::seconds(limit)) != std::future_status::ready) {
            slot->abandoned.store(true);
            return fail(PSE_ERR_COMM, "RCCL communicator of %d ranks did not form within %d s: a peer is missing (rank %d waited; "
                        "PSE_TEAM_CONNECT_TIMEOUT sets the limit)", G_, limit, r_);
        }
        const ncclResult_t r0 = fut.get();
        if (r0 != ncclSuccess) return fail(PSE_ERR_COMM, "ncclCommInitRank failed: %s", ncclGetErrorString(r0));
        T->nccl = slot->comm;
    }
    // Two compute lanes + a communication stream of their own are OPT-IN for an RCCL team (PSE_TEAM_LANES=1): no multi-GPU node has
    // run that path yet.  Default: one stream carries the kernels and the RCCL calls, in program order -- nothing can interleave.
    {
        const char *e = getenv("PSE_TEAM_LANES");
        T->lanes = e && atoi(e) > 0;
    }
    if (T->G > 1 && T->lanes) {   // the one stream every RCCL call of the team is issued on (see pse_team)
        HIPCHK(T->streams.make(&T->comm, hipStreamNonBlocking));
        T->evs.resize(32);
        for (hipEvent_t &e : T->evs) HIPCHK(T->events.make(&e, hipEventDisableTiming));
    }
    return team_ring_test(*T);
}

extern "C" int pse_team_create(pse_handle **members, int n_members, const void *id128_host, pse_team **out) {
    if (!members || n_members < 1 || !out) return fail(PSE_ERR_INVALID, "bad argument");
    *out = nullptr;
    if (!members[0]) return fail(PSE_ERR_INVALID, "null member");
    const int G = members[0]->n_slabs;
    std::vector<char> seen(G, 0);
    for (int i = 0; i < n_members; ++i) {
        pse_handle *h = members[i];
        if (!h || h->n_slabs != G) return fail(PSE_ERR_INVALID, "members disagree on n_slabs");
        if (h->d.Nx != members[0]->d.Nx || h->d.Ny != members[0]->d.Ny || h->d.Nz != members[0]->d.Nz || h->n_pad != members[0]->n_pad)
            return fail(PSE_ERR_INVALID, "members disagree on grid or capacity");
        if (seen[h->slab_rank]) return fail(PSE_ERR_INVALID, "slab rank %d appears twice", h->slab_rank);
        seen[h->slab_rank] = 1;
    }
    if (n_members == 1 && (G > 1 || id128_host)) {
        if (!id128_host) return fail(PSE_ERR_INVALID, "a one-rank-per-process team needs the RCCL unique id of rank 0");
    } else if (n_members != G) {
        return fail(PSE_ERR_INVALID, "an in-process team must hold all %d slab ranks (got %d)", G, n_members);
    }
    pse_team *T = new pse_team();
    T->m.assign(members, members + n_members);
    T->G = G;
    if (const char *e = getenv("PSE_TEAM_LANES")) T->lanes = atoi(e) > 0;   // in-process and host-staged teams: two lanes unless switched off
    if (n_members > 1)   // in-process team: one side stream for all members, so every lane is ordered by its stream alone
        for (int i = 1; i < n_members; ++i) members[i]->side = members[0]->side;
    int rc = team_connect(T, id128_host);
    if (rc) { std::string keep = error_text(); pse_team_destroy(T); error_text() = keep; return rc; }
    *out = T;
    return 0;
}

extern "C" int pse_team_create_transport(pse_handle *member, const pse_transport *transport, pse_team **out) {
    if (!member || !transport || !out || !transport->exchange) return fail(PSE_ERR_INVALID, "bad argument");
    *out = nullptr;
    if (member->n_slabs < 2) return fail(PSE_ERR_INVALID, "a team needs handles created with n_slabs >= 2");
    pse_team *T = new pse_team();
    T->m = {member};
    T->G = member->n_slabs;
    T->cb = *transport;
    T->has_cb = true;
    if (const char *e = getenv("PSE_TEAM_LANES")) T->lanes = atoi(e) > 0;
    if (int rc = team_ring_test(*T)) { std::string keep = error_text(); pse_team_destroy(T); error_text() = keep; return rc; }
    *out = T;
    return 0;
}

extern "C" int pse_team_destroy(pse_team *T) {
    if (!T) return 0;
    for (pse_handle *h : T->m) {   // members take their own side stream back (an in-process team shared member 0's)
        if (h->side != h->side_owned) {
            h->side = h->side_owned; h->side_on = false; h->wstream = h->stream;
            // the rocFFT execution infos were bound to member 0's side stream: rebind, or the next call with the wave chain on
            // the main stream finds (side_on, wstream) already as it wants them and the transforms run on the stale stream
            (void)bind_wave_stream(h);
        }
    }
    T->streams.synchronize();   // the communication stream is idle before the communicator goes, and goes after it
    if (T->nccl) ncclCommDestroy(T->nccl);
    delete T;
    return 0;
}

extern "C" int pse_team_debug_solo(pse_team *T, int slab_rank) {
    if (!T) return fail(PSE_ERR_INVALID, "null team");
    if (slab_rank < 0) { T->solo = -1; T->solo_m.clear(); return 0; }
    if (!loopback(*T)) return fail(PSE_ERR_INVALID, "pse_team_debug_solo needs an in-process team");
    for (pse_handle *h : T->m)
        if (h->slab_rank == slab_rank) { T->solo = slab_rank; T->solo_m = {h}; return 0; }
    return fail(PSE_ERR_INVALID, "no member with slab rank %d", slab_rank);
}

// the members of an in-process team run one Lanczos iteration together: they must apply the same operator
static int team_same_operator(const pse_team *T) {
    for (size_t r = 1; r < T->m.size(); ++r)
        if (T->m[r]->lz_op != T->m[0]->lz_op)
            return fail(PSE_ERR_INVALID, "team members use different Lanczos operators (member 0: %d, member %zu: %d): pse_set_lanczos_operator on every member",
                        T->m[0]->lz_op, r, T->m[r]->lz_op);
    return 0;
}

extern "C" int pse_team_mobility(pse_team *T, const pse_double4 *const *pos, const pse_double4 *const *force,
                                 pse_double4 *const *vel, const unsigned *group, unsigned N, int parts) {
    if (!T || !pos || !force || !vel) return fail(PSE_ERR_INVALID, "null argument");
    std::vector<Args> a;
    for (size_t r = 0; r < T->m.size(); ++r) a.push_back(Args{(const double4 *)pos[r], (const double4 *)force[r], (double4 *)vel[r]});
    return do_mobility(*T, a, group, N, parts);
}

extern "C" int pse_team_brownian_velocity(pse_team *T, const pse_double4 *const *pos, const pse_double4 *const *force,
                                          pse_double4 *const *vel, const unsigned *group, unsigned N, double kT, double dt,
                                          unsigned timestep, int *lanczos_m) {
    if (!T || !pos || !force || !vel) return fail(PSE_ERR_INVALID, "null argument");
    TRY(team_same_operator(T));
    std::vector<Args> a;
    for (size_t r = 0; r < T->m.size(); ++r) a.push_back(Args{(const double4 *)pos[r], (const double4 *)force[r], (double4 *)vel[r]});
    return do_brownian(*T, a, group, N, kT, dt, timestep, lanczos_m);
}

extern "C" int pse_team_step(pse_team *T, pse_double4 *const *pos, pse_double4 *const *vel, pse_double3 *const *accel,
                             pse_int3 *const *image, const pse_double4 *const *net_force, const unsigned *group, unsigned N,
                             double kT, double dt, unsigned timestep, double shear_rate, int *lanczos_m) {
    if (!T || !pos || !vel || !accel || !image || !net_force) return fail(PSE_ERR_INVALID, "null argument");
    TRY(team_same_operator(T));
    std::vector<StepArgs> a;
    for (size_t r = 0; r < T->m.size(); ++r)
        a.push_back(StepArgs{(double4 *)pos[r], (double4 *)vel[r], (double3 *)accel[r], (int3 *)image[r], (const double4 *)net_force[r]});
    return do_step(*T, a, group, N, kT, dt, timestep, shear_rate, lanczos_m);
}

extern "C" int pse_team_step_local(pse_team *T, pse_double4 *const *pos, pse_double4 *const *vel, pse_double3 *const *accel, pse_int3 *const *image,
                                   const pse_double4 *const *net_force, unsigned int *const *tag, unsigned int *const *n_local, double kT,
                                   double dt, unsigned int timestep, double shear_rate, int integrate, int *lanczos_m) {
    if (!T || !pos || !vel || !accel || !image || !net_force || !tag || !n_local) return fail(PSE_ERR_INVALID, "null argument");
    TRY(team_same_operator(T));
    std::vector<LocalCaller> ca;
    for (size_t r = 0; r < T->m.size(); ++r)
        ca.push_back(LocalCaller{(double4 *)pos[r], (double4 *)vel[r], (double3 *)accel[r], (int3 *)image[r], (const double4 *)net_force[r], tag[r], n_local[r]});
    return local_call(*T, ca, kT, dt, timestep, shear_rate, integrate, lanczos_m);
}

// Every particle to the rank that owns it under the CURRENT box (after pse_set_box has taken the tilt through a Lees-Edwards flip):
// what HOOMD's domain decomposition does when the box is re-mapped (PSEv1/VariantShearFunction.cc:34-43 drives the flip).  Two
// exchanges of the team's own transfer list around three kernels (pse_local.hip); the host sizes the second exchange from the count
// rows of the first, so this call WAITS twice -- it runs once per unit of strain.
static int redistribute_local(pse_team &T, const std::vector<LocalCaller> &ca) {
    if (T.G < 2) return fail(PSE_ERR_INVALID, "pse_team_redistribute_local needs a team of >= 2 ranks");
    if (T.solo >= 0) return fail(PSE_ERR_INVALID, "pse_team_redistribute_local: not in solo mode");
    const int G = T.G, row = (G + 2 + 1) & ~1;      // ints per count row: G counts, capacity, particle count (+ padding to whole doubles)
    for (size_t r = 0; r < T.m.size(); ++r) {
        pse_handle *h = T.m[r];
        if (!h->loc.on) return fail(PSE_ERR_INVALID, "pse_team_redistribute_local: member %zu was not created with local_rows", r);
        if (h->loc.err_host[0]) return fail(PSE_ERR_INVALID, "owned-particle rank %d: an earlier step failed on the device (flags %d)", h->slab_rank, h->loc.err_host[0]);
        const LocalCaller &c = ca[r];
        if (!c.pos || !c.vel || !c.accel || !c.image || !c.force || !c.tag || !c.n_local) return fail(PSE_ERR_INVALID, "null array");
        HIPCHK(hipSetDevice(h->device));
        if (!h->loc.rd_send) {
            const size_t nrec = (size_t)h->loc.g.c_own * LOCAL_REC;
            TRY(dmalloc(h, &h->loc.rd_send, nrec)); TRY(dmalloc(h, &h->loc.rd_recv, nrec));
            TRY(dmalloc(h, &h->loc.rd_rows, (size_t)G * row)); TRY(dmalloc(h, &h->loc.rd_off, (size_t)2 * G));
            HIPCHK(h->pinned.make((void **)&h->loc.rd_host, ((size_t)G * row + 2 * G) * sizeof(int)));
            h->info.device_bytes = h->bytes;
        }
    }
    // (1) new owners and the count row of every rank
    for (size_t r = 0; r < T.m.size(); ++r) {
        pse_handle *h = T.m[r];
        HIPCHK(hipSetDevice(h->device));
        int *mine = h->loc.rd_rows + (size_t)h->slab_rank * row;
        HIPCHK(hipMemsetAsync(h->loc.rd_rows, 0, (size_t)G * row * sizeof(int), h->stream));
        launch_redist_count(ca[r], h->loc.g, h->dbox, h->nc, h->keys, mine, h->loc.err, h->stream);
        HIPCHK(hipMemcpyAsync(mine + G, &h->loc.g.c_own, sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(mine + G + 1, ca[r].n_local, sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    }
    TRY(team_run_exchange(T, [&](pse_handle *h) {
        std::vector<Xfer> ops;
        for (int p = 0; p < G; ++p) {
            if (p == h->slab_rank) continue;
            ops.push_back(Xfer{(const double *)(h->loc.rd_rows + (size_t)h->slab_rank * row), (size_t)row / 2, p,
                               (double *)(h->loc.rd_rows + (size_t)p * row), (size_t)row / 2, p});
        }
        return ops; }, false, DIAG_GHOST));
    for (pse_handle *h : T.m) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipMemcpyAsync(h->loc.rd_host, h->loc.rd_rows, (size_t)G * row * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(h->loc.err_host, h->loc.err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    for (pse_handle *h : T.m) { HIPCHK(hipSetDevice(h->device)); HIPCHK(hipStreamSynchronize(h->stream)); }
    // (2) every rank holds every row: the same verdict everywhere -- nothing moves unless everything fits
    const int *M = T.m[0]->loc.rd_host;
    for (pse_handle *h : T.m)
        if (h->loc.err_host[0]) return fail(PSE_ERR_INVALID, "owned-particle rank %d: flags %d while counting (16: n_local above capacity)", h->slab_rank, h->loc.err_host[0]);
    for (int d = 0; d < G; ++d) {
        long in = 0;
        for (int src = 0; src < G; ++src) in += M[(size_t)src * row + d];
        if (in > M[(size_t)d * row + G])
            return fail(PSE_ERR_INVALID, "redistribution: rank %d would own %ld particles, its arrays hold %d (pse_local_layout rows_own): nothing was moved", d, in, M[(size_t)d * row + G]);
    }
    // (3) pack by destination, exchange exactly those records, unpack into the caller's arrays
    for (size_t r = 0; r < T.m.size(); ++r) {
        pse_handle *h = T.m[r];
        HIPCHK(hipSetDevice(h->device));
        int *off = h->loc.rd_host + (size_t)G * row;     // [G] send offsets, then [G] zeros for the fill counters
        const int *mine = h->loc.rd_host + (size_t)h->slab_rank * row;
        int acc = 0;
        for (int d = 0; d < G; ++d) { off[d] = acc; acc += mine[d]; off[G + d] = 0; }
        HIPCHK(hipMemcpyAsync(h->loc.rd_off, off, 2 * G * sizeof(int), hipMemcpyHostToDevice, h->stream));
        launch_redist_pack(ca[r], h->loc.g, h->keys, h->loc.rd_off, h->loc.rd_off + G, h->loc.rd_send, h->stream);
    }
    TRY(team_run_exchange(T, [&](pse_handle *h) {
        const int me = h->slab_rank;
        const int *Mh = h->loc.rd_host;
        std::vector<Xfer> ops;
        size_t so = 0, ro = 0;
        std::vector<size_t> soff(G), roff(G);
        for (int p = 0; p < G; ++p) { soff[p] = so; so += (size_t)Mh[(size_t)me * row + p]; roff[p] = ro; ro += (size_t)Mh[(size_t)p * row + me]; }
        for (int p = 0; p < G; ++p) {   // (the diagonal block is a local copy in every transport: team_exchange)
            const size_t ns = (size_t)Mh[(size_t)me * row + p] * LOCAL_REC, nr = (size_t)Mh[(size_t)p * row + me] * LOCAL_REC;
            if (ns || nr) ops.push_back(Xfer{h->loc.rd_send + soff[p] * LOCAL_REC, ns, p, h->loc.rd_recv + roff[p] * LOCAL_REC, nr, p});
        }
        return ops; }, false, DIAG_FIRST));
    for (size_t r = 0; r < T.m.size(); ++r) {
        pse_handle *h = T.m[r];
        HIPCHK(hipSetDevice(h->device));
        long in = 0;
        for (int src = 0; src < G; ++src) in += h->loc.rd_host[(size_t)src * row + h->slab_rank];
        launch_redist_unpack(h->loc.rd_recv, (int)in, ca[r], h->stream);
        h->sorted_N = 0; h->nb_valid = false; h->vl_valid = false;
        HIPCHK(hipGetLastError());
    }
    return 0;
}

extern "C" int pse_team_redistribute_local(pse_team *T, pse_double4 *const *pos, pse_double4 *const *vel, pse_double3 *const *accel, pse_int3 *const *image,
                                           pse_double4 *const *net_force, unsigned int *const *tag, unsigned int *const *n_local) {
    if (!T || !pos || !vel || !accel || !image || !net_force || !tag || !n_local) return fail(PSE_ERR_INVALID, "null argument");
    std::vector<LocalCaller> ca;
    for (size_t r = 0; r < T->m.size(); ++r)
        ca.push_back(LocalCaller{(double4 *)pos[r], (double4 *)vel[r], (double3 *)accel[r], (int3 *)image[r], (const double4 *)net_force[r], tag[r], n_local[r]});
    return redistribute_local(*T, ca);
}

extern "C" int pse_team_set_lanczos_extra(pse_team *T, int extra) {
    if (!T) return fail(PSE_ERR_INVALID, "null team");
    if (extra > 32) return fail(PSE_ERR_INVALID, "at most 32 extra Lanczos iterations");
    T->lz_extra = extra < 0 ? -1 : extra;
    return 0;
}

extern "C" int pse_team_local_status(pse_team *T, int *flags) {
    if (!T) return fail(PSE_ERR_INVALID, "null team");
    int any = 0;
    for (size_t r = 0; r < T->m.size(); ++r) {
        pse_handle *h = T->m[r];
        if (!h->loc.on) return fail(PSE_ERR_INVALID, "member %zu is not an owned-particle handle", r);
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->side) HIPCHK(hipStreamSynchronize(h->side));
        int f = 0;
        HIPCHK(hipMemcpy(&f, h->loc.err, sizeof(int), hipMemcpyDeviceToHost));
        h->loc.err_host[0] = f;
        if (flags) flags[r] = f;
        any |= f;
    }
    if (any) return fail(PSE_ERR_INVALID, "owned-particle step failed on the device (flags %d: 1 own rows, 2 ghost rows, 4 message capacity exceeded, "
                         "8 a particle moved beyond the neighbour, 16 n_local above capacity)", any);
    return 0;
}

extern "C" int pse_team_set_diag(pse_team *T, int enabled) {
    if (!T) return fail(PSE_ERR_INVALID, "null team");
    HIPCHK(hipSetDevice(T->m[0]->device));
    if (enabled && T->diag.ev.empty()) {
        T->diag.ev.resize(2 * PSE_DIAG_MAX + 4);
        for (hipEvent_t &e : T->diag.ev) HIPCHK(T->events.make(&e));
    }
    T->diag.on = enabled != 0;
    T->diag.n = 0;
    return 0;
}
extern "C" int pse_team_get_diag(pse_team *T, pse_team_diag *out) {
    if (!T || !out) return fail(PSE_ERR_INVALID, "null argument");
    memset(out, 0, sizeof *out);
    if (!T->diag.on) return fail(PSE_ERR_INVALID, "diagnosis is off (pse_team_set_diag)");
    pse_handle *h = T->solo >= 0 ? T->solo_m[0] : T->m[0];
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->side) HIPCHK(hipStreamSynchronize(h->side));
    out->n_exchanges = T->diag.n;
    for (int q = 0; q < T->diag.n; ++q) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, T->diag.ev[2 * q], T->diag.ev[2 * q + 1]) != hipSuccess) ms = 0.0f;
        out->kind[q] = T->diag.kind[q]; out->lane[q] = T->diag.lane[q]; out->device_us[q] = 1e3 * ms; out->host_us[q] = T->diag.host_us[q];
        out->bytes[q] = T->diag.bytes[q];
    }
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, T->diag.ev[2 * PSE_DIAG_MAX], T->diag.ev[2 * PSE_DIAG_MAX + 1]) == hipSuccess) out->main_lane_ms = ms;
    if (T->diag.side_used && hipEventElapsedTime(&ms, T->diag.ev[2 * PSE_DIAG_MAX + 2], T->diag.ev[2 * PSE_DIAG_MAX + 3]) == hipSuccess) out->side_lane_ms = ms;
    out->critical_path_ms = out->main_lane_ms;
    return 0;
}
