// The life cycle of the engine handle (include/pse_amd.h): pse_create with its rocFFT plans, cell grid and grid placement, the setters
// and getters of the handle's state, pse_destroy.  Everything the handle acquires -- here, or later in the driver (pse_capi.hip) -- is
// made through one of its owners (pse_handle.h), which is what releases it; the one exception is place_grids, whose candidates are
// raw until one pair of them is kept.  All workspaces are allocated once, in pse_create (the reference cudaMalloc/cudaFree's
// ~109 N Scalar4 every step).  Host code: the kernels are behind the launch wrappers of the kernel units.
#include <hip/hip_runtime.h>
#include <rocfft/rocfft.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "pse_forces.h"
#include "pse_handle.h"

static std::once_flag g_fft_once;

// The Lanczos operator of the handle (pse_set_lanczos_operator): it travels with the pair list -- nb.c64 non-null selects the F64
// instantiations of every kernel that writes or reads the list (pse_kernels.hip), so each launch keeps the mode it was queued with.
static int set_lanczos_op(pse_handle *h, int op) {
    if (op == PSE_LANCZOS_FP64 && h->nb.cap > 0 && !h->nb64) {   // (no pair list: every mat-vec walks the cells with the exact f, g already)
        HIPCHK(hipSetDevice(h->device));
        TRY(dmalloc(h, &h->nb64, nb_list64_bytes((size_t)h->n_pad + 1024, h->nb.cap) / sizeof(double4)));   // the geometry of nb.data
        h->info.device_bytes = h->bytes;
    }
    if (op != h->lz_op) h->nb_valid = false;   // the list in place was written for the other operator
    h->lz_op = op;
    h->nb.c64 = op == PSE_LANCZOS_FP64 ? h->nb64 : nullptr;
    return 0;
}
// The passes that READ the spectra (inverse z, both y passes, the x pass) run 5 - 20 % faster or slower depending on where the driver
// placed the two grids -- a property of the allocation that holds for the life of the buffers (round 5: the two speeds of the 512^3 x
// pass; round 6: at 256^3 the inverse y + z passes take 0.293 - 0.329 ms on six pairs allocated one after another in one process, the
// step 3.15 - 3.26 ms from process to process; at 512^3 the FIRST pair of a process is the slow one, 4.60 ms for the three passes
// against 3.98 - 4.05 on the next five: docs/HISTORY.md).  A planner's answer: with the first pair in place, allocate more
// pairs (all alive at once, so that they ARE elsewhere), time the x pass + the inverse y + z passes on each, keep the fastest and free the rest.
// Only for grids large enough to matter, only while the device has room for all the candidates; results do not depend on the choice.
static int place_grids(pse_handle *h, size_t nr, size_t ncx) {
    const DGrid &G = h->G;
    const size_t bytes_r = 3 * nr * sizeof(double), bytes_c = 3 * ncx * sizeof(double2);
    int K = h->tun.place_trials;
    if (K < 2 || bytes_c < ((size_t)96 << 20)) return 0;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    K = (int)std::min<size_t>((size_t)K, 1 + free_b / 4 / (bytes_r + bytes_c));   // the candidates may take a quarter of what is free
    if (K < 2) return 0;
    struct Cand { double *r = nullptr; double2 *c = nullptr; float t = 1e30f; } cand[12];
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    int best = 0, got = 0, rc = 0;
    for (int k = 0; k < K && rc == 0; ++k) {
        Cand &c = cand[k];
        if (k == 0) { c.r = h->rgrid; c.c = h->cgrid; }           // the pair the engine already holds
        else {
            if (hipMalloc((void **)&c.r, bytes_r) != hipSuccess) { (void)hipGetLastError(); c.r = nullptr; break; }
            if (hipMalloc((void **)&c.c, bytes_c) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(c.r); c.r = nullptr; break; }
        }
        ++got;
        auto probe = [&]() -> int {
            HIPCHK(hipMemsetAsync(c.r, 0, bytes_r, h->stream));
            HIPCHK(hipMemsetAsync(c.c, 0, bytes_c, h->stream));
            double *zr[3]; double2 *zs[3];
            for (int q = 0; q < 3; ++q) { zr[q] = c.r + q * nr + (size_t)G.hl * G.Ny * G.Nz; zs[q] = c.c + q * ncx; }
            const ScaleArgs sa = scale_args(h, false, 0.0, 1.0, 0);
            for (int it = 0; it < 4; ++it) {                      // (the first one untimed)
                HIPCHK(hipEventRecord(e0, h->stream));
                if (h->xfuse) launch_xfft_scale(c.c, c.c + ncx, c.c + 2 * ncx, G, h->dbox, sa, h->twiddle, h->stream);   // (zeros in, zeros out)
                launch_yfft(c.c, G, true, h->twiddle_y, h->stream, h->tun.yfft_kb);
                launch_zfft(zr, zs, G.Nx * G.Ny, G.Nz, G.Nzp, true, h->twiddle_z, h->stream);
                HIPCHK(hipEventRecord(e1, h->stream));
                HIPCHK(hipEventSynchronize(e1));
                float ms = 0;
                HIPCHK(hipEventElapsedTime(&ms, e0, e1));
                if (it && ms < c.t) c.t = ms;
            }
            return 0;
        };
        rc = probe();
        if (h->tun.verbose) fprintf(stderr, "grid placement %d: real %p spectra %p: x + inverse y + z passes %.4f ms\n", k, (void *)c.r, (void *)c.c, c.t);
        if (rc == 0 && c.t < cand[best].t) best = k;
        // about one pair in six is of the fast kind (5 - 8 % below the rest, which lie within 2 - 3 % of one another): once one has
        // shown up there is nothing more to find
        if (rc == 0 && got >= 3) {
            float worst = 0.0f;
            for (int q = 0; q < got; ++q) worst = std::max(worst, cand[q].t);
            if (cand[best].t < 0.95f * worst) break;
        }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (rc) best = 0;
    for (int k = 1; k < got; ++k) if (k != best) { (void)hipFree(cand[k].r); (void)hipFree(cand[k].c); }
    if (best != 0) {   // the handle owns the kept pair in place of its first one
        h->arrays.replace(cand[0].r, cand[best].r); h->arrays.replace(cand[0].c, cand[best].c);
        (void)hipFree(cand[0].r); (void)hipFree(cand[0].c); h->rgrid = cand[best].r; h->cgrid = cand[best].c;
    }
    h->place_tried = got; h->place_ms_first = cand[0].t; h->place_ms_kept = cand[best].t;
    if (h->tun.verbose) fprintf(stderr, "grid placement: kept %d of %d (%.4f ms; the first one %.4f)\n", best, got, cand[best].t, cand[0].t);
    return rc;
}
static void set_dbox(pse_handle *h) {
    h->dbox = DBox{h->box.Lx, h->box.Ly, h->box.Lz, h->box.xy, 1.0 / h->box.Lx, 1.0 / h->box.Ly, 1.0 / h->box.Lz};
}

// cells of at least rcut perpendicular width for tilts up to gamma; a dimension with fewer than 3 cells uses 1
int cells_for(const Box &box, double rc, double gamma, int n_slabs, int bz_want, DCells &out, int xpad) {
    const double wx = box.Lx / std::sqrt(1.0 + gamma * gamma), wy = box.Ly, wz = box.Lz;
    if (rc > 0.5 * wx * (1 + 1e-12) || rc > 0.5 * wy * (1 + 1e-12) || rc > 0.5 * wz * (1 + 1e-12))
        return fail(PSE_ERR_INVALID, "real-space cutoff %.4f exceeds half the box width (%.4f, %.4f, %.4f at tilt %.3f): "
                    "the minimum-image near field needs rcut <= L/2; increase xi", rc, wx, wy, wz, gamma);
    auto n = [&](double w) { int c = (int)std::floor(w / rc); if (c < 3) c = 1; if (c > 1024) c = 1024; return c; };
    out = DCells{n(wx), n(wy), n(wz), 0, 1, xpad};
    // Blocks of six cells along z in the storage order (pse_device.h; PSE_CELL_BZ=b at pse_create overrides, 0 = plain (x, y, z) order).
    // Measured at the metric point: the pair-list mat-vec 0.163 -> 0.153 ms (a wave's gathers come from ~95 cells instead of
    // ~130), the cell pass 0.60 -> 0.62 ms (lanes of a wave no longer walk the same z lines): about 1 % per step in four of four
    // paired bench runs.
    out.bz = (bz_want > 0 && out.nz >= 2 * bz_want) ? bz_want : out.nz;
    out.nzb = (out.nz + out.bz - 1) / out.bz;
    if (n_slabs > 1) {
        // cell slabs coincide with grid slabs: every rank owns ncx/G whole cell layers = one contiguous row range
        const int c = (int)std::floor(wx / rc) / n_slabs * n_slabs;
        if (c < 3 || c < n_slabs)
            return fail(PSE_ERR_INVALID, "box too small to split the near field over %d ranks: only %d cells of width >= rcut "
                        "fit along x", n_slabs, (int)std::floor(wx / rc));
        out.nx = std::min(c, 1024 / n_slabs * n_slabs);
    }
    return 0;
}
static double near_radius(const pse_handle *h) { return h->d.rcut + h->skin_max; }   // cells are as wide as the kept list reaches
static int set_cells(pse_handle *h, double gamma) {
    DCells nc;
    TRY(cells_for(h->box, near_radius(h), gamma, h->n_slabs, h->tun.cell_bz, nc, h->loc.on ? 1 : 0));
    h->nc = nc;
    h->cell_gamma = gamma;
    h->nc_wide = h->skin_max > 0.0;
    return 0;
}

extern "C" int pse_destroy(pse_handle *h) {
    if (!h) return 0;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (DeviceObject *t : h->topologies) delete t;
    h->topologies.clear();
    h->fft.release();      // the plans and the execution infos before the work buffer the infos are bound to
    h->arrays.release();
    delete h;              // (events, the side stream -- after the synchronise above --, pinned buffers)
    return 0;
}

// *dst = [N] exp(-2 pi i m / N) on the device, rounded from long double
static int make_twiddle(pse_handle *h, double2 **dst, int N) {
    std::vector<double2> tw(N);
    for (int m = 0; m < N; ++m) {
        const long double ang = -2.0L * 3.14159265358979323846264338327950288L * m / N;
        tw[m] = make_double2((double)cosl(ang), (double)sinl(ang));
    }
    TRY(dmalloc(h, dst, (size_t)N));
    HIPCHK(hipMemcpy(*dst, tw.data(), N * sizeof(double2), hipMemcpyHostToDevice));
    return 0;
}
// rocFFT runs where the wave chain runs: whoever changes h->wstream (pse_set_stream, the driver's choice of lane, a team that hands a
// side stream back) rebinds the two execution infos, or the transforms stay on the stale stream
int bind_wave_stream(pse_handle *h) {
    if (h->info_fwd) FFTCHK(rocfft_execution_info_set_stream(h->info_fwd, h->wstream));
    if (h->info_inv) FFTCHK(rocfft_execution_info_set_stream(h->info_inv, h->wstream));
    return 0;
}

static int make_plans(pse_handle *h) {
    std::call_once(g_fft_once, [] { rocfft_setup(); });
    const DGrid &G = h->G;
    size_t work = 0, w = 0;
    h->xfuse = xfuse_supported(G.Nx) && !h->tun.no_xfuse;   // x axis by k_xfft_scale (also after the slab transpose)
    if (h->xfuse) TRY(make_twiddle(h, &h->twiddle, G.Nx));
    // the y transforms of a single GPU's grid by the own in-place pass where rocFFT's strided pass is slow (not a power of two)
    const bool z_ok = h->tun.own_z > 0 && zfft_supported(G.Nz);
    h->own_y = h->xfuse && h->grid_slabs == 1 && h->tun.own_y > 0 &&
               (yfft_supported(G.Ny) || (h->tun.own_y_pow2 && yfft_regs_supported(G.Ny, G.Nz, z_ok)));
    // a slab rank: the own y pass for ANY smooth Ny -- it writes the all-to-all blocks directly (no pack / unpack pass)
    h->own_y_slab = h->xfuse && h->grid_slabs > 1 && h->tun.own_y > 0 && yfft_possible(G.Ny);
    h->own_z = z_ok && (h->own_y || h->own_y_slab);   // (where rocFFT's plan is its 1-D z plan)
    if (h->own_z) {
        if (G.Nz == G.Nx) h->twiddle_z = h->twiddle;
        else TRY(make_twiddle(h, &h->twiddle_z, G.Nz));
    }
    if (h->own_y || h->own_y_slab) {
        if (G.Ny == G.Nx) h->twiddle_y = h->twiddle;
        else TRY(make_twiddle(h, &h->twiddle_y, G.Ny));
    }
    // real grid rows hold Nz doubles, spectrum rows Nzp >= Nz/2 + 1 complex numbers (padded to 128 bytes)
    auto real_plans = [&](size_t dims, const size_t *len, size_t batch) -> int {
        size_t rs[3] = {1, (size_t)G.Nz, (size_t)G.Ny * G.Nz}, cs[3] = {1, (size_t)G.Nzp, (size_t)G.Ny * G.Nzp};
        const size_t rdist = dims == 1 ? (size_t)G.Nz : (dims == 2 ? (size_t)G.Ny * G.Nz : (size_t)G.Nx * G.Ny * G.Nz);
        const size_t cdist = dims == 1 ? (size_t)G.Nzp : (dims == 2 ? (size_t)G.Ny * G.Nzp : (size_t)G.Nx * G.Ny * G.Nzp);
        rocfft_plan_description df = nullptr, di = nullptr;
        FFTCHK(rocfft_plan_description_create(&df));
        FFTCHK(rocfft_plan_description_create(&di));
        FFTCHK(rocfft_plan_description_set_data_layout(df, rocfft_array_type_real, rocfft_array_type_hermitian_interleaved, nullptr, nullptr,
                                                       dims, rs, rdist, dims, cs, cdist));
        FFTCHK(rocfft_plan_description_set_data_layout(di, rocfft_array_type_hermitian_interleaved, rocfft_array_type_real, nullptr, nullptr,
                                                       dims, cs, cdist, dims, rs, rdist));
        FFTCHK(h->fft.plan(&h->plan_fwd, rocfft_placement_notinplace, rocfft_transform_type_real_forward, dims, len, batch, df));
        FFTCHK(h->fft.plan(&h->plan_inv, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, dims, len, batch, di));
        rocfft_plan_description_destroy(df);
        rocfft_plan_description_destroy(di);
        return 0;
    };
    if (h->own_y) {
        // 1-D real transforms along z of every row; the y transforms are k_fft_cols', the x transforms k_xfft_scale's
        const size_t len1[1] = {(size_t)G.Nz};
        TRY(real_plans(1, len1, (size_t)3 * G.Nx * G.Ny));
    } else if (h->xfuse && h->grid_slabs == 1) {
        // 2-D (y,z) real transforms of all 3 Nx planes in one batch
        const size_t len2[2] = {(size_t)G.Nz, (size_t)G.Ny};
        TRY(real_plans(2, len2, (size_t)3 * G.Nx));
    } else if (h->grid_slabs == 1) {
        // rocFFT lengths are fastest-first: z, y, x.  Real grids [3][Nx][Ny][Nz] -> half spectra [3][Nx][Ny][Nzp].
        const size_t len[3] = {(size_t)G.Nz, (size_t)G.Ny, (size_t)G.Nx};
        TRY(real_plans(3, len, 3));
    } else {
        // slab mode: 2-D (y,z) real transforms of the nxl local planes of one component, then (after the transpose)
        // 1-D complex transforms along x on [Nx][nyl][Nzp]: stride nyl*Nzp, one transform per (y,kz) column
        const size_t len2[2] = {(size_t)G.Nz, (size_t)G.Ny};
        const size_t len1[1] = {(size_t)G.Nz};
        if (h->own_y_slab) TRY(real_plans(1, len1, (size_t)G.nxl * G.Ny));   // z transforms only; the y transforms are k_fft_cols'
        else TRY(real_plans(2, len2, (size_t)G.nxl));
        const size_t lenx[1] = {(size_t)G.Nx};
        size_t stride[1] = {(size_t)h->nyl * G.Nzp};
        rocfft_plan_description desc = nullptr;
        FFTCHK(rocfft_plan_description_create(&desc));
        FFTCHK(rocfft_plan_description_set_data_layout(desc, rocfft_array_type_complex_interleaved,
                                                       rocfft_array_type_complex_interleaved, nullptr, nullptr, 1, stride, 1,
                                                       1, stride, 1));
        FFTCHK(h->fft.plan(&h->plan_x_fwd, rocfft_placement_inplace, rocfft_transform_type_complex_forward, 1, lenx, stride[0], desc));
        FFTCHK(h->fft.plan(&h->plan_x_inv, rocfft_placement_inplace, rocfft_transform_type_complex_inverse, 1, lenx, stride[0], desc));
        rocfft_plan_description_destroy(desc);
        FFTCHK(rocfft_plan_get_work_buffer_size(h->plan_x_fwd, &w)); work = std::max(work, w);
        FFTCHK(rocfft_plan_get_work_buffer_size(h->plan_x_inv, &w)); work = std::max(work, w);
    }
    FFTCHK(rocfft_plan_get_work_buffer_size(h->plan_fwd, &w)); work = std::max(work, w);
    FFTCHK(rocfft_plan_get_work_buffer_size(h->plan_inv, &w)); work = std::max(work, w);
    h->fft_work_bytes = work;
    if (work) TRY(dmalloc(h, (char **)&h->fft_work, work));
    FFTCHK(h->fft.info(&h->info_fwd));
    FFTCHK(h->fft.info(&h->info_inv));
    if (work) {
        FFTCHK(rocfft_execution_info_set_work_buffer(h->info_fwd, h->fft_work, work));
        FFTCHK(rocfft_execution_info_set_work_buffer(h->info_inv, h->fft_work, work));
    }
    return bind_wave_stream(h);
}

static int create_impl(const pse_params *p, pse_handle *h) {
    h->par = *p;
    h->box = Box{p->Lx, p->Ly, p->Lz, p->xy};
    std::string e = select_params(h->box, p->xi, p->error, p->max_strain, p->Nx, p->Ny, p->Nz, p->P, p->rcut, h->d);
    if (!e.empty()) return fail(PSE_ERR_INVALID, "%s", e.c_str());
    if (p->n_max == 0) return fail(PSE_ERR_INVALID, "n_max must be positive");
    TRY(gaussian_fits(h->d, h->d.hx, h->d.hy, h->d.hz));
    if (!(std::fabs(p->xy) <= 0.5 * (1.0 + 1e-9)))
        return fail(PSE_ERR_INVALID, "tilt xy = %g outside [-0.5, 0.5]: HOOMD flips the box there, and the sequential minimum image "
                    "(PSEv1/Mobility.cu:648) is exact only up to that tilt", p->xy);
    const Derived &d = h->d;
    if (p->device >= 0) { HIPCHK(hipSetDevice(p->device)); h->device = p->device; }
    else HIPCHK(hipGetDevice(&h->device));
    h->n_max = (int)p->n_max;
    set_dbox(h);
    h->n_slabs = std::max(1, p->n_slabs);
    h->loc.on = p->local_rows != 0;
    if (h->loc.on && h->n_slabs < 2) return fail(PSE_ERR_INVALID, "local_rows needs n_slabs >= 2 (an owned-particle rank is a member of a team)");
    roctx_lookup();   // PSE_ROCTX: looked up here, once per process
    {   // the developer switches: the environment is read here and nowhere else
        auto ienv = [](const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; };
        auto &t = h->tun;
        t.cell_bz = std::min(16, std::max(0, ienv("PSE_CELL_BZ", 6)));   // n_cells_alloc pads every z line by up to 15 cells
        if (const char *v = getenv("PSE_SKIN")) t.skin = atof(v);
        t.overlap = ienv("PSE_OVERLAP", 1);   // (Brownian steps fork too: with the lighter pair-list mat-vec the far-field chain fits beside the Lanczos chain, 3.23 -> 3.11 ms; rounds 4-5: a loss)
        t.no_xfuse = getenv("PSE_NO_XFUSE") != nullptr;
        t.own_y = ienv("PSE_OWN_Y", 1); t.own_y_pow2 = ienv("PSE_OWN_Y_POW2", 1); t.yfft_kb = ienv("PSE_YFFT_KB", 4); t.own_z = ienv("PSE_OWN_Z", 1); t.yslab_regs = ienv("PSE_YSLAB_REGS", 1);
        if (const char *v = getenv("PSE_WAVE_MODE")) t.wave_mode = !strcmp(v, "slab") ? 1 : (!strcmp(v, "replicated") ? 2 : 0);
        t.spread_tz = ienv("PSE_SPREAD_TZ", 0); t.spread_nw = ienv("PSE_SPREAD_NW", 0);
        t.gather_bz = ienv("PSE_GATHER_BZ", 0); t.xmix_runtime = ienv("PSE_XMIX", 0) == 1; t.xfft_small_wide = ienv("PSE_XFFT_SMALL_KB", 2) == 8;
        t.verbose = ienv("PSE_VERBOSE", 0) > 0;
        t.team_sstep = ienv("PSE_TEAM_SSTEP", 1) > 0;
        t.lz_extra = std::max(0, std::min(32, ienv("PSE_LANCZOS_EXTRA", 2)));
        t.place_trials = std::max(0, std::min(12, ienv("PSE_PLACE_TRIALS", 10)));
        t.vq = ienv("PSE_VQ", 1);
        if (const char *v = getenv("PSE_LANCZOS_OP")) t.lz_op = !strcmp(v, "fp64") ? PSE_LANCZOS_FP64 : PSE_LANCZOS_RECORDS16;
        t.rows24 = ienv("PSE_ROWS24", 1);
        if (const char *v = getenv("PSE_TEAM_SCHED")) {
            int a = 1, b = 2, c = 3;
            if (sscanf(v, "%d,%d,%d", &a, &b, &c) == 3) { t.team_sched[0] = a; t.team_sched[1] = b; t.team_sched[2] = c; }
        }
        h->sw.force_tz = t.spread_tz; h->sw.force_nw = t.spread_nw; h->sw.force_bz = t.gather_bz;
    }
    {
        // Neighbour list across steps: on by default with the reference's r_buff = 0.4 (PSEv1/integrate.py:60), single GPU, table
        // in LDS, box wide enough for rcut + skin; PSE_SKIN overrides (0: off), pse_set_neighbor_skin may lower it later.
        double skin = h->tun.skin;
        const int nint = (int)std::ceil(d.rcut * RS_PER_UNIT) + 1;
        const double gam = std::max(std::fabs(p->xy), p->max_strain);
        const double wmin = std::min(std::min(h->box.Lx / std::sqrt(1.0 + gam * gam), h->box.Ly), h->box.Lz);
        if (!(skin > 0.0) || h->n_slabs > 1 || !mreal_table_in_lds(nint * 2 * RS_NCOEF) || d.rcut + skin > 0.5 * wmin)
            skin = 0.0;
        h->skin = h->skin_max = skin;
    }
    TRY(set_cells(h, std::max(std::fabs(p->xy), p->max_strain)));
    fill_info(d, &h->info);
    h->info.ncell_x = h->nc.nx; h->info.ncell_y = h->nc.ny; h->info.ncell_z = h->nc.nz;

    DGrid &G = h->G;
    G.Nx = d.Nx; G.Ny = d.Ny; G.Nz = d.Nz; G.Nzh = d.Nz / 2 + 1; G.P = d.P;
    G.Nzp = (G.Nzh + 7) & ~7;   // spectrum rows padded to 128 bytes: the x pass reads and writes whole aligned lines
    h->n_slabs = std::max(1, p->n_slabs);
    h->slab_rank = h->n_slabs > 1 ? p->slab_rank : 0;
    if (h->slab_rank < 0 || h->slab_rank >= h->n_slabs) return fail(PSE_ERR_INVALID, "slab_rank outside [0, n_slabs)");
    // Far field of a team: slab-decomposed (2 all-to-alls per evaluation), or kept whole on every rank with only the near
    // field and Lanczos sharded.  With two ranks the all-to-all is one xGMI link each way (101 MB per direction at 256^3:
    // ~2 ms, longer than the far field itself), so two ranks replicate the far field; PSE_WAVE_MODE=slab|replicated overrides.
    h->grid_slabs = h->n_slabs;
    if (h->n_slabs > 1) {
        const bool replicate = h->tun.wave_mode ? h->tun.wave_mode == 2 : h->n_slabs == 2;
        if (replicate && !h->loc.on) h->grid_slabs = 1;   // (an owned-particle rank has no particles to spread a whole grid with)
    }
    if (h->grid_slabs > 1) {
        if (d.Nx % h->grid_slabs || d.Ny % h->grid_slabs)
            return fail(PSE_ERR_INVALID, "slab decomposition needs Nx and Ny divisible by the number of ranks (%d x %d over %d)",
                        d.Nx, d.Ny, h->grid_slabs);
        if (d.Nx / h->grid_slabs < d.P)
            return fail(PSE_ERR_INVALID, "slabs of %d planes are thinner than the support P = %d", d.Nx / h->grid_slabs, d.P);
    }
    const int grid_rank = h->grid_slabs > 1 ? h->slab_rank : 0;
    G.nxl = d.Nx / h->grid_slabs; G.x0 = grid_rank * G.nxl;
    // the gather of a particle is done by the rank whose slab holds the particle; its support reaches (P-1)/2 planes
    // below and (P+1)/2 planes above that slab: copies of the neighbours' planes are stored around the own ones
    G.hl = h->grid_slabs > 1 ? (d.P - 1) / 2 : 0;
    G.nhalo = h->grid_slabs > 1 ? (d.P + 1) / 2 : 0;
    h->nyl = d.Ny / h->grid_slabs; h->y0 = grid_rank * h->nyl;
    G.hx = d.hx; G.hy = d.hy; G.hz = d.hz;
    const double c = 2.0 * d.xi * d.xi / d.eta;
    G.expfac = c;                                      // PSEv1/Brownian.cu:829
    G.prefac = (c / M_PI) * std::sqrt(c / M_PI);       // PSEv1/Brownian.cu:828

    // particle arrays are padded so that equal row chunks of every rank fit (all-gather inside Lanczos)
    const size_t n = ((size_t)h->n_max + h->n_slabs - 1) / h->n_slabs * h->n_slabs;
    h->n_pad = (int)n;
    TRY(dmalloc(h, &h->keys, n)); TRY(dmalloc(h, &h->keys_s, n)); TRY(dmalloc(h, &h->vals, n));
    TRY(dmalloc(h, &h->perm, n)); TRY(dmalloc(h, &h->tag_s, n));

    // size the cell arrays for zero tilt (most cells)
    {
        const double rc = d.rcut;
        auto cnt = [&](double w) { int c2 = (int)std::floor(w / rc); if (c2 < 3) c2 = 1; if (c2 > 1024) c2 = 1024; return (size_t)c2; };
        h->n_cells_alloc = cnt(h->box.Lx) * cnt(h->box.Ly) * (cnt(h->box.Lz) + 16) + cnt(h->box.Lx);   // + the padding of the last z block (bz <= 16), + one empty cell per x layer (xpad)
    }
    TRY(dmalloc(h, &h->cell_off, h->n_cells_alloc + 1));
    h->sort_tmp_bytes = cell_sort_temp_bytes(h->n_cells_alloc);
    TRY(dmalloc(h, (char **)&h->sort_tmp, h->sort_tmp_bytes));
    // the counters every call starts from zero, side by side: [bin counts | flags[0], flags[1] | cell counts] -- one memset
    // covers what a call needs (a call that checks the kept list stops after flags[0]: flags[1] is the mark of its build)
    const size_t nbins = (size_t)((d.Nx + 7) / 8) * ((d.Ny + 7) / 8) * ((d.Nz + 7) / 8);
    const bool fast_far = d.P >= 4 && d.P <= FAR_PMAX;
    // layout in ints: [0, B - 1) bin counts (incl. sentinel, padded) | B - 1: flags[0] | B: flags[1] | B + 4 ...: cell counts.  B and every
    // memset size are multiples of four ints: a memset that is not a multiple of 16 bytes takes two fill kernels.
    h->cnt_bins = ((fast_far ? nbins + 1 : 0) + 1 + 3) & ~(size_t)3;   // B
    constexpr size_t LAYER_INTS = (size_t)LOCAL_MAX_LAYERS * LOCAL_LAYER_SLOTS;   // (the per-layer counts of an owned-particle rank's sort)
    TRY(dmalloc(h, &h->cnt_block, h->cnt_bins + 4 + h->n_cells_alloc + 1 + 8 + LOCAL_NCOUNTER + 2 + LAYER_INTS + 4));
    h->loc.counters = h->cnt_block + ((h->cnt_bins + 4 + h->n_cells_alloc + 1 + 8 + 1) & ~(size_t)1);   // 8-byte aligned
    h->loc.layer_cnt = h->loc.counters + LOCAL_NCOUNTER;
    h->loc.zero_ints = ((size_t)(h->loc.layer_cnt - h->cnt_block) + LAYER_INTS + 3) & ~(size_t)3;
    if (h->nc.nx > LOCAL_MAX_LAYERS && p->local_rows) return fail(PSE_ERR_INVALID, "more than %d cell layers along x", LOCAL_MAX_LAYERS);
    h->vl.flags = h->cnt_block + h->cnt_bins - 1;
    h->gate_word = h->cnt_block + h->cnt_bins + 1;   // (B + 1: between flags[1] and the cell counts; no memset covers it alone)
    h->cell_cnt = h->cnt_block + h->cnt_bins + 4;
    if (fast_far) {   // fast far-field path: bin-ordered 64-byte records
        h->sw.fb.cnt = h->cnt_block;
        TRY(dmalloc(h, (char **)&h->sw.rec_t, (n + 64) * 64));   // 64-byte records (idle lanes read past the last one)
        TRY(dmalloc(h, &h->sw.fb.rank_s, n));
        TRY(dmalloc(h, &h->sw.fb.off, nbins + 1));
        h->sw.fb.tmp_bytes = bin_scan_temp_bytes(nbins);
        TRY(dmalloc(h, (char **)&h->sw.fb.tmp, h->sw.fb.tmp_bytes));
    }
    std::vector<double> coef;
    build_realspace_table(d.xi, d.rcut, coef, h->n_intervals);
    TRY(dmalloc(h, &h->coef, coef.size()));
    HIPCHK(hipMemcpy(h->coef, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice));
    TRY(dmalloc(h, &h->nb.cnt, n));
    {   // per-step pair list: capacity from the mean neighbour count
        const double vol = h->box.Lx * h->box.Ly * h->box.Lz;
        // particles of the whole box behind the capacity (an owned-particle rank holds its slab + four ghost layers of it, with slack)
        const double n_box = h->loc.on ? (double)n * h->n_slabs * (h->nc.nx / h->n_slabs) / (h->nc.nx / h->n_slabs + 4.0) : (double)n;
        const double nbar = n_box / vol * 4.18879020478639 * d.rcut * d.rcut * d.rcut;
        int cap = (int)std::ceil(1.5 * nbar + 16.0);
        cap = (std::max(16, std::min(cap, 256)) + 3) & ~3;   // whole groups of four slots
        const double bytes = (double)cap * (double)n * 20.0;
        if (bytes > 32e9 || n >= ((size_t)1 << 27)) cap = 0;   // too large: mat-vecs always walk the cells
        h->nb.cap = cap;
        if (cap > 0) {
            TRY(dmalloc(h, &h->nb.data, nb_list_bytes(n + 1024, cap)));   // + the padding of up to three row ranges to whole workgroups (RowMap)
        }
        if (cap == 0) h->skin = h->skin_max = 0.0;
        if (h->skin_max > 0.0) {
            const double rs = d.rcut + h->skin_max, nbar_v = n_box / vol * 4.18879020478639 * rs * rs * rs;
            h->vl.cap = (std::max(16, std::min((int)std::ceil(2.0 * nbar_v + 32.0), 512)) + 3) & ~3;   // 4 bytes per slot: generous
            h->vl.rskin = rs;
            TRY(dmalloc(h, (char **)&h->vl.idx, verlet_list_bytes(n + 1024, h->vl.cap)));   // + padding rows (the lanes past the last row of the build pass write there)
            TRY(dmalloc(h, &h->vl.cnt, n));
            TRY(dmalloc(h, &h->pos_build, n));
            HIPCHK(h->pinned.make((void **)&h->flags_host, 2 * sizeof(int)));
        }
    }
    TRY(dmalloc(h, &h->pos_s, n)); TRY(dmalloc(h, &h->posf_s, n));
    TRY(dmalloc(h, &h->pv, 3 * n));   // packed (position, force) records of the near-field passes
    TRY(dmalloc(h, &h->f_s, n)); TRY(dmalloc(h, &h->uw_s, n)); TRY(dmalloc(h, &h->ur_s, n));
    TRY(dmalloc(h, &h->ub_s, n)); TRY(dmalloc(h, &h->psi_s, n)); TRY(dmalloc(h, &h->w_s, n));

    const size_t nr = (size_t)(G.nxl + G.hl + G.nhalo) * G.Ny * G.Nz, ncx = (size_t)G.nxl * G.Ny * G.Nzp;
    TRY(dmalloc(h, &h->rgrid, 3 * nr));
    TRY(dmalloc(h, &h->cgrid, 3 * ncx));
    if (h->grid_slabs > 1) { TRY(dmalloc(h, &h->sendbuf, 3 * ncx)); TRY(dmalloc(h, &h->recvbuf, 3 * ncx)); }
    if (h->n_slabs > 1) {
        HIPCHK(h->pinned.make((void **)&h->bounds_host, ((size_t)5 * h->n_slabs + 1) * sizeof(int), hipHostMallocMapped));
        HIPCHK(hipHostGetDevicePointer((void **)&h->bounds_host_dev, h->bounds_host, 0));
        HIPCHK(h->events.make(&h->ev_bounds, hipEventDisableTiming));
        TRY(dmalloc(h, &h->d_bidx, (size_t)5 * h->n_slabs + 1)); TRY(dmalloc(h, &h->d_bounds, (size_t)5 * h->n_slabs + 1));
        TRY(dmalloc(h, &h->utot_s, n));
        TRY(dmalloc(h, &h->sums_all, (size_t)h->n_slabs * LZ_NGRAM));
        if (h->tun.team_sstep && h->nb.cap > 0) {
            TRY(dmalloc(h, &h->w2_s, n)); TRY(dmalloc(h, &h->u_s, n));
        }
    }
    if (h->loc.on) {
        // owned-particle rank: the row space [own | left ghosts | right ghosts] and the messages of the step's first exchange
        auto &L = h->loc;
        const int G_ = h->n_slabs, per = h->nc.nx / G_, depth = 2;
        if (per < depth + 1 || (G_ - 1) * per < 2 * depth)
            return fail(PSE_ERR_INVALID, "an owned-particle rank needs >= %d cell layers of width rcut per rank along x (%d ranks: %d layers each)",
                        G_ == 2 ? 2 * depth : depth + 1, G_, per);
        if (!team_sstep(h))
            return fail(PSE_ERR_INVALID, "an owned-particle rank needs the per-step pair list and the real-space table in LDS (rcut = %.3f, n_max = %d)",
                        d.rcut, h->n_max);
        if ((d.P / 2 + 1.0) / d.Nx > (double)depth / h->nc.nx)
            return fail(PSE_ERR_INVALID, "the spreading support (P = %d on %d planes) reaches beyond the %d ghost cell layers of an owned-particle rank", d.P, d.Nx, depth);
        const int c_g = (int)((double)h->n_max * depth / (per + 2 * depth)) / 256 * 256, c_own = (h->n_max - 2 * c_g) / 256 * 256;
        if (c_g < 256 || c_own < c_g)
            return fail(PSE_ERR_INVALID, "n_max = %d is too small a row capacity for an owned-particle rank (%d layers + 2 x %d ghost layers)", h->n_max, per, depth);
        L.g = LocalGeom{h->slab_rank, G_, per, depth, h->nc.nx, c_own, c_g, c_g};
        L.rows_cap = c_own + 2 * c_g;
        L.msg = (size_t)LOCAL_HDR + (size_t)LOCAL_REC * c_g;
        for (int q = 0; q < 2; ++q) { TRY(dmalloc(h, &L.send[q], L.msg)); TRY(dmalloc(h, &L.recv[q], L.msg)); HIPCHK(hipMemset(L.recv[q], 0, L.msg * sizeof(double))); }
        TRY(dmalloc(h, &L.stage_w1, (size_t)c_g)); TRY(dmalloc(h, &L.stage_w2, (size_t)c_g));
        TRY(dmalloc(h, &L.porig_s, (size_t)c_own)); TRY(dmalloc(h, &L.mass_s, (size_t)c_own)); TRY(dmalloc(h, &L.image_s, (size_t)c_own));
        TRY(dmalloc(h, &L.rows, 1));
        TRY(dmalloc(h, &L.err, 4));
        HIPCHK(hipMemset(L.err, 0, 4 * sizeof(int)));
        HIPCHK(hipMemset(L.rows, 0, sizeof(LocalRows)));
        HIPCHK(h->pinned.make((void **)&L.err_host, 4 * sizeof(int)));
        L.err_host[0] = 0;
    }
    // The wave-space chain (spread -> FFTs -> gather) and the real-space chain (near field + Lanczos) only meet in the
    // final sum: on a single GPU they run on two streams, so latency-bound kernels of one chain fill the gaps of the
    // other and the Lanczos host checks do not stall the far field.  (Teams keep one stream: one RCCL communicator.)
    h->wstream = h->stream;
    // Deterministic evaluations (kT = 0) fork whenever no phase timing is requested: the far-field chain runs on a side stream next
    // to the near field (+3.5 % M.F evaluations per second).  Brownian steps stay on ONE stream by default since the end of round 3:
    // with the build pass at three workgroups per CU, the gather at six and the spread at twelve, every kernel fills the chip on
    // its own and a second chain buys nothing measurable (six paired runs: forked minus one stream between -1.2 % and +1.8 %;
    // PSE_OVERLAP=1 forks them too, -1 never forks).  With pse_set_timing on, everything runs on one stream: per-kernel
    // durations -- the roofline evidence -- are then those of the kernel alone.
    if (h->tun.overlap >= 0) {
        {   // PSE_SIDE_PRIORITY=low|high|default: the far-field lane at the lowest / highest / the default stream priority.  Default: the
            // default priority -- but LOW on an owned-particle rank, whose near field + Lanczos chain is the longer lane by ~100 us at
            // eight ranks: its mat-vecs then lose less to the transforms that run next to them (solo rank, metric point 0.724 -> 0.701 ms,
            // BASELINE config 4 2.72 -> 2.69)
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);   // lo: numerically largest = lowest priority
            const char *pr = getenv("PSE_SIDE_PRIORITY");
            if (!pr || !*pr) pr = h->loc.on ? "low" : "default";
            const int prio = !strcmp(pr, "low") ? lo : hi;
            HIPCHK(h->streams.make(&h->side, hipStreamNonBlocking, !strcmp(pr, "low") || !strcmp(pr, "high") ? &prio : nullptr));
        }
        h->side_owned = h->side;
        HIPCHK(h->events.make(&h->ev_fork, hipEventDisableTiming));
        HIPCHK(h->events.make(&h->ev_join, hipEventDisableTiming));
        h->overlap_all = h->tun.overlap > 0;    // Brownian steps fork unless PSE_OVERLAP=0
    }
    TRY(make_plans(h));
    if (h->tun.place_trials > 1 && h->own_z && h->own_y && h->grid_slabs == 1)
        TRY(place_grids(h, (size_t)(G.nxl + G.hl + G.nhalo) * G.Ny * G.Nz, (size_t)G.nxl * G.Ny * G.Nzp));

    // The basis in 24-byte rows where only the coalesced kernels of the single-GPU pair-list path touch it (k_lz_update, k_mreal_list's own
    // row, k_basis_combine): a quarter of every double4 row they moved was the padding word.  Everything a team, an owned-particle rank,
    // k_lz_block, k_lz_dots or a cell pass reads stays double4 -- so does a handle created with the fp64 operator, whose mat-vec gathers
    // its neighbours' rows from the basis itself.
    h->rows24 = h->n_slabs == 1 && !h->loc.on && h->nb.cap > 0 && h->tun.lz_op != PSE_LANCZOS_FP64 && h->tun.rows24 != 0;
    if (h->rows24) {
        TRY(dmalloc(h, &h->V, ((size_t)(M_MAX + 1) * n * 3 + 3) / 4));   // (counted in double4: three quarters of them)
        h->w24 = reinterpret_cast<double *>(h->V);                       // slot 0 of the basis: x_0 = psi is never copied into it
    } else TRY(dmalloc(h, &h->V, (size_t)(M_MAX + 1) * n));
    // single GPU: the newest Lanczos vector also in 16 bytes per row (vq_pack): what the pair-list mat-vec gathers its neighbours from
    if (h->n_slabs == 1 && !h->loc.on && h->tun.vq > 0) TRY(dmalloc(h, (char **)&h->vq, (size_t)16 * n));
    TRY(dmalloc(h, &h->pv_rows, pair_virial_rows((int)n)));
    TRY(dmalloc(h, &h->scal, (size_t)LZ_NSCAL));
    TRY(dmalloc(h, &h->lz_state, 1));
    HIPCHK(hipMemset(h->lz_state, 0, sizeof(LzState)));
    HIPCHK(h->pinned.make((void **)&h->sc_host, LZ_NSCAL * sizeof(double), hipHostMallocMapped));
    HIPCHK(hipHostGetDevicePointer((void **)&h->sc_host_dev, h->sc_host, 0));
    memset(h->sc_host, 0, LZ_NSCAL * sizeof(double));
    HIPCHK(h->events.make(&h->ev_scal, hipEventDisableTiming));
    if (!h->partials) {
        h->npart_cap = std::max(LZ_NPART, mreal_partials_needed((int)n + 1024));   // + the padding of the row ranges (RowMap)
        TRY(dmalloc(h, &h->partials, (size_t)LZ_NGRAM * h->npart_cap));
    }
    TRY(dmalloc(h, &h->lz_sums, (size_t)2 * LZ_NPART));
    for (auto &ph : h->ph) { HIPCHK(h->events.make(&ph.a)); HIPCHK(h->events.make(&ph.b)); }
    TRY(set_lanczos_op(h, h->tun.lz_op));
    h->info.device_bytes = h->bytes;
    if (h->tun.verbose) {
        // the parameter summary the reference prints at notice level 2 (PSEv1/Stokes.cc:241-252), one block on stderr
        fprintf(stderr, "--- NUFFT Hydrodynamics Statistics ---\nMx: %d\nMy: %d\nMz: %d\nrcut: %.6g\n"
                "Points per radius (x,y,z): %.4g, %.4g, %.4g\n--- Gaussian Spreading Parameters ---\ngauss_m: %.4g\ngauss_P: %d\n"
                "gauss_eta: %.6g\ngauss_w: %.6g\ngauss_gridh (x,y,z): %.6g, %.6g, %.6g\n"
                "--- engine ---\ncells: %d x %d x %d, ranks: %d (far-field slabs %d), device memory: %.2f GB\n",
                d.Nx, d.Ny, d.Nz, d.rcut, d.Nx / h->box.Lx, d.Ny / h->box.Ly, d.Nz / h->box.Lz, d.gaussm, d.P, d.eta,
                d.P * d.hx / 2.0, d.hx, d.hy, d.hz, h->nc.nx, h->nc.ny, h->nc.nz, h->n_slabs, h->grid_slabs, h->bytes / 1e9);
        fprintf(stderr, "grids at: real %p, spectra %p\n", (void *)h->rgrid, (void *)h->cgrid);   // (the x pass at 512^3 has two speeds that go with the allocation: tools/debug/mode_probe.py)
    }
    return 0;
}

extern "C" int pse_create(const pse_params *p, pse_handle **out) {
    if (!p || !out) return fail(PSE_ERR_INVALID, "null argument");
    *out = nullptr;
    pse_handle *h = new pse_handle();
    int r = create_impl(p, h);
    if (r) { std::string keep = error_text(); pse_destroy(h); error_text() = keep; return r; }
    *out = h;
    return 0;
}

extern "C" int pse_set_box(pse_handle *h, double Lx, double Ly, double Lz, double xy) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    if (!(Lx > 0 && Ly > 0 && Lz > 0)) return fail(PSE_ERR_INVALID, "box lengths must be positive");
    if (!(std::fabs(xy) <= 0.5 * (1.0 + 1e-9)))
        return fail(PSE_ERR_INVALID, "tilt xy = %g outside [-0.5, 0.5]: HOOMD flips the box there, and the sequential minimum image "
                    "(PSEv1/Mobility.cu:648) is exact only up to that tilt", xy);
    // Nothing of the handle changes unless every check passes: the candidate cell grid is computed on the side.
    // The grid, P and eta were chosen for the creation box (the reference also fixes them in setParams and only
    // recomputes wave vectors per step, PSEv1/Stokes.cu:298); lengths may change only by re-deriving h.
    const Box nb{Lx, Ly, Lz, xy};
    const double gamma = std::max(std::fabs(xy), h->par.max_strain);
    DCells nc, nc_narrow;
    TRY(cells_for(nb, near_radius(h), gamma, h->n_slabs, h->tun.cell_bz, nc, h->loc.on ? 1 : 0));
    // prepare() switches to the narrow grid (cells of width rcut: more of them) whenever the kept list is suspended or off
    TRY(cells_for(nb, h->d.rcut, gamma, h->n_slabs, h->tun.cell_bz, nc_narrow, h->loc.on ? 1 : 0));
    if (h->loc.on && nc.nx != h->nc.nx)
        return fail(PSE_ERR_INVALID, "an owned-particle rank cannot change its cell layers along x (%d -> %d): the slabs are the ownership", h->nc.nx, nc.nx);
    if ((size_t)std::max(cells_total(nc), cells_total(nc_narrow)) > h->n_cells_alloc)
        return fail(PSE_ERR_INVALID, "box grew beyond the cell-list capacity sized at creation");
    TRY(gaussian_fits(h->d, Lx / h->d.Nx, Ly / h->d.Ny, Lz / h->d.Nz));
    h->box = nb;
    h->nc = nc;
    h->cell_gamma = gamma;
    h->nc_wide = h->skin_max > 0.0;
    // the kept neighbour list is tied to the box it was built in: prepare() compares vl_box with the box of the call
    h->d.hx = Lx / h->d.Nx; h->d.hy = Ly / h->d.Ny; h->d.hz = Lz / h->d.Nz;
    h->G.hx = h->d.hx; h->G.hy = h->d.hy; h->G.hz = h->d.hz;
    set_dbox(h);
    h->info.ncell_x = h->nc.nx; h->info.ncell_y = h->nc.ny; h->info.ncell_z = h->nc.nz;
    h->info.hx = h->d.hx; h->info.hy = h->d.hy; h->info.hz = h->d.hz;
    return 0;
}

extern "C" int pse_set_neighbor_skin(pse_handle *h, double r_buff) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    if (!(r_buff >= 0.0)) return fail(PSE_ERR_INVALID, "r_buff must be >= 0");
    if (r_buff > h->skin_max * (1 + 1e-12))
        return fail(PSE_ERR_INVALID, "r_buff = %g exceeds %g, what the cell grid and the list capacity were sized for at creation "
                    "(0 here: the neighbour list is not kept on this handle -- slab rank, cutoff too large for the box or the table)",
                    r_buff, h->skin_max);
    h->skin = r_buff;
    h->vl_valid = false;
    for (int q = 0; q < 2; ++q) { h->vl_misses[q] = 0; h->vl_suspend_left[q] = 0; h->vl_suspend_len[q] = 32; }
    return 0;
}
extern "C" int pse_neighbor_stats(pse_handle *h, double *r_buff, unsigned long long *builds, unsigned long long *reuses) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    if (r_buff) *r_buff = h->skin;
    if (builds) *builds = h->nlist_builds;
    if (reuses) *reuses = h->nlist_reuses;
    return 0;
}

extern "C" int pse_set_stream(pse_handle *h, void *stream) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    h->stream = (hipStream_t)stream;
    if (!h->side_on) {
        h->wstream = h->stream;
        TRY(bind_wave_stream(h));
    }
    return 0;
}
extern "C" int pse_set_async(pse_handle *h, int enabled) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    h->async_mode = enabled != 0;
    h->vl_valid = false;
    return 0;
}
extern "C" int pse_set_timestep_offset(pse_handle *h, const unsigned int *device_word) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    h->ts_off = device_word;
    return 0;
}
extern "C" int pse_set_timing(pse_handle *h, int enabled) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    h->timing = enabled != 0;
    return 0;
}
extern "C" int pse_get_info(pse_handle *h, pse_info *info) {
    if (!h || !info) return fail(PSE_ERR_INVALID, "null argument");
    if (h->lz_last_queued && h->lz_seq > 0 && h->sc_host && h->sc_host[LZ_HOST_SEQ] > 0.0) {   // (not after a host-checked call: its numbers are in h->info already)
        // queue-only Brownian calls: what the device-side decision of the most recent COMPLETED call left in the host mirror (the
        // caller synchronises its stream first if it wants the call it has just queued)
        h->info.lanczos_m = (int)h->sc_host[LZ_HOST_M];
        h->info.lanczos_stepnorm = h->sc_host[LZ_HOST_STEPNORM];
        h->info.lanczos_status = (int)h->sc_host[LZ_HOST_STATUS];
    }
    h->info.lanczos_open_calls = h->sc_host ? (unsigned long long)h->sc_host[LZ_HOST_OPEN] : 0ull;
    *info = h->info;
    return 0;
}

extern "C" int pse_local_layout(pse_handle *h, int *rows_own, int *rows_ghost, int *records, int *layers, int *layers_per_rank) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    if (!h->loc.on) return fail(PSE_ERR_INVALID, "not an owned-particle handle (pse_params.local_rows)");
    if (rows_own) *rows_own = h->loc.g.c_own;
    if (rows_ghost) *rows_ghost = h->loc.g.c_g;
    if (records) *records = h->loc.g.c_x;
    if (layers) *layers = h->loc.g.nx;
    if (layers_per_rank) *layers_per_rank = h->loc.g.per;
    return 0;
}

extern "C" int pse_set_lanczos_operator(pse_handle *h, int op) {
    if (!h) return fail(PSE_ERR_INVALID, "pse_set_lanczos_operator: null handle");
    if (op != PSE_LANCZOS_RECORDS16 && op != PSE_LANCZOS_FP64)
        return fail(PSE_ERR_INVALID, "pse_set_lanczos_operator: %d is neither PSE_LANCZOS_RECORDS16 (0) nor PSE_LANCZOS_FP64 (1)", op);
    return set_lanczos_op(h, op);
}
extern "C" int pse_get_lanczos_operator(pse_handle *h, int *op) {
    if (!h || !op) return fail(PSE_ERR_INVALID, "pse_get_lanczos_operator: null argument");
    *op = h->lz_op;
    return 0;
}

extern "C" int pse_set_lanczos_extra(pse_handle *h, int extra) {
    if (!h) return fail(PSE_ERR_INVALID, "null handle");
    if (extra > 32) return fail(PSE_ERR_INVALID, "at most 32 extra Lanczos iterations");
    h->lz_extra = extra < 0 ? -1 : extra;
    return 0;
}
