// Kernels of the force providers (pse_forces.h): pair repulsion, tabulated and typed pair tables with exclusions on the engine's cell
// list, bonds, angles and dihedrals on the caller-order arrays, and the type mirror (k_type_mirror) that every typed cell-list pass
// runs behind the sort.  They stand beside the path: the step consumes the forces they leave in net_force.  The analyses are in
// pse_analysis.hip and pse_order.hip.  gfx950, wave64, fp64.
#include "pse_forces.h"
#include "pse_excl.h"

#include <type_traits>

namespace pse {

// Force providers next to the path (the step consumes net_force, PSEv1/Stokes.cc:447).  What the passes below share:
constexpr int PV_NOBS = PAIR_VIRIAL_NOBS;
typedef double pt_entry __attribute__((ext_vector_type(2)));   // a 16-byte LDS word (see k_pair_table)

// The force row of one particle under `accumulate`: read before it is written, so that w is kept.
__device__ __forceinline__ void force_row_store(double4 *__restrict__ force, unsigned idx, int accumulate, double Fx, double Fy, double Fz) {
    double4 f = force[idx];
    if (accumulate) { f.x += Fx; f.y += Fy; f.z += Fz; } else { f.x = Fx; f.y = Fy; f.z = Fz; }
    force[idx] = f;
}
// The row of a particle without entries: accumulate != 0 neither reads nor writes it, accumulate == 0 overwrites its xyz, w kept.
__device__ __forceinline__ void force_row_clear(double4 *__restrict__ force, unsigned idx, int accumulate) {
    if (force && !accumulate) force_row_store(force, idx, 0, 0.0, 0.0, 0.0);
}
// One pair of a central force c d (d = r_i - r_j minimum image) with energy u: U, the six components W_ab = c d_a d_b of the
// symmetric virial sum_{i<j} r_ij (x) F_ij, and a count.
__device__ __forceinline__ void obs_add_central(double (&o)[PV_NOBS], double u, double c, double dx, double dy, double dz) {
    const double cdx = c * dx, cdy = c * dy;
    o[0] += u;
    o[1] += cdx * dx; o[2] += cdx * dy; o[3] += cdx * dz;
    o[4] += cdy * dy; o[5] += cdy * dz; o[6] += c * dz * dz;
    o[7] += 1.0;
}
// The reduction of the eight sums: over the wave with wave_sum, over the four waves through LDS with ONE barrier for the whole
// 8-vector, and the workgroup writes row `blk` of eight doubles; k_pair_virial_finish adds the rows up.  No floating-point atomics:
// every sum has a fixed order.  EVERY lane of the workgroup must arrive here (lanes past the last row with zeros).
__device__ __forceinline__ void obs_rows_store(double (&o)[PV_NOBS], int blk, double *__restrict__ rows /* [gridDim.x][PV_NOBS] */) {
    static_assert(TPB == 256, "the sum over the four waves of a workgroup is written out");
    __shared__ double sh[TPB / 64][PV_NOBS];
#pragma unroll
    for (int q = 0; q < PV_NOBS; ++q) o[q] = wave_sum(o[q]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < PV_NOBS; ++q) sh[threadIdx.x >> 6][q] = o[q];
    }
    __syncthreads();
    if (threadIdx.x < PV_NOBS) rows[(size_t)blk * PV_NOBS + threadIdx.x] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}
// Per-type parameters of the bonded passes: the type differs from lane to lane, so a wave-uniform (scalar) load cannot serve them;
// they are staged in LDS instead, 32 bytes per type, at most 2 KB, copied by the first 2 ntypes lanes of each workgroup before one
// barrier, and read as two 16-byte words per entry.  In the common case of one type every lane reads the same word, which the LDS
// broadcasts.  EVERY lane must arrive here.
__device__ __forceinline__ void stage_type_params(pt_entry *dst, const void *__restrict__ par, int ntypes, int words = 2) {
    if ((int)threadIdx.x < words * ntypes) dst[threadIdx.x] = ((const pt_entry *)par)[threadIdx.x];
    __syncthreads();
}

// Soft repulsion F_i = sum_j k (sigma - r) (r_i - r_j)/r over pairs closer than sigma, from the engine's own cell list.  One thread
// per particle; the result is added to (or stored in) the caller's force array in the caller's order.
// (the cell walk is written out here and in k_pair_table: shared through a lambda-taking helper in the style of for_each_run it
// compiled to another register allocation and cost the table pass 1 %, docs/HISTORY.md)
// OBS: the same pass with the pair observables of a rheology run: besides the force on row i from ALL its neighbours, the rows
// j > i of the sorted order -- every unordered pair once -- add U = k/2 (sigma - r)^2 and the virial of c = k (sigma - r)/r
// (obs_add_central), reduced by obs_rows_store.  The sorted order fixes every sum, and the cell sort is a stable sort (k_cell_order),
// so the eight numbers are bit-reproducible from call to call on equal inputs.  force == nullptr: observables only.
// EXCL: the pairs of `ex` contribute nothing (pse_pair_repulsion_excl).  The lane reads its tag and its row bounds once; a pair
// that has passed the distance test -- a few per particle -- is looked up by the partner's tag (excl_has), and only by a lane whose row
// is not empty: the others load neither tag_s[j] nor an entry.  The test is symmetric (every pair is in both rows), so the forces stay
// equal and opposite and the rule j > i of the sums stays; the kept pairs are summed in the order of the plain pass.  EXCL = false
// is the plain pass: `ex` is not read.
template <bool OBS, bool EXCL>
__global__ void __launch_bounds__(TPB)
k_pair_repulsion(const double4 *__restrict__ pos_s, const unsigned *__restrict__ tag_s, int N, const int *__restrict__ cell_off,
                 DBox box, DCells nc, double k, double sigma, int accumulate, double4 *__restrict__ force,
                 double *__restrict__ rows /* OBS: [gridDim.x][PV_NOBS] */, ExclRows ex) {
    const int blk = xcd_block(blockIdx.x, gridDim.x);
    const int i = blk * TPB + threadIdx.x;
    double o[PV_NOBS];
#pragma unroll
    for (int q = 0; q < PV_NOBS; ++q) o[q] = 0.0;
    if (i < N) {   // (no early return: the lanes past the last row take part in the reduction with zeros)
        const double4 pi = pos_s[i];
        double fx, fy, fz;
        frac_coords(box, pi.x, pi.y, pi.z, fx, fy, fz);
        const int cx = cell_coord(fx, nc.nx), cy = cell_coord(fy, nc.ny), cz = cell_coord(fz, nc.nz);
        const double s2 = sigma * sigma;
        double Fx = 0.0, Fy = 0.0, Fz = 0.0;
        unsigned eb = 0u, ee = 0u;
        if (EXCL) excl_row(ex, tag_s[i], eb, ee);
        for_each_run(nc, cell_off, cx, cy, cz, [&](int jb, int je, unsigned) {
            for (int j = jb; j < je; ++j) {
                const double4 pj = pos_s[j];
                double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                min_image(box, dx, dy, dz);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (r2 < s2 && j != i && r2 > 0.0 && !(EXCL && eb < ee && excl_has(ex.ent, eb, ee, tag_s[j]))) {
                    const double r = sqrt(r2), c = k * (sigma - r) / r;
                    Fx += c * dx; Fy += c * dy; Fz += c * dz;
                    if (OBS && j > i) obs_add_central(o, 0.5 * k * (sigma - r) * (sigma - r), c, dx, dy, dz);
                }
            }
        });
        if (force) force_row_store(force, tag_s[i], accumulate, Fx, Fy, Fz);
    }
    if (OBS) obs_rows_store(o, blk, rows);
}
// One workgroup adds the nrows workgroup rows in a fixed order (the reduce_partials pattern, for the 8-vector at once): thread t
// owns component t % 8 of the rows t / 8, t / 8 + 32, ...; then the 32 partial sums of a component are added in index order.
__global__ void __launch_bounds__(TPB)
k_pair_virial_finish(const double *__restrict__ rows, int nrows, double *__restrict__ out8) {
    __shared__ double sh[TPB];
    const int q = threadIdx.x % PV_NOBS;
    double v = 0.0;
    for (int r = threadIdx.x / PV_NOBS; r < nrows; r += TPB / PV_NOBS) v += rows[(size_t)r * PV_NOBS + q];
    sh[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x < PV_NOBS) {
        double s = 0.0;
        for (int t = threadIdx.x; t < TPB; t += PV_NOBS) s += sh[t];
        out8[threadIdx.x] = s;
    }
}
// The launch pair of every provider: out8 != null: launch(true, rows), then the rows are added up into out8; out8 == null:
// launch(false, nullptr), no reduction.  `launch` takes the OBS flag as a std::bool_constant.
template <class L>
static void launch_with_obs(int nb, double *rows, double *out8, hipStream_t s, L &&launch) {
    if (out8) {
        launch(std::true_type{}, rows);
        hipLaunchKernelGGL(k_pair_virial_finish, dim3(1), dim3(TPB), 0, s, rows, nb, out8);
    } else {
        launch(std::false_type{}, (double *)nullptr);
    }
}
void launch_pair_repulsion(const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc,
                           double k, double sigma, int accumulate, double4 *force, double *rows, double *out8, hipStream_t s,
                           const PairExclusions *ex) {
    const int nb = nblocks(N, TPB);
    launch_with_excl(ex, [&](auto excl, ExclRows er) {
        launch_with_obs(nb, rows, out8, s, [&](auto obs, double *r) {
            hipLaunchKernelGGL((k_pair_repulsion<decltype(obs)::value, decltype(excl)::value>), dim3(nb), dim3(TPB), 0, s, pos_s, tag_s, N,
                               cell_off, box, nc, k, sigma, accumulate, force, r, er);
        });
    });
}
size_t pair_virial_rows(int n) { return (size_t)nblocks(n, TPB) * PV_NOBS; }

// Tabulated central pair potential on the same cell list (the counterpart of HOOMD's pair.table for the engine's one particle type;
// no reference counterpart: the reference leaves forces to HOOMD).  table[e] = (V, F) at r_e = rmin + e dr, F the magnitude of the
// radial force, positive for a repulsion; between the nodes both are interpolated linearly: t = (r - rmin) scale with
// scale = (width - 1)/(rmax - rmin), e = min(floor(t), width - 2), w = t - e.  A pair with rmin <= r, r^2 < rmax^2, r > 0 adds
// F(r) d / r to row i; the rest contributes nothing.
// LDS: every workgroup first copies the table, one 16-byte (V, F) entry per lane and trip (global_load_dwordx4 -> ds_write_b128,
// coalesced), into `width` 16-byte entries -- 32 KB at the cap of PAIR_TABLE_MAX_WIDTH -- and a pair then makes two ds_read_b128, entries
// e and e + 1: V and F of a node share one read, the LDS serves 16-byte reads at its full rate and an entry never straddles two
// bank rows.  The lanes' e are unrelated, so these reads conflict; that is accepted, the pass is bound by the position gathers.
// OBS: the eight sums of k_pair_repulsion<true> with U = V(r) and c = F(r)/r, over the rows j > i, reduced and written to `rows`
// exactly as there.  No lane leaves before the barrier behind the staging loop, nor, with OBS, before the one of the reduction.
// (pt_entry is the native vector type, not double2: hipcc splits a double2 read from LDS into its members and pairs them up again as
// ds_read2_b64, which the LDS serves at a quarter of the rate of ds_read_b128; x = V, y = F)
// EXCL: the pairs of `ex` contribute nothing (pse_pair_table_excl), exactly as in k_pair_repulsion<OBS, true>: tag and row bounds
// once per lane, the lookup (excl_has) behind both distance tests and only in a lane with a row; EXCL = false does not read `ex`.
template <bool OBS, bool EXCL>
__global__ void __launch_bounds__(TPB)
k_pair_table(const double4 *__restrict__ pos_s, const unsigned *__restrict__ tag_s, int N, const int *__restrict__ cell_off, DBox box,
             DCells nc, const double2 *__restrict__ table, int width, double rmin, double rmax, double scale, int accumulate,
             double4 *__restrict__ force, double *__restrict__ rows /* OBS: [gridDim.x][PV_NOBS] */, ExclRows ex) {
    extern __shared__ pt_entry pt_tab[];   // [width]
    for (int e = threadIdx.x; e < width; e += TPB) pt_tab[e] = ((const pt_entry *)table)[e];
    __syncthreads();
    const int blk = xcd_block(blockIdx.x, gridDim.x);
    const int i = blk * TPB + threadIdx.x;
    double o[PV_NOBS];
#pragma unroll
    for (int q = 0; q < PV_NOBS; ++q) o[q] = 0.0;
    if (i < N) {
        const double4 pi = pos_s[i];
        double fx, fy, fz;
        frac_coords(box, pi.x, pi.y, pi.z, fx, fy, fz);
        const int cx = cell_coord(fx, nc.nx), cy = cell_coord(fy, nc.ny), cz = cell_coord(fz, nc.nz);
        const double rmax2 = rmax * rmax;
        const int elast = width - 2;
        double Fx = 0.0, Fy = 0.0, Fz = 0.0;
        unsigned eb = 0u, ee = 0u;
        if (EXCL) excl_row(ex, tag_s[i], eb, ee);
        for_each_run(nc, cell_off, cx, cy, cz, [&](int jb, int je, unsigned) {
            for (int j = jb; j < je; ++j) {
                const double4 pj = pos_s[j];
                double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                min_image(box, dx, dy, dz);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (r2 < rmax2 && j != i && r2 > 0.0) {
                    const double r = sqrt(r2);
                    if (r >= rmin && !(EXCL && eb < ee && excl_has(ex.ent, eb, ee, tag_s[j]))) {
                        const double t = (r - rmin) * scale;        // 0 <= t <= width - 1 (+ an ulp): e stays inside the table
                        const int e = min((int)t, elast);
                        const double w = t - (double)e;
                        const pt_entry a = pt_tab[e], b = pt_tab[e + 1];
                        const double c = (a.y + w * (b.y - a.y)) * (1.0 / r);
                        Fx += c * dx; Fy += c * dy; Fz += c * dz;
                        if (OBS && j > i) obs_add_central(o, a.x + w * (b.x - a.x), c, dx, dy, dz);
                    }
                }
            }
        });
        if (force) force_row_store(force, tag_s[i], accumulate, Fx, Fy, Fz);
    }
    if (OBS) obs_rows_store(o, blk, rows);
}
void launch_pair_table(const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc, const double *table,
                       int width, double rmin, double rmax, int accumulate, double4 *force, double *rows, double *out8, hipStream_t s,
                       const PairExclusions *ex) {
    const int nb = nblocks(N, TPB);
    const size_t lds = (size_t)width * sizeof(double2);
    const double scale = (double)(width - 1) / (rmax - rmin);
    launch_with_excl(ex, [&](auto excl, ExclRows er) {
        launch_with_obs(nb, rows, out8, s, [&](auto obs, double *r) {
            hipLaunchKernelGGL((k_pair_table<decltype(obs)::value, decltype(excl)::value>), dim3(nb), dim3(TPB), lds, s, pos_s, tag_s, N,
                               cell_off, box, nc, (const double2 *)table, width, rmin, rmax, scale, accumulate, force, r, er);
        });
    });
}

// Typed pair tables (pse_pair_table_typed; HOOMD's pair.table with one pair_coeff per pair of types): k_pair_table with, for every
// pair, the table and the range of its pair type p(a, b) = a ntypes - a (a - 1)/2 + (b - a), a <= b.  A kernel of its own and not a
// third flag of k_pair_table: the plain pass keeps its instruction stream (see the note on shared code above k_pair_repulsion).
// LDS: the tables of all pair types lie one after another in `total` <= PAIR_TYPED_MAX_ENTRIES 16-byte entries of dynamic LDS (56 KB at
// the cap), staged as in k_pair_table; the pair type differs from lane to lane, so its parameters cannot come from a scalar load and
// are staged too (stage_type_params): two 16-byte words per pair type, (rmin, rmax^2) and (scale, {base, width - 2} as two ints in the
// bits of one double), at most 36 pair types = 1152 bytes of static LDS.  With the 256 bytes of obs_rows_store that is 1408 bytes of
// static LDS: 57344 + 1408 = 58752 <= 65536.  In the common case of few types most lanes read the same parameter word, which the LDS
// broadcasts.  An off pair type has rmax^2 = 0 and fails the range test.
// Where the types come from: a one-byte-per-row mirror in sorted order, type_s[i] = types[tag_s[i]] (0 for a tag >= n), filled by
// k_type_mirror behind the sort on every call.  A pair in range then costs one byte load at type_s[j], issued next to pos_s[j] and
// on a line that the neighbouring rows of the run share (64 rows per 64 bytes), where types[tag_s[j]] would be two dependent loads,
// the second a scattered one -- the chain that makes the exclusion lookup cost what it does.  The mirror pass reads 4 + 1 bytes and
// writes one per row, against the 32-byte position gathers of some tens of partners per row here.  Nobody has measured the other form.
// Per pair: the wave-uniform prefilter r^2 < max_p rmax^2, j != i, r^2 > 0 first; only behind it the partner's type and the
// parameter words; then the pair type's own rmax^2 and rmin and, with EXCL, the lookup of k_pair_table<OBS, true> (the tag is read
// only by lanes that have a row).  From t on the arithmetic is k_pair_table's line for line.  No lane leaves before a barrier.
__global__ void __launch_bounds__(TPB)
k_type_mirror(const unsigned *__restrict__ tag_s, int N, const unsigned char *__restrict__ types, unsigned n, unsigned char *__restrict__ type_s) {
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < N) {
        const unsigned t = tag_s[i];
        type_s[i] = t < n ? types[t] : (unsigned char)0;   // never past n
    }
}
void launch_type_mirror(const unsigned *tag_s, int N, const unsigned char *types, unsigned n, unsigned char *type_s, hipStream_t s) {
    hipLaunchKernelGGL(k_type_mirror, dim3(nblocks(N, TPB)), dim3(TPB), 0, s, tag_s, N, types, n, type_s);
}
template <bool OBS, bool EXCL>
__global__ void __launch_bounds__(TPB)
k_pair_table_typed(const double4 *__restrict__ pos_s, const unsigned *__restrict__ tag_s, const unsigned char *__restrict__ type_s, int N,
                   const int *__restrict__ cell_off, DBox box, DCells nc, const double2 *__restrict__ tables, int total,
                   const double2 *__restrict__ par /* 2 npt words */, int ntypes, double rmax2_all, int accumulate,
                   double4 *__restrict__ force, double *__restrict__ rows /* OBS: [gridDim.x][PV_NOBS] */, ExclRows ex) {
    extern __shared__ pt_entry pt_tab[];   // [total]
    __shared__ pt_entry tp[2 * PAIR_TYPED_MAX_PAIR_TYPES];   // [pair type][0] = (rmin, rmax2), [1] = (scale, {base, width - 2})
    for (int e = threadIdx.x; e < total; e += TPB) pt_tab[e] = ((const pt_entry *)tables)[e];
    stage_type_params(tp, par, ntypes * (ntypes + 1) / 2);   // (its barrier is the one behind both stages)
    const int blk = xcd_block(blockIdx.x, gridDim.x);
    const int i = blk * TPB + threadIdx.x;
    double o[PV_NOBS];
#pragma unroll
    for (int q = 0; q < PV_NOBS; ++q) o[q] = 0.0;
    if (i < N) {
        const double4 pi = pos_s[i];
        double fx, fy, fz;
        frac_coords(box, pi.x, pi.y, pi.z, fx, fy, fz);
        const int cx = cell_coord(fx, nc.nx), cy = cell_coord(fy, nc.ny), cz = cell_coord(fz, nc.nz);
        const int ti = type_s[i];
        double Fx = 0.0, Fy = 0.0, Fz = 0.0;
        unsigned eb = 0u, ee = 0u;
        if (EXCL) excl_row(ex, tag_s[i], eb, ee);
        for_each_run(nc, cell_off, cx, cy, cz, [&](int jb, int je, unsigned) {
            for (int j = jb; j < je; ++j) {
                const double4 pj = pos_s[j];
                double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                min_image(box, dx, dy, dz);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (r2 < rmax2_all && j != i && r2 > 0.0) {
                    const int tj = type_s[j];
                    const int lo = min(ti, tj), hi = max(ti, tj);
                    const int p = lo * ntypes - ((lo * (lo - 1)) >> 1) + (hi - lo);
                    const pt_entry q0 = tp[2 * p];
                    if (r2 < q0.y) {
                        const double r = sqrt(r2), rmin = q0.x;
                        if (r >= rmin && !(EXCL && eb < ee && excl_has(ex.ent, eb, ee, tag_s[j]))) {
                            const pt_entry q1 = tp[2 * p + 1];
                            const double scale = q1.x;
                            const long long bw = __double_as_longlong(q1.y);
                            const int base = (int)(unsigned)bw, elast = (int)(bw >> 32);
                            const double t = (r - rmin) * scale;        // 0 <= t <= width - 1 (+ an ulp): e stays inside the table
                            const int e = min((int)t, elast);
                            const double w = t - (double)e;
                            const pt_entry a = pt_tab[base + e], b = pt_tab[base + e + 1];
                            const double c = (a.y + w * (b.y - a.y)) * (1.0 / r);
                            Fx += c * dx; Fy += c * dy; Fz += c * dz;
                            if (OBS && j > i) obs_add_central(o, a.x + w * (b.x - a.x), c, dx, dy, dz);
                        }
                    }
                }
            }
        });
        if (force) force_row_store(force, tag_s[i], accumulate, Fx, Fy, Fz);
    }
    if (OBS) obs_rows_store(o, blk, rows);
}
void launch_pair_table_typed(const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc,
                             const PairTypedTables &tt, int accumulate, double4 *force, double *rows, double *out8, hipStream_t s,
                             const PairExclusions *ex) {
    static_assert(2 * PAIR_TYPED_MAX_PAIR_TYPES <= TPB, "one lane stages one 16-byte word of the parameters");
    static_assert((size_t)PAIR_TYPED_MAX_ENTRIES * sizeof(pt_entry) + 2 * PAIR_TYPED_MAX_PAIR_TYPES * sizeof(pt_entry)
                  + (TPB / 64) * PV_NOBS * sizeof(double) <= 65536, "tables, parameters and the reduction share 64 KB of LDS");
    const int nb = nblocks(N, TPB);
    const size_t lds = (size_t)tt.total * sizeof(pt_entry);
    hipLaunchKernelGGL(k_type_mirror, dim3(nb), dim3(TPB), 0, s, tag_s, N, tt.types, tt.n, tt.type_s);
    launch_with_excl(ex, [&](auto excl, ExclRows er) {
        launch_with_obs(nb, rows, out8, s, [&](auto obs, double *r) {
            hipLaunchKernelGGL((k_pair_table_typed<decltype(obs)::value, decltype(excl)::value>), dim3(nb), dim3(TPB), lds, s, pos_s, tag_s,
                               tt.type_s, N, cell_off, box, nc, (const double2 *)tt.tables, tt.total, (const double2 *)tt.par, tt.ntypes,
                               tt.rmax2_all, accumulate, force, r, er);
        });
    });
}

// Bonded forces (HOOMD's bond.harmonic and bond.fene; no reference counterpart: the reference leaves forces to HOOMD).  One thread
// per particle of the CALLER-order arrays walks its row of the bond object -- entries (partner, type), one 8-byte load each, sorted by
// (partner, type) on the host -- and gathers each partner's position with one double4 load.  With d = r_i - r_j (minimum image),
// the force on i from j is c d, c = -k (r - r0)/r (harmonic) or -k / (1 - (r/r0)^2) (FENE, r < r0).  Every bond is in both
// endpoints' rows, so each thread owns its force row: no atomics on forces, and the order of the sum is the order of the row, a function
// of the bond SET -- forces and sums are bit-identical for any permutation of the bond list and either order of a bond's endpoints
// (min_image is odd in d, so both ends see the same r).  A bond with r == 0 does nothing; a FENE bond with r >= r0 does nothing either
// and is counted: its lower endpoint adds it to a per-thread count, and a thread that saw one makes ONE integer atomicAdd.
// Per-type parameters (stage_type_params): (k, r0, 1/r0^2, kind).
// OBS: the endpoint with the LOWER index adds the bond to the eight sums U, W (six), count (obs_add_central, obs_rows_store).  No lane
// leaves before either barrier.
// accumulate != 0: the rows of unbonded particles are neither read nor written; accumulate == 0: every row's xyz is overwritten, w kept.
template <bool OBS>
__global__ void __launch_bounds__(TPB)
k_bond_forces(const double4 *__restrict__ pos, int n, const unsigned *__restrict__ row_off, const uint2 *__restrict__ entries,
              const BondParam *__restrict__ par, int ntypes, DBox box, int accumulate, double4 *__restrict__ force,
              double *__restrict__ rows /* OBS: [gridDim.x][PV_NOBS] */, unsigned long long *__restrict__ overstretched) {
    __shared__ pt_entry bp[2 * BOND_MAX_TYPES];   // [type][0] = (k, r0), [type][1] = (1/r0^2, kind)
    stage_type_params(bp, par, ntypes);
    const int blk = xcd_block(blockIdx.x, gridDim.x);
    const int i = blk * TPB + threadIdx.x;
    double o[PV_NOBS];
#pragma unroll
    for (int q = 0; q < PV_NOBS; ++q) o[q] = 0.0;
    if (i < n) {
        const unsigned eb = row_off[i], ee = row_off[i + 1];
        if (ee > eb) {
            const double4 pi = pos[i];
            double Fx = 0.0, Fy = 0.0, Fz = 0.0;
            unsigned over = 0;
            for (unsigned e = eb; e < ee; ++e) {
                const uint2 en = entries[e];                  // x = partner, y = type
                const double4 pj = pos[en.x];
                const pt_entry a = bp[2 * en.y], b = bp[2 * en.y + 1];
                double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                min_image(box, dx, dy, dz);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (r2 > 0.0) {
                    const bool lower = (unsigned)i < en.x;
                    double c, u;
                    bool acts = true;
                    if (b.y == 0.0) {                          // harmonic
                        const double r = sqrt(r2), dr = r - a.y;
                        c = -a.x * dr / r;
                        u = 0.5 * a.x * dr * dr;
                    } else {                                   // FENE
                        const double x = r2 * b.x;             // (r / r0)^2
                        acts = x < 1.0;
                        c = -a.x / (1.0 - x);
                        u = OBS ? -0.5 * a.x * a.y * a.y * log1p(-x) : 0.0;
                        if (!acts && lower) ++over;
                    }
                    if (acts) {
                        Fx += c * dx; Fy += c * dy; Fz += c * dz;
                        if (OBS && lower) obs_add_central(o, u, c, dx, dy, dz);
                    }
                }
            }
            if (force) force_row_store(force, i, accumulate, Fx, Fy, Fz);
            if (over) atomicAdd(overstretched, (unsigned long long)over);
        } else {
            force_row_clear(force, i, accumulate);
        }
    }
    if (OBS) obs_rows_store(o, blk, rows);
}
void launch_bond_forces(const double4 *pos, int n, const unsigned *row_off, const uint2 *entries, const BondParam *par, int ntypes, DBox box,
                        int accumulate, double4 *force, double *rows, double *out8, unsigned long long *overstretched, hipStream_t s) {
    static_assert(sizeof(BondParam) == 2 * sizeof(pt_entry) && 2 * BOND_MAX_TYPES <= TPB, "one lane stages one 16-byte word of the parameters");
    const int nb = nblocks(n, TPB);
    launch_with_obs(nb, rows, out8, s, [&](auto obs, double *r) {
        hipLaunchKernelGGL(k_bond_forces<decltype(obs)::value>, dim3(nb), dim3(TPB), 0, s, pos, n, row_off, entries, par, ntypes, box,
                           accumulate, force, r, overstretched);
    });
}

// Angle forces (HOOMD's angle.harmonic and angle.cosinesq; no reference counterpart: the reference leaves forces to HOOMD).  One
// thread per particle of the CALLER-order arrays walks its row of the angle object -- entries (i, j, k, type), j the vertex, i < k,
// one 16-byte load each, sorted by (i, j, k, type) on the host.  The thread loads all three positions from memory, its own included,
// and evaluates d1 = r_i - r_j, d2 = r_k - r_j (minimum image), c = d1.d2 / (r1 r2) in [-1, 1], g = -dV/dc and
//   F_i = g (d2/(r1 r2) - c d1/r1^2),  F_k = g (d1/(r1 r2) - c d2/r2^2),  F_j = -(F_i + F_k)
// in this CANONICAL order whatever its own role is, then takes the force of its role: the three threads of an angle run the same
// arithmetic on the same numbers and hold bit-identical F_i and F_k.  Each thread owns its force row: no atomics on forces, and the
// order of the sum is the order of the row, a function of the angle SET -- forces and sums are bit-identical for any permutation of
// the list and either order of an angle's ends.  harmonic: g = k (theta - theta0)/s with s = max(sqrt(1 - c^2), 1e-3) (HOOMD's floor
// for the straight angle), the only branch that takes an acos; cosine-squared: g = -k (c - cos theta0).  An angle with r1 == 0 or
// r2 == 0 does nothing.
// Per-type parameters (stage_type_params): (k, theta0, cos theta0, kind).
// OBS: the VERTEX thread alone adds the angle to the eight sums U, W_ab = d1_a F_i,b + d2_a F_k,b (six), count (obs_rows_store).  No
// lane leaves before either barrier.
// accumulate != 0: the rows of particles in no angle are neither read nor written; accumulate == 0: every row's xyz is overwritten, w kept.
template <bool OBS>
__global__ void __launch_bounds__(TPB)
k_angle_forces(const double4 *__restrict__ pos, int n, const int *__restrict__ row_off, const uint4 *__restrict__ entries,
               const AngleParam *__restrict__ par, int ntypes, DBox box, int accumulate, double4 *__restrict__ force,
               double *__restrict__ rows /* OBS: [gridDim.x][PV_NOBS] */) {
    __shared__ pt_entry ap[2 * ANGLE_MAX_TYPES];   // [type][0] = (k, theta0), [type][1] = (cos theta0, kind)
    stage_type_params(ap, par, ntypes);
    const int blk = xcd_block(blockIdx.x, gridDim.x);
    const int p = blk * TPB + threadIdx.x;
    double o[PV_NOBS];
#pragma unroll
    for (int q = 0; q < PV_NOBS; ++q) o[q] = 0.0;
    if (p < n) {
        const int eb = row_off[p], ee = row_off[p + 1];
        if (ee > eb) {
            double Fx = 0.0, Fy = 0.0, Fz = 0.0;
            for (int e = eb; e < ee; ++e) {
                const uint4 en = entries[e];                  // x = i, y = j (vertex), z = k, w = type
                const double4 pi = pos[en.x], pj = pos[en.y], pk = pos[en.z];
                const pt_entry a = ap[2 * en.w], b = ap[2 * en.w + 1];
                double d1x = pi.x - pj.x, d1y = pi.y - pj.y, d1z = pi.z - pj.z;
                double d2x = pk.x - pj.x, d2y = pk.y - pj.y, d2z = pk.z - pj.z;
                min_image(box, d1x, d1y, d1z);
                min_image(box, d2x, d2y, d2z);
                const double r1sq = d1x * d1x + d1y * d1y + d1z * d1z, r2sq = d2x * d2x + d2y * d2y + d2z * d2z;
                if (r1sq > 0.0 && r2sq > 0.0) {
                    const double ir12 = 1.0 / (sqrt(r1sq) * sqrt(r2sq));
                    double c = (d1x * d2x + d1y * d2y + d1z * d2z) * ir12;
                    c = fmin(1.0, fmax(-1.0, c));
                    double g, u;
                    if (b.y == 0.0) {                          // harmonic
                        const double dth = acos(c) - a.y;
                        g = a.x * dth / fmax(sqrt(1.0 - c * c), 1e-3);
                        u = 0.5 * a.x * dth * dth;
                    } else {                                   // cosine-squared
                        const double dc = c - b.x;
                        g = -a.x * dc;
                        u = 0.5 * a.x * dc * dc;
                    }
                    const double g12 = g * ir12, g11 = g * c / r1sq, g22 = g * c / r2sq;
                    const double Fix = g12 * d2x - g11 * d1x, Fiy = g12 * d2y - g11 * d1y, Fiz = g12 * d2z - g11 * d1z;
                    const double Fkx = g12 * d1x - g22 * d2x, Fky = g12 * d1y - g22 * d2y, Fkz = g12 * d1z - g22 * d2z;
                    if ((unsigned)p == en.y) {                 // the vertex
                        Fx -= Fix + Fkx; Fy -= Fiy + Fky; Fz -= Fiz + Fkz;
                        if (OBS) {
                            o[0] += u;
                            o[1] += d1x * Fix + d2x * Fkx; o[2] += d1x * Fiy + d2x * Fky; o[3] += d1x * Fiz + d2x * Fkz;
                            o[4] += d1y * Fiy + d2y * Fky; o[5] += d1y * Fiz + d2y * Fkz; o[6] += d1z * Fiz + d2z * Fkz;
                            o[7] += 1.0;
                        }
                    } else {
                        const bool first = (unsigned)p == en.x;
                        Fx += first ? Fix : Fkx; Fy += first ? Fiy : Fky; Fz += first ? Fiz : Fkz;
                    }
                }
            }
            if (force) force_row_store(force, p, accumulate, Fx, Fy, Fz);
        } else {
            force_row_clear(force, p, accumulate);
        }
    }
    if (OBS) obs_rows_store(o, blk, rows);
}
void launch_angle_forces(const double4 *pos, int n, const int *row_off, const uint4 *entries, const AngleParam *par, int ntypes, DBox box,
                         int accumulate, double4 *force, double *rows, double *out8, hipStream_t s) {
    static_assert(sizeof(AngleParam) == 2 * sizeof(pt_entry) && 2 * ANGLE_MAX_TYPES <= TPB, "one lane stages one 16-byte word of the parameters");
    const int nb = nblocks(n, TPB);
    launch_with_obs(nb, rows, out8, s, [&](auto obs, double *r) {
        hipLaunchKernelGGL(k_angle_forces<decltype(obs)::value>, dim3(nb), dim3(TPB), 0, s, pos, n, row_off, entries, par, ntypes, box,
                           accumulate, force, r);
    });
}

// Dihedral forces (HOOMD's dihedral.harmonic and dihedral.opls; no reference counterpart: the reference leaves forces to HOOMD).
// One thread per particle of the CALLER-order arrays walks its row of the dihedral object -- entries (i, j, k, l), i < l, one 16-byte
// load each, and the entry's type from the parallel array, sorted by (i, j, k, l, type) on the host.  The thread loads all four
// positions from memory, its own included, and evaluates, by minimum image,
//   d1 = r_i - r_j, d2 = r_k - r_j, d3 = r_k - r_l,  m = d1 x d2, nn = d2 x d3, b = |d2|,
//   cos phi = m.nn / (|m| |nn|),  sin phi = b d1.nn / (|m| |nn|)   (phi = atan2(b d1.nn, m.nn): cis 0, trans pi; no atan2 is taken),
//   g = dV/dphi,  F_i = -g b/|m|^2 m,  F_l = g b/|nn|^2 nn,  s = d1.d2/b^2, t = d3.d2/b^2,
//   F_j = -F_i + s F_i - t F_l,  F_k = -F_l - s F_i + t F_l
// in this CANONICAL order whatever its own role is, then takes the force of its role: the four threads of a dihedral run the same
// arithmetic on the same numbers and hold bit-identical forces.  Each thread owns its force row: no atomics on forces, and the order
// of the sum is the order of the row, a function of the dihedral SET -- forces and sums are bit-identical for any permutation of the
// list and either direction of a quadruple.  cos and sin of the multiples of phi come from the angle-addition recurrence:
// harmonic: (cm, sm) of mult phi by mult - 1 rotations, V = kh (1 + cd cm + sd sm), g = kh mult (sd cm - cd sm) with kh = k/2,
// (cd, sd) = d (cos phi0, sin phi0); OPLS: the double-angle forms for 2 phi, 4 phi and one rotation for 3 phi.
// A dihedral with |m|^2 == 0 or |nn|^2 == 0 does nothing.
// Per-type parameters (stage_type_params, three words): harmonic (kh, cd), (sd, unused), (mult, 0); OPLS (k1, k2), (k3, k4), (0, 0):
// mult == 0 is the OPLS kind.
// OBS: the thread of j alone adds the dihedral to the eight sums U, W_ab = d1_a F_i,b + d2_a F_k,b + (d2 - d3)_a F_l,b (six), count
// (obs_rows_store).  No lane leaves before either barrier.
// accumulate != 0: the rows of particles in no dihedral are neither read nor written; accumulate == 0: every row's xyz is overwritten, w kept.
template <bool OBS>
__global__ void __launch_bounds__(TPB)
k_dihedral_forces(const double4 *__restrict__ pos, int n, const int *__restrict__ row_off, const uint4 *__restrict__ entries,
                  const unsigned *__restrict__ types, const DihedralParam *__restrict__ par, int ntypes, DBox box, int accumulate,
                  double4 *__restrict__ force, double *__restrict__ rows /* OBS: [gridDim.x][PV_NOBS] */) {
    __shared__ pt_entry dp[3 * DIHEDRAL_MAX_TYPES];
    stage_type_params(dp, par, ntypes, 3);
    const int blk = xcd_block(blockIdx.x, gridDim.x);
    const int p = blk * TPB + threadIdx.x;
    double o[PV_NOBS];
#pragma unroll
    for (int q = 0; q < PV_NOBS; ++q) o[q] = 0.0;
    if (p < n) {
        const int eb = row_off[p], ee = row_off[p + 1];
        if (ee > eb) {
            double Fx = 0.0, Fy = 0.0, Fz = 0.0;
            for (int e = eb; e < ee; ++e) {
                const uint4 en = entries[e];                  // x = i, y = j, z = k, w = l
                const unsigned ty = types[e];
                const double4 pi = pos[en.x], pj = pos[en.y], pk = pos[en.z], pl = pos[en.w];
                double d1x = pi.x - pj.x, d1y = pi.y - pj.y, d1z = pi.z - pj.z;
                double d2x = pk.x - pj.x, d2y = pk.y - pj.y, d2z = pk.z - pj.z;
                double d3x = pk.x - pl.x, d3y = pk.y - pl.y, d3z = pk.z - pl.z;
                min_image(box, d1x, d1y, d1z);
                min_image(box, d2x, d2y, d2z);
                min_image(box, d3x, d3y, d3z);
                const double mx = d1y * d2z - d1z * d2y, my = d1z * d2x - d1x * d2z, mz = d1x * d2y - d1y * d2x;
                const double nx = d2y * d3z - d2z * d3y, ny = d2z * d3x - d2x * d3z, nz = d2x * d3y - d2y * d3x;
                const double m2 = mx * mx + my * my + mz * mz, n2 = nx * nx + ny * ny + nz * nz;
                if (m2 > 0.0 && n2 > 0.0) {
                    const double b2 = d2x * d2x + d2y * d2y + d2z * d2z, b = sqrt(b2);
                    const double inv = 1.0 / sqrt(m2 * n2);
                    const double c = (mx * nx + my * ny + mz * nz) * inv;
                    const double sn = b * (d1x * nx + d1y * ny + d1z * nz) * inv;
                    const pt_entry a0 = dp[3 * ty], a1 = dp[3 * ty + 1], a2 = dp[3 * ty + 2];
                    double g, u;
                    if (a2.x != 0.0) {                         // harmonic: a0 = (kh, cd), a1.x = sd, a2.x = mult
                        double cm = c, sm = sn;
                        const int mult = (int)a2.x;
                        for (int q = 1; q < mult; ++q) {
                            const double t = cm * c - sm * sn;
                            sm = sm * c + cm * sn;
                            cm = t;
                        }
                        u = a0.x * (1.0 + a0.y * cm + a1.x * sm);
                        g = a0.x * a2.x * (a1.x * cm - a0.y * sm);
                    } else {                                   // OPLS: a0 = (k1, k2), a1 = (k3, k4)
                        const double c2 = 2.0 * c * c - 1.0, s2 = 2.0 * sn * c;
                        const double c3 = c2 * c - s2 * sn, s3 = s2 * c + c2 * sn;
                        const double c4 = 2.0 * c2 * c2 - 1.0, s4 = 2.0 * s2 * c2;
                        u = 0.5 * (a0.x * (1.0 + c) + a0.y * (1.0 - c2) + a1.x * (1.0 + c3) + a1.y * (1.0 - c4));
                        g = 0.5 * (-a0.x * sn + 2.0 * a0.y * s2 - 3.0 * a1.x * s3 + 4.0 * a1.y * s4);
                    }
                    const double gi = -g * b / m2, gl = g * b / n2;
                    const double Fix = gi * mx, Fiy = gi * my, Fiz = gi * mz;
                    const double Flx = gl * nx, Fly = gl * ny, Flz = gl * nz;
                    const double ib2 = 1.0 / b2;
                    const double s = (d1x * d2x + d1y * d2y + d1z * d2z) * ib2, t = (d3x * d2x + d3y * d2y + d3z * d2z) * ib2;
                    const double Sx = s * Fix - t * Flx, Sy = s * Fiy - t * Fly, Sz = s * Fiz - t * Flz;   // F_j = S - F_i, F_k = -S - F_l
                    if ((unsigned)p == en.y) {                 // j
                        Fx += Sx - Fix; Fy += Sy - Fiy; Fz += Sz - Fiz;
                        if (OBS) {
                            const double Fkx = -Sx - Flx, Fky = -Sy - Fly, Fkz = -Sz - Flz;
                            const double ex = d2x - d3x, ey = d2y - d3y, ez = d2z - d3z;   // r_l - r_j
                            o[0] += u;
                            o[1] += d1x * Fix + d2x * Fkx + ex * Flx; o[2] += d1x * Fiy + d2x * Fky + ex * Fly;
                            o[3] += d1x * Fiz + d2x * Fkz + ex * Flz; o[4] += d1y * Fiy + d2y * Fky + ey * Fly;
                            o[5] += d1y * Fiz + d2y * Fkz + ey * Flz; o[6] += d1z * Fiz + d2z * Fkz + ez * Flz;
                            o[7] += 1.0;
                        }
                    } else if ((unsigned)p == en.z) {          // k
                        Fx -= Sx + Flx; Fy -= Sy + Fly; Fz -= Sz + Flz;
                    } else {
                        const bool first = (unsigned)p == en.x;
                        Fx += first ? Fix : Flx; Fy += first ? Fiy : Fly; Fz += first ? Fiz : Flz;
                    }
                }
            }
            if (force) force_row_store(force, p, accumulate, Fx, Fy, Fz);
        } else {
            force_row_clear(force, p, accumulate);
        }
    }
    if (OBS) obs_rows_store(o, blk, rows);
}
void launch_dihedral_forces(const double4 *pos, int n, const int *row_off, const uint4 *entries, const unsigned *types,
                            const DihedralParam *par, int ntypes, DBox box, int accumulate, double4 *force, double *rows, double *out8,
                            hipStream_t s) {
    static_assert(sizeof(DihedralParam) == 3 * sizeof(pt_entry) && 3 * DIHEDRAL_MAX_TYPES <= TPB, "one lane stages one 16-byte word of the parameters");
    const int nb = nblocks(n, TPB);
    launch_with_obs(nb, rows, out8, s, [&](auto obs, double *r) {
        hipLaunchKernelGGL(k_dihedral_forces<decltype(obs)::value>, dim3(nb), dim3(TPB), 0, s, pos, n, row_off, entries, types, par, ntypes,
                           box, accumulate, force, r);
    });
}

}  // namespace pse
