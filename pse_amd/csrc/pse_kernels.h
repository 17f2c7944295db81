// Launch wrappers of the cell sort, the gates, the gather into cell order, the near field and k_eval_fg (defined in pse_kernels.hip).  All take the stream explicitly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pse_device.h"

namespace pse {

// ---- particle binning ------------------------------------------------------------------------------------
// counting sort by cell, equal to a stable sort by key: perm[slot] = input index, cell_off[c] = first slot of cell c.
// keys, rank, slots: N unsigned each; cnt: ncell + 1 ints; tmp: cell_sort_temp_bytes(ncell)
size_t cell_sort_temp_bytes(size_t ncell);
// A slab rank of a team works on its own cell layers and the neighbouring ghost layer on either side only: up to three ranges
// [c0, c1) of storage cells (x is the slowest cell index, so a range of layers is a range of cells and -- through cell_off -- a
// range of rows).  n = 0: everything (single GPU).  EVERY particle is still counted (the row offsets are global); the ordering
// inside the cells, the gather into cell order, the far-field records and the random vector are done for these rows alone.
struct CellRanges {
    int n, c0[3], c1[3];
    __device__ __forceinline__ bool cell(int c) const {
        if (n == 0) return true;
        for (int q = 0; q < n; ++q) if (c >= c0[q] && c < c1[q]) return true;
        return false;
    }
    __device__ __forceinline__ bool row(int s, const int *__restrict__ cell_off) const {
        if (n == 0) return true;
        for (int q = 0; q < n; ++q) if (s >= cell_off[c0[q]] && s < cell_off[c1[q]]) return true;
        return false;
    }
};
// Rows a near-field pass works on: up to three ranges [lo, hi) of sorted rows (a slab rank's own rows FIRST, then the ghost cell
// layers of its neighbours -- the last layers of the box wrap round to rank 0, hence three), laid out back to back in "list rows":
// range k starts at list row base[k], a multiple of 256, so that no workgroup straddles two ranges.  The per-step pair list is
// stored by list row; a pass over the own rows alone (n = 1) therefore reads the list a pass over all ranges wrote.
struct RowMap {
    int n, lo[3], hi[3], base[3];
    __host__ __device__ int list_rows() const { return n ? base[n - 1] + ((hi[n - 1] - lo[n - 1] + 255) & ~255) : 0; }
    // sorted row of list row lr, or -1 (padding)
    __device__ __forceinline__ int first_row() const { return hi[0] > lo[0] ? lo[0] : (n > 1 && hi[1] > lo[1] ? lo[1] : lo[2]); }
    __device__ __forceinline__ int row(int lr) const {   // (constant indices only: the struct then lives in scalar registers, also when it was loaded from memory)
        int l = lo[0], h = hi[0], b = base[0];
        if (n > 1 && lr >= base[1]) { l = lo[1]; h = hi[1]; b = base[1]; }
        if (n > 2 && lr >= base[2]) { l = lo[2]; h = hi[2]; b = base[2]; }
        const int i = l + (lr - b);
        return i < h ? i : -1;
    }
};
struct RowRanges { int n, lo[3], hi[3]; };   // up to three disjoint row ranges (own rows and the two ghost regions)
// Row space of an owned-particle rank (pse_team_step_local), written ON THE DEVICE by the cell sort of the step (k_local_scatter):
// the host never learns these numbers inside a step -- kernels are launched for the capacities and read their rows here.
//   own rows [0, n_own) | left ghosts [c_own, c_own + n_gl) | right ghosts [c_own + c_g, c_own + c_g + n_gr)      (c_own, c_g: capacities)
struct LocalRows {
    int n_own, n_gl, n_gr;
    int first_end;                // own rows [0, first_end): the first `depth` cell layers -- the left neighbour's right ghosts
    int last_begin;               // own rows [last_begin, n_own): the last `depth` layers -- the right neighbour's left ghosts
    int ok;                       // 0: a capacity was exceeded (flagged): every range here is empty
    RowMap own, own1;             // own rows; own rows + the ADJACENT ghost layer on either side (list-row bases as RowMap wants them)
    RowRanges all;                // own + all ghost rows
};
// rows of a near-field / vector pass given on the device (rm nullable: the RowMap passed by value counts), + where a mat-vec
// parks the rows of the last `depth` layers on their way to the right neighbour (their first row is known on the device only)
struct DevRowArgs {
    const RowMap *rm;             // device
    const LocalRows *lr;          // device (nullable): for stage_hi
    double4 *stage_hi;            // rows [lr->last_begin, lr->n_own) of the result also go to stage_hi[row - last_begin]
    int rows_cap;                 // list rows to launch for (>= what *rm will say)
    int stage_cap;                // rows stage_hi holds (the ghost capacity c_g)
};
// a RowMap in scalars: what a kernel works with when the map may come from device memory (assigning a loaded struct to the by-value
// kernel argument put it in scratch memory: 44 bytes per lane and 20 % on the pair-list mat-vec)
struct RowMapRegs {
    int n, l0, l1, l2, h0, h1, h2, b1, b2;
    __device__ __forceinline__ RowMapRegs(const RowMap &m, const RowMap *dev) {
        n = m.n; l0 = m.lo[0]; l1 = m.lo[1]; l2 = m.lo[2]; h0 = m.hi[0]; h1 = m.hi[1]; h2 = m.hi[2]; b1 = m.base[1]; b2 = m.base[2];
        if (dev) { n = dev->n; l0 = dev->lo[0]; l1 = dev->lo[1]; l2 = dev->lo[2]; h0 = dev->hi[0]; h1 = dev->hi[1]; h2 = dev->hi[2]; b1 = dev->base[1]; b2 = dev->base[2]; }
    }
    __device__ __forceinline__ int list_rows() const { return n == 0 ? 0 : (n == 1 ? ((h0 - l0 + 255) & ~255) : (n == 2 ? b1 + ((h1 - l1 + 255) & ~255) : b2 + ((h2 - l2 + 255) & ~255))); }
    __device__ __forceinline__ int first_row() const { return h0 > l0 ? l0 : (n > 1 && h1 > l1 ? l1 : l2); }
    __device__ __forceinline__ int row(int lr) const {
        int l = l0, h = h0, b = 0;
        if (n > 1 && lr >= b1) { l = l1; h = h1; b = b1; }
        if (n > 2 && lr >= b2) { l = l2; h = h2; b = b2; }
        const int i = l + (lr - b);
        return i < h ? i : -1;
    }
};
inline RowMap row_map(int lo, int hi) { return RowMap{1, {lo, 0, 0}, {hi, 0, 0}, {0, 0, 0}}; }
inline RowMap row_map(const int (*rg)[2], int n) {
    RowMap m{};
    m.n = n;
    int base = 0;
    for (int k = 0; k < n; ++k) { m.lo[k] = rg[k][0]; m.hi[k] = rg[k][1]; m.base[k] = base; base += (rg[k][1] - rg[k][0] + 255) & ~255; }
    return m;
}

// A launch that runs only on one outcome of a decision taken ON THE DEVICE earlier in the stream (asynchronous mode: whether the kept
// neighbour list may be reused): every workgroup reads the word and leaves at once when the gate is closed.  word = null: always open.
struct Gate {
    const int *word;
    int want;   // 1: run if *word != 0 (rebuild), 0: run if *word == 0 (reuse)
    __device__ __forceinline__ bool closed() const { return word != nullptr && ((*word != 0) != (want != 0)); }
};
// gate word <- flags[0] | flags[1] (moved beyond the skin | a row overflowed at the build); a rebuild starts with flags[1] cleared
void launch_gate_decide(int *flags, int *word, hipStream_t s);
void launch_gate_zero(Gate g, int *a, size_t na, int *b, size_t nb, hipStream_t s);          // two int ranges zeroed if the gate is open
void launch_gate_copy(Gate g, double4 *dst, const double4 *src, size_t n, hipStream_t s);    // dst <- src if the gate is open
// n > 0 (a slab rank that keeps only some cell layers): the particles of cells it does not keep are counted per slab of
// cells_per_slab storage cells, on cell book[slab] -- the first cell of that slab the rank does not keep
struct SlabBook { int n, cells_per_slab, spread, book[64]; };   // spread: the counts go to cells book[slab] .. book[slab] + spread - 1 (one layer)
hipError_t cell_sort(const double4 *pos, const unsigned *group, int N, DBox box, DCells nc, unsigned *keys, unsigned *rank,
                     unsigned *slots, int *cnt, int ncell, void *tmp, size_t tmp_bytes, int *cell_off, unsigned *perm, hipStream_t s,
                     CellRanges need = CellRanges{}, SlabBook sb = SlabBook{}, bool cnt_is_zero = false,   // cnt[0 .. ncell] already zeroed by the caller
                     Gate gate = Gate{});
// exclusive prefix sum of n ints (the cell counts -> row offsets), same scratch as cell_sort
hipError_t launch_cell_scan(const int *cnt, int *out, int n, void *tmp, size_t tmp_bytes, hipStream_t s);
// pos_s[i] = wrapped position of particle perm[i], vec_s[i] = vec[tag].xyz, tag_s[i] = its index in the caller's arrays
// pos_build (nullable): the sorted positions the neighbour list was built at; a particle that has moved more than
// sqrt(half_skin2) from there (minimum image) sets flags[0] -- HOOMD's NeighborList distance check (r_buff / 2)
void launch_permute(const double4 *pos, const double4 *vec, const unsigned *group, const unsigned *perm, int N, DBox box,
                    double4 *pos_s, float4 *posf_s, double2 *pv, double4 *vec_s, unsigned *tag_s, hipStream_t s,
                    const double4 *pos_build = nullptr, double half_skin2 = 0.0, int *flags = nullptr,
                    CellRanges need = CellRanges{}, const int *cell_off = nullptr,    // a slab rank: the needed rows only
                    const struct FarBinArgs *far = nullptr,                           // rank the particles in their far-field bins
                    double4 *psi_s = nullptr, uint32_t seed = 0, uint32_t timestep = 0,    // draw the particle noise of this step (K14)
                    Gate gate = Gate{}, const uint32_t *ts_off = nullptr);             // ts_off (nullable): ... at timestep + *ts_off
void launch_permute_vec(const double4 *vec, const unsigned *tag_s, int N, double4 *vec_s, hipStream_t s);

// ---- near field (K9) -------------------------------------------------------------------------------------
// Per-step pair list, 16 B per pair, in wave-blocked ELL layout: four slots of the 64 rows a wavefront owns form one
// contiguous 4096-byte group [4 slots][64 lanes] of records (neighbour row 27 bits | sign of h | fr 26-bit fixed point | s = d sqrt|h| as
// three 22-bit mantissas under one exponent: nb_pack in pse_kernels.hip; pair term f v + sgn (s.v) s), groups of one wave back to back
// -- a wave streams one contiguous region with 16-byte loads only.  Read by the Lanczos mat-vecs only.
// Row r = i - lo (lo: first row of the rank, fixed within a step); record (r / 64) * cap + slot.
// c64 (nullable): the fp64 Lanczos operator (pse_set_lanczos_operator) -- a parallel plane of 32-byte records (f, s = d sqrt|h|) in
// the same geometry (record k of data <-> c64[k]); the 16-byte record then supplies the row and the sign of h only.  Kernels that
// see c64 != null take their F64 instantiation: the list passes write the plane, the mat-vecs read it and gather the rows as doubles.
struct NbList {
    char *data;
    int *cnt;             // neighbour count per particle; -1 if it exceeded cap (dense cluster): that row walks the cells
    int cap;
    double4 *c64;
};
__host__ __device__ inline size_t nb_list64_bytes(size_t rows, int cap) { return ((rows + 63) / 64) * (size_t)cap * 64 * 32; }
// Neighbour (Verlet) list kept ACROSS steps, as the reference keeps HOOMD's NeighborListGPUBinned(rcut, r_buff = 0.4) with a
// distance check every step (PSEv1/integrate.py:60,79; Stokes.cc:433): every pair closer than rcut + skin when it was built.
// The same wave-blocked layout, entries only: groups of four slots [64 lanes][4 x u32 neighbour slot] = 1024 bytes.
struct VerletList {
    unsigned *idx;
    int *cnt;             // entries per row; -1: the row did not fit (flags[1] is set: the list is not reused)
    int cap;              // slots per row, a multiple of 4
    int *flags;           // [0] a particle moved beyond skin / 2 since the build, [1] a row overflowed at the build
    double rskin;         // rcut + skin
};
__host__ __device__ inline size_t verlet_list_bytes(size_t rows, int cap) { return ((rows + 63) / 64) * (size_t)(cap / 4) * 1024; }
enum { VL_NONE = 0, VL_WRITE = 1, VL_USE = 2 };
constexpr size_t NB_REC = 64 * 16;   // 64 rows x one 16-byte record
__host__ __device__ inline size_t nb_list_bytes(size_t rows, int cap) { return ((rows + 63) / 64) * (size_t)cap * NB_REC; }
enum { MREAL_CELLS = 0, MREAL_BUILD_LIST = 1, MREAL_USE_LIST = 2 };
// Lanczos sums fused into the pair-list mat-vec (see k_lz_update): with x = vec and y = M x the kernel also leaves the
// per-block partial sums of x.x, x.y and x.x_{j-1} -- or (sums = 4, a single GPU from iteration 1 on) of x.y alone: x.x and
// x.x_{j-1} were summed by the k_lz_update that wrote x, which held both rows in registers (its `next_sums`, pse_vectors.h)
struct LzFuse {
    const double4 *vprev;   // x_{j-1}, unnormalised (null for j = 0; not read with sums = 4)
    double *partials;       // [LZ_NGRAM][npart_cap]
    int npart_cap;
    const double4 *q, *p, *u;   // two-step blocks of a team (sums = 2, 3): v_j, v_{j-1} (nullable), M v_{j-1} (nullable)
    // sums = 4: what the update that wrote x left, [2][LZ_NPART] partials of x.x and x.x_{j-1}, n_upd of each: the reduction
    // launch behind the mat-vec adds them next to the mat-vec's own partials of x.y, so scal[LZ_TMP ..] ends as with sums = 1
    const double *upd;
    int n_upd;
};
// slots of the Gram sums of a two-step block (k_lz_block): products of q = v_j, p = v_{j-1}, u = M p, w1 = M q, w2 = M w1
// -- the eight that M = M^T leaves independent: q.w2 = w1.w1, u.w1 = p.w2, q.u = p.w1 (the pair list holds every pair twice with
// bit-identical coefficients, so the products agree to summation rounding), and u.u is carried over from the block that made u
enum { LZG_QW1 = 0, LZG_W1W1, LZG_W1W2, LZG_W2W2, LZG_PW1, LZG_PW2, LZG_UW2, LZG_QQ, LZ_NGRAM };
// out = M_real . vec (+ self). mode: cells only / cells + write the pair list / use the pair list
// rows [lo, hi) of the mat-vec (the whole vector is read; multi-GPU ranks each take a row range)
void launch_mreal(const double4 *pos_s, const float4 *posf_s, const double4 *vec_s, double4 *out_s, RowMap rows,
                  const int *cell_off, DBox box, DCells nc, double rcut, double self, const double *coef, int ncoef, NbList nb,
                  int mode, hipStream_t s, const double4 *vec2_s = nullptr, double4 *out2_s = nullptr,   // BUILD_LIST: a second vector rides along
                  VerletList vl = VerletList{}, int vl_mode = VL_NONE,   // VL_WRITE: the cell pass also writes the neighbour list; VL_USE: no cell walk
                  const double2 *pv = nullptr,                           // packed (position, vec_s) records for the drain's gathers
                  double *sums0 = nullptr, int sums0_cap = 0, double *scal = nullptr,    // ... and the sums vec2.vec2, vec2.out2 are left in scal[LZ_TMP ..] (Lanczos iteration 0)
                  Gate gate = Gate{},                                    // cell pass / kept-list pass without a pair list: run on one outcome of the device-side list check only
                  DevRowArgs dr = DevRowArgs{});                         // owned-particle ranks: the rows come from device memory (cell passes only; stage_hi takes out2)
bool mreal_table_in_lds(int ncoef);   // the neighbour list across steps needs the LDS copy of the table
// pair-list mat-vec + Lanczos sums; leaves the three reduced sums in scal[LZ_TMP .. LZ_TMP + 2]
// vec and out: each in its own row layout (pse_device.h VecIn / VecOut; a plain double4 pointer converts to the double4 layout).  The
// mirror vec_q, lz.vprev and the vectors of the two-step blocks are what they were.
void launch_mreal_lanczos(const double4 *pos_s, VecIn vec, VecOut out, RowMap rows, const int *cell_off,
                          DBox box, DCells nc, double rcut, double self, const double *coef, NbList nb, LzFuse lz,
                          double *scal, hipEvent_t ev_begin, hipEvent_t ev_end, hipStream_t s,   // events (nullable) bracket the mat-vec kernel
                          VerletList vl = VerletList{},   // in use this step: rows that overflowed the pair list walk it instead of the cells
                          int sums = 1,                   // 0 none, 1 one-step Lanczos sums, 2 Gram sums of a two-step block, 3 single step of that driver,
                                                          // 4 x.y alone; x.x and x.x_{j-1} from lz.upd
                          const int *stop = nullptr,      // nullable: leave at once if *stop != 0 (the device-side Lanczos decision)
                          DevRowArgs dr = DevRowArgs{},   // owned-particle ranks: rows from device memory
                          const void *vec_q = nullptr,    // (sums == 1) the 16-byte mirror of vec_s (launch_lz_update's xq): the neighbours' rows in ONE gather per pair
                          bool no_reduce = false);        // the mat-vec kernel only: no reduction of its partial sums behind it
int mreal_partials_needed(int rows);
void launch_eval_fg(const double *r, int n, const double *coef, double *f, double *g, hipStream_t s);

}  // namespace pse
