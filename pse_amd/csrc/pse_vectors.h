// Launch wrappers of the vector kernels (defined in pse_vectors.hip).  All take the stream explicitly.
#pragma once
#include "pse_host.h"
#include "pse_kernels.h"

namespace pse {

// ---- vector kernels (K10-K14) ----------------------------------------------------------------------------
void launch_psi(double4 *psi_s, const unsigned *tag_s, int N, uint32_t seed, uint32_t timestep, hipStream_t s,
                CellRanges need = CellRanges{}, const int *cell_off = nullptr);
// scal layout (device doubles): [0..127] alpha, [128..255] beta, [256] psi norm (LZ_ALPHA, LZ_BETA, LZ_NORM: pse_host.h), [257] scratch
constexpr int LZ_TMP = 257, LZ_UU = 272, LZ_NSCAL = 400;   // TMP: 3 sums (one-step) or the LZ_NGRAM sums of a two-step block; UU[j] = |M v_{j-1}|^2 of the block that starts at j
constexpr int LZ_NPART = 1024;  // partial-sum slots
// scal[LZ_TMP + q] = sum of partials[q * cap .. q * cap + npart), q < nsum, in a fixed order; stop (nullable): leave at once if *stop != 0
void launch_lz_reduce(const double *partials, int npart, int cap, int nsum, double *scal, const int *stop, hipStream_t s);
// out_s = scale * sum_q t[q] X[q], X[0] = x0, X[q] = V[q] (the UNNORMALISED Lanczos vectors: t carries the 1 / |x_q|)
// rows [lo, hi)
struct BasisCoef { double t[104]; };   // the m <= 100 coefficients of the final combination, passed by value
// sink.on: the result is not stored in out_s but added to add_a + add_b (nullable) of the row and sent on: vel[tag].xyz (single GPU) or
// rows[i] = (sum, tag) (a team's all-gathered array)
struct CombineSink { bool on; const double4 *add_a, *add_b; const unsigned *tag_s; double4 *vel; double4 *rows; };
// x0 and V each in their own layout (pse_device.h VecIn); stride: ROWS from one basis vector to the next
void launch_basis_combine(VecIn x0, VecIn V, size_t stride, const BasisCoef &t, int m, const double *scal,
                          double scale, int use_norm, double4 *out_s, int lo, int hi, hipStream_t s, CombineSink sink = CombineSink{},
                          const struct LzState *st = nullptr);   // st: m and the coefficients come from the device-side decision
// Lanczos iteration on the own rows [lo, hi) (see k_lz_update in pse_vectors.hip).  dots: sums of x.x, x.y, x.vprev ->
// scal[LZ_TMP..+2] (y = null: x.x only), for mat-vecs that did not fuse them; [all-reduce by the caller when sharded];
// update: alpha_j, beta_j -> scal, x_{j+1} -> xnext
void launch_lz_dots(const double4 *x, const double4 *y, const double4 *vprev, int lo, int hi, double *partials, int cap,
                    double *scal, hipStream_t s);
// one block of the two-iterations-per-exchange Lanczos of a team (k_lz_block in pse_vectors.hip)
struct LzBlockArgs {
    const double4 *q, *p, *w1, *w2;   // p null for j = 0; w2 null: a single step (scalars alpha_j, beta_{j+1} only)
    double4 *u;                       // in: M p (not read for j = 0); out: M v_{j+1} (two steps) or M v_j = w1 (one step)
    double4 *v1, *v2;                 // V[j + 1], V[j + 2]
    int j;
};
// sums_all / nranks (teams): [nranks][LZ_NGRAM] partial sums of all ranks, added in rank order by the kernel; nranks = 0: scal[LZ_TMP ..]
// sch: the host's copy of the scalars (device pointer of mapped pinned memory, nullable): alpha, beta, the norm are written there too
void launch_lz_block(const LzBlockArgs &a, bool full, double *scal, const int (*row_ranges)[2], int n_ranges, hipStream_t s,
                     const double *sums_all = nullptr, int nranks = 0, double *sch = nullptr,
                     const RowRanges *rg_dev = nullptr, int rows_cap = 0,   // owned-particle ranks: the ranges come from device memory (vectors_off: scalars only)
                     bool vectors_off = false, const int *stop = nullptr);
void launch_vq_roundtrip(const double *in, double *out, int n, hipStream_t s);   // debug: vq_unpack(vq_pack(row)) of n rows of three doubles
// Two of the three sums of iteration j, x_j.x_j and x_j.x_{j-1}, need no pass of their own: the update that wrote x_j had both rows
// in registers.  A launch given next_sums ([2][LZ_NPART]) leaves one pair of partial sums per workgroup there -- x_{j+1}.x_{j+1},
// then x_{j+1}.x_j; fixed rows per workgroup, so a fixed summation order -- and the pair-list mat-vec of iteration j + 1 then sums
// x.y alone (launch_mreal_lanczos, sums = 4, LzFuse.upd): the one reduction launch behind it adds these partials as well.
int lz_update_grid(int rows);   // workgroups launch_lz_update uses for this many rows: the partials per sum it leaves
// scal[LZ_TMP + 1] = sum of xy[0 .. n_xy), scal[LZ_TMP] and scal[LZ_TMP + 2] = the sums of upd[0 .. n_upd) and upd[LZ_NPART .. + n_upd)
void launch_lz_reduce_split(const double *xy, int n_xy, const double *upd, int n_upd, double *scal, const int *stop, hipStream_t s);
// xin, y, xprev (p null: none), xnext: each array with its own row layout (pse_device.h VecIn / VecOut)
void launch_lz_update(VecIn xin, VecIn y, VecIn xprev, VecOut xnext, int j,
                      double *scal, const int (*row_ranges)[2], int n_ranges, hipStream_t s,   // up to three disjoint row ranges in one launch
                      const double *sums_all = nullptr, int nranks = 0, double *sch = nullptr, const int *stop = nullptr,
                      void *xq = nullptr,    // nullable: [rows] 16-byte mirror of xnext (vq_pack, pse_device.h), written on the same rows
                      double *next_sums = nullptr);   // nullable: see above; not written by a launch without rows (scalars only)
// ---- the convergence decision of the Lanczos iteration ON THE DEVICE (queue-only Brownian calls: pse_set_async) ----------------
// Replaces, for calls that may not wait for the host, what the host driver does between batches of iterations (the reference's
// LAPACKE_spteqr + host loops, PSEv1/Brownian.cu:540-582, and its step-norm test, PSEv1/Brownian.cu:673-724): one workgroup solves
// the tridiagonal eigenproblems of the sizes to be checked (one wavefront each, implicit QL as tridiag_eigen in pse_params.cpp),
// walks m upward exactly as the host does and, once the step norm is below the tolerance, closes the gate `done` that every later
// kernel of the iteration reads, and leaves the coefficients of the final combination for k_basis_combine.  LzState and LzDecide,
// the contract it shares with the host drivers' lz_decide_host: pse_host.h.
constexpr int LZ_HOST_M = 380, LZ_HOST_STEPNORM = 381, LZ_HOST_STATUS = 382, LZ_HOST_SEQ = 383, LZ_HOST_OPEN = 384;   // (OPEN: calls so far that ended with status != 0)   // slots of the host mirror (sch) the decision writes
void launch_lz_decide(const LzDecide &d, double *scal, LzState *st, double *sch, double seq, hipStream_t s);
bool lz_decide_supported(int m_hi);   // the eigenvectors of both sizes fit the LDS of one workgroup
// tag_s (nullable): out[i].w = the particle's index in the caller's arrays, so the rows can be scattered by ranks that did not sort them
void launch_sum_rows(const double4 *a, const double4 *b, const double4 *c, double4 *out, int lo, int hi, hipStream_t s,
                     const unsigned *tag_s = nullptr);
void launch_pick(const int *cell_off, const int *idx, int n, int *out, hipStream_t s);
// vel[tag].xyz = a + b + c (each may be null), keep w;  tag_s = null: the tag travels in a[s].w (launch_sum_rows)
void launch_scatter_sum(const double4 *a, const double4 *b, const double4 *c, const unsigned *tag_s, int N,
                        double4 *vel, hipStream_t s);
void launch_integrate(double4 *pos, const double4 *vel, double3 *accel, int3 *image, const double4 *force,
                      const unsigned *group, int N, DBox box, double dt, double shear_rate, hipStream_t s);
void launch_add_inplace(double *a, const double *b, size_t n, hipStream_t s);
// in-process teams: the device copies that stand for one exchange, as ONE launch (a message transport posts one group too)
struct CopyList { int n; const double *src[40]; double *dst[40]; unsigned cnt[40]; };   // counts in doubles
void launch_copy_list(const CopyList &l, hipStream_t s);

}  // namespace pse
