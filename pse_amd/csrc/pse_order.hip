// Kernels of the bond-orientational order (pse_order.h; pse_bond_order_compute, pse_bond_order_histogram): the Steinhardt q_l per
// particle, the neighbour-averaged q-bar_l and the solid-like bonds, on the engine's cell list.  gfx950, wave64, fp64.
//
// For the unit vector d = (x, y, z) to a neighbour the semi-normalised harmonic of degree l and order m >= 0 is
//   C_lm(d) = sqrt((l - m)!/(l + m)!) P_l^m(z) e^{i m phi} = T_l^m(z) (x + i y)^m,    T_l^m(z) = sqrt((l - m)!/(l + m)!) P_l^m(z)/sin^m(theta),
// with the Condon-Shortley phase in P_l^m.  T_l^m is a POLYNOMIAL in z (the m-th derivative of P_l, scaled): there is no angle, no
// trigonometric call and nothing singular at the poles, where (x + i y)^m vanishes by itself.  For a fixed m it obeys, upward in l,
//   T_m^m = (-1)^m sqrt((2m - 1)!!/(2m)!!),    T_{m+1}^m = sqrt(2m + 1) z T_m^m,
//   T_l^m = a_lm z T_{l-1}^m - b_lm T_{l-2}^m,   a_lm = (2l - 1)/sqrt(l^2 - m^2),   b_lm = sqrt(((l - 1)^2 - m^2)/(l^2 - m^2)),
// the stable direction of the three-term recurrence; every a, b and starting value is a compile-time constant of the instantiation
// for the degree L (bo_a, bo_b, bo_start: a constexpr Newton square root, within one ulp), the recursion is unrolled by templates,
// and a step is one product a z, one product b T and one fused multiply-add.  (x + i y)^m comes from m - 1 complex multiplications.
// Only m = 0..L is formed: c_{l,-m} = (-1)^m conj c_lm.  The error of one term against the exact harmonic of the same d is bounded in
// DESIGN.md (tests/bond_order_ref.py restates the arithmetic in NumPy and evaluates the bound).
#include "pse_order.h"
#include "pse_excl.h"

#include <type_traits>

namespace pse {

// sqrt(x) for the compile-time coefficients: Newton from above, which decreases until it has converged; within one ulp.
constexpr double bo_sqrt(double x) {
    double r = x > 1.0 ? x : 1.0;
    for (int k = 0; k < 200; ++k) {
        const double n = 0.5 * (r + x / r);
        if (!(n < r)) break;
        r = n;
    }
    return r;
}
constexpr double bo_a(int l, int m) { return (double)(2 * l - 1) / bo_sqrt((double)((l - m) * (l + m))); }
constexpr double bo_b(int l, int m) { return bo_sqrt((double)((l - 1 - m) * (l - 1 + m)) / (double)((l - m) * (l + m))); }
constexpr double bo_start(int m) {   // T_m^m
    double p = 1.0;
    for (int k = 1; k <= m; ++k) p *= (double)(2 * k - 1) / (double)(2 * k);
    const double s = bo_sqrt(p);
    return (m & 1) ? -s : s;
}
// T_L^M(z) from p1 = T_{l-1}^M and p2 = T_{l-2}^M, upward from l
template <int L, int M, int l>
__device__ __forceinline__ double bo_up(double z, double p1, double p2) {
    if constexpr (l > L) {
        return p1;
    } else {
        constexpr double a = bo_a(l, M), b = bo_b(l, M);
        return bo_up<L, M, l + 1>(z, fma(a * z, p1, -(b * p2)), p1);
    }
}
template <int L, int M>
__device__ __forceinline__ double bo_legendre(double z) {
    constexpr double s = bo_start(M);
    if constexpr (M == L) {
        return s;
    } else {
        constexpr double a1 = bo_a(M + 1, M);
        return bo_up<L, M, M + 2>(z, (a1 * z) * s, s);
    }
}
// adds C_Lm(d), m = M..L, to the accumulators: (wx, wy) = (x + i y)^M on entry
template <int L, int M>
__device__ __forceinline__ void bo_terms(double z, double wx, double wy, double x, double y, double (&ar)[L + 1], double (&ai)[L + 1]) {
    const double t = bo_legendre<L, M>(z);
    ar[M] = fma(t, wx, ar[M]);
    ai[M] = fma(t, wy, ai[M]);
    if constexpr (M < L) bo_terms<L, M + 1>(z, wx * x - wy * y, wx * y + wy * x, x, y, ar, ai);
}
// |c|^2 summed over m = -L..L from the stored half, m ascending: |c_0|^2 + 2 |c_1|^2 + ...
template <int L>
__device__ __forceinline__ double bo_norm2(const double (&cr)[L + 1], const double (&ci)[L + 1]) {
    double s = cr[0] * cr[0] + ci[0] * ci[0];
#pragma unroll
    for (int m = 1; m <= L; ++m) s += 2.0 * (cr[m] * cr[m] + ci[m] * ci[m]);
    return s;
}
__device__ __forceinline__ int bo_pair_type(int ti, int tj, int ntypes) {
    const int lo = min(ti, tj), hi = max(ti, tj);
    return lo * ntypes - ((lo * (lo - 1)) >> 1) + (hi - lo);
}

// Pass 1, one instantiation per degree: c_Lm(i) = (1/nb) sum_j C_Lm(d_ij) over the neighbours of sorted row i, and q_L(i).  One thread
// per sorted row, the walk of k_pair_hist over the FULL neighbour range (every j, not j > i: the relation is symmetric, every row
// needs its own sum), rn2[p] = rnb[p]^2 staged in LDS as in k_cluster_link.  Per pair: first the prefilter r^2 < max_p rn2 (one bound
// for the whole wave; the lanes pass or fail it each for itself) and r^2 > 0 (which also drops j == i), behind it the partner's
// type byte, the pair type's own rn2 and the exclusion lookup; a neighbour then costs one square root and one division for d = (r_j - r_i)/r and the L + 1 terms.  The 2 (L + 1) sums stay in registers (26 doubles at
// L = 12) and are added to in walk order: the sort is stable, so equal inputs give equal bits.  nb = 0 gives c = 0 and q = 0.
// The row of c_Lm and q_L go to the workspace by sorted row (pass 2 gathers them), nnb and q to the caller's arrays by tag.
// clm, ql_s and q point at this degree's offset and column.  No lane leaves before the barrier.
template <int L, bool EXCL>
__global__ void __launch_bounds__(TPB)
k_bond_order_c(const double4 *__restrict__ pos_s, const unsigned *__restrict__ tag_s, const unsigned char *__restrict__ type_s, int N,
               const int *__restrict__ cell_off, DBox box, DCells nc, int ntypes, const double *__restrict__ rnb2 /* npt */, double r2_all,
               double2 *__restrict__ clm, int stride, double *__restrict__ ql_s, int nl, unsigned *__restrict__ nnb, double *__restrict__ q,
               ExclRows ex) {
    __shared__ double rn2[PAIR_TYPED_MAX_PAIR_TYPES];
    if ((int)threadIdx.x < ntypes * (ntypes + 1) / 2) rn2[threadIdx.x] = rnb2[threadIdx.x];
    __syncthreads();
    const int i = xcd_block(blockIdx.x, gridDim.x) * TPB + threadIdx.x;
    if (i < N) {
        const double4 pi = pos_s[i];
        double fx, fy, fz;
        frac_coords(box, pi.x, pi.y, pi.z, fx, fy, fz);
        const int cx = cell_coord(fx, nc.nx), cy = cell_coord(fy, nc.ny), cz = cell_coord(fz, nc.nz);
        const int ti = type_s[i];
        const unsigned tag = tag_s[i];
        unsigned eb = 0u, ee = 0u;
        if (EXCL) excl_row(ex, tag, eb, ee);
        double ar[L + 1], ai[L + 1];
#pragma unroll
        for (int m = 0; m <= L; ++m) ar[m] = ai[m] = 0.0;
        unsigned nb = 0u;
        for_each_run(nc, cell_off, cx, cy, cz, [&](int jb, int je, unsigned) {
            for (int j = jb; j < je; ++j) {
                const double4 pj = pos_s[j];
                double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                min_image(box, dx, dy, dz);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (r2 < r2_all && r2 > 0.0) {
                    const int p = bo_pair_type(ti, type_s[j], ntypes);
                    if (r2 < rn2[p] && !(EXCL && eb < ee && excl_has(ex.ent, eb, ee, tag_s[j]))) {
                        const double ir = -1.0 / sqrt(r2);   // (d = r_j - r_i)
                        bo_terms<L, 0>(dz * ir, 1.0, 0.0, dx * ir, dy * ir, ar, ai);
                        ++nb;
                    }
                }
            }
        });
        const double inv = nb ? 1.0 / (double)nb : 0.0;
        double2 *row = clm + (size_t)i * stride;
#pragma unroll
        for (int m = 0; m <= L; ++m) {
            ar[m] *= inv; ai[m] *= inv;
            row[m] = make_double2(ar[m], ai[m]);
        }
        const double ql = sqrt(bo_norm2<L>(ar, ai));
        ql_s[(size_t)i * nl] = ql;
        if (nnb) nnb[tag] = nb;
        if (q) q[(size_t)tag * nl] = ql;
    }
}

// Pass 2, for the degrees that need q-bar or the solid bonds: the same walk and the same r^2 expression as pass 1, so the neighbour
// set is identical bit for bit.  For each neighbour j the row of c_Lm(j) is gathered (L + 1 contiguous 16-byte words);
// QBAR: it is added to c-bar, which starts from the row's own c_Lm, and q-bar = |c-bar|/(nb + 1) with the norm of pass 1;
// SOLID: s_ij = Re sum_m c_Lm(i) conj c_Lm(j) / (q_L(i) q_L(j)) over m = -L..L (the stored half, m ascending, the m > 0 terms doubled),
// 0 where either q is 0, and the neighbours with s_ij > threshold are counted; the row is solid-like with at least min_conn of them.
// stats (SOLID only; zeroed by k_bond_order_stats_zero): members and solid-like members per type in 2 ntypes unsigned LDS counters,
// flushed behind ONE barrier with one 64-bit integer atomic per non-zero counter.  No lane leaves before a barrier.
template <int L, bool EXCL, bool QBAR, bool SOLID>
__global__ void __launch_bounds__(TPB)
k_bond_order_nb(const double4 *__restrict__ pos_s, const unsigned *__restrict__ tag_s, const unsigned char *__restrict__ type_s, int N,
                const int *__restrict__ cell_off, DBox box, DCells nc, int ntypes, const double *__restrict__ rnb2 /* npt */, double r2_all,
                const double2 *__restrict__ clm, int stride, const double *__restrict__ ql_s, int nl, double *__restrict__ qbar,
                double threshold, unsigned min_conn, unsigned *__restrict__ nconn, unsigned long long *__restrict__ stats, ExclRows ex) {
    __shared__ double rn2[PAIR_TYPED_MAX_PAIR_TYPES];
    __shared__ unsigned st[2 * PAIR_TYPED_MAX_TYPES];
    if ((int)threadIdx.x < ntypes * (ntypes + 1) / 2) rn2[threadIdx.x] = rnb2[threadIdx.x];
    if (threadIdx.x < 2 * PAIR_TYPED_MAX_TYPES) st[threadIdx.x] = 0u;
    __syncthreads();
    const int i = xcd_block(blockIdx.x, gridDim.x) * TPB + threadIdx.x;
    if (i < N) {
        const double4 pi = pos_s[i];
        double fx, fy, fz;
        frac_coords(box, pi.x, pi.y, pi.z, fx, fy, fz);
        const int cx = cell_coord(fx, nc.nx), cy = cell_coord(fy, nc.ny), cz = cell_coord(fz, nc.nz);
        const int ti = type_s[i];
        const unsigned tag = tag_s[i];
        unsigned eb = 0u, ee = 0u;
        if (EXCL) excl_row(ex, tag, eb, ee);
        double cr[L + 1], ci[L + 1], br[L + 1], bi[L + 1];
        const double2 *own = clm + (size_t)i * stride;
#pragma unroll
        for (int m = 0; m <= L; ++m) {
            const double2 v = own[m];
            cr[m] = br[m] = v.x; ci[m] = bi[m] = v.y;
        }
        const double qi = SOLID ? ql_s[(size_t)i * nl] : 0.0;
        unsigned nb = 0u, conn = 0u;
        for_each_run(nc, cell_off, cx, cy, cz, [&](int jb, int je, unsigned) {
            for (int j = jb; j < je; ++j) {
                const double4 pj = pos_s[j];
                double dx = pi.x - pj.x, dy = pi.y - pj.y, dz = pi.z - pj.z;
                min_image(box, dx, dy, dz);
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (r2 < r2_all && r2 > 0.0) {
                    const int p = bo_pair_type(ti, type_s[j], ntypes);
                    if (r2 < rn2[p] && !(EXCL && eb < ee && excl_has(ex.ent, eb, ee, tag_s[j]))) {
                        const double2 *rj = clm + (size_t)j * stride;
                        double dot = 0.0;
#pragma unroll
                        for (int m = 0; m <= L; ++m) {
                            const double2 v = rj[m];
                            if (QBAR) { br[m] += v.x; bi[m] += v.y; }
                            if (SOLID) dot += (m ? 2.0 : 1.0) * (cr[m] * v.x + ci[m] * v.y);
                        }
                        if (SOLID) {
                            const double den = qi * ql_s[(size_t)j * nl];
                            const double sij = den > 0.0 ? dot / den : 0.0;
                            conn += sij > threshold ? 1u : 0u;
                        }
                        ++nb;
                    }
                }
            }
        });
        if (QBAR) {
            const double inv = 1.0 / (double)(nb + 1u);
#pragma unroll
            for (int m = 0; m <= L; ++m) { br[m] *= inv; bi[m] *= inv; }
            qbar[(size_t)tag * nl] = sqrt(bo_norm2<L>(br, bi));
        }
        if (SOLID) {
            if (nconn) nconn[tag] = conn;
            if (stats) {
                atomicAdd(st + 2 * ti, 1u);
                if (conn >= min_conn) atomicAdd(st + 2 * ti + 1, 1u);
            }
        }
    }
    __syncthreads();
    if (SOLID && stats && (int)threadIdx.x < 2 * ntypes && st[threadIdx.x]) atomicAdd(stats + threadIdx.x, (unsigned long long)st[threadIdx.x]);
}

// stats of a call: zeroed in front of the kernel that counts into it ...
__global__ void __launch_bounds__(64)
k_bond_order_stats_zero(int ntypes, unsigned long long *__restrict__ stats) {
    if ((int)threadIdx.x < 2 * ntypes) stats[threadIdx.x] = 0ull;
}
// ... and, without a solid-bond pass, the members per type alone (the solid-like words stay 0), counted as pass 2 counts them
__global__ void __launch_bounds__(TPB)
k_bond_order_members(const unsigned char *__restrict__ type_s, int N, int ntypes, unsigned long long *__restrict__ stats) {
    __shared__ unsigned st[PAIR_TYPED_MAX_TYPES];
    if (threadIdx.x < PAIR_TYPED_MAX_TYPES) st[threadIdx.x] = 0u;
    __syncthreads();
    const int i = blockIdx.x * TPB + threadIdx.x;
    if (i < N) atomicAdd(st + type_s[i], 1u);
    __syncthreads();
    if ((int)threadIdx.x < ntypes && st[threadIdx.x]) atomicAdd(stats + 2 * threadIdx.x, (unsigned long long)st[threadIdx.x]);
}

// the degree of a launch as a std::integral_constant: `launch` is instantiated for the six even degrees
template <class F>
static void with_degree(int L, F &&launch) {
    switch (L) {
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    case 6: launch(std::integral_constant<int, 6>{}); break;
    case 8: launch(std::integral_constant<int, 8>{}); break;
    case 10: launch(std::integral_constant<int, 10>{}); break;
    case 12: launch(std::integral_constant<int, 12>{}); break;
    default: break;   // (refused at creation)
    }
}
void launch_bond_order(const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc, const BondOrder &bo,
                       unsigned *nnb, double *q, double *qbar, int solid_degree, double threshold, unsigned min_conn, unsigned *nconn,
                       unsigned long long *stats, hipStream_t s, const PairExclusions *ex) {
    static_assert(PAIR_TYPED_MAX_PAIR_TYPES <= TPB && BOND_ORDER_MAX_L == 12, "one lane stages one neighbour distance; six even degrees");
    const int nb = nblocks(N, TPB);
    launch_type_mirror(tag_s, N, bo.types, bo.n, bo.type_s, s);
    if (stats) hipLaunchKernelGGL(k_bond_order_stats_zero, dim3(1), dim3(64), 0, s, bo.ntypes, stats);
    const bool solid = solid_degree >= 0 && (nconn || stats);
    // pass 1 only where something reads it: every degree for q or q-bar, the solid degree for its bonds, and one degree -- the first
    // that runs, else the first of the object -- for nnb alone; stats without a solid pass needs none (k_bond_order_members)
    bool need[BOND_ORDER_MAX_DEGREES];
    int counts_nnb = -1;
    for (int d = 0; d < bo.nl; ++d) {
        need[d] = q || qbar || (solid && d == solid_degree);
        if (need[d] && counts_nnb < 0) counts_nnb = d;
    }
    if (nnb && counts_nnb < 0) need[counts_nnb = 0] = true;
    launch_with_excl(ex, [&](auto excl, ExclRows er) {
        constexpr bool EX = decltype(excl)::value;
        for (int d = 0; d < bo.nl; ++d) {
            if (!need[d]) continue;
            with_degree(bo.degree[d], [&](auto deg) {
                hipLaunchKernelGGL((k_bond_order_c<decltype(deg)::value, EX>), dim3(nb), dim3(TPB), 0, s, pos_s, tag_s, bo.type_s, N, cell_off, box,
                                   nc, bo.ntypes, bo.rnb2, bo.r2_all, bo.clm + bo.off[d], bo.stride, bo.ql_s + d, bo.nl,
                                   d == counts_nnb ? nnb : nullptr, q ? q + d : nullptr, er);
            });
        }
        for (int d = 0; d < bo.nl; ++d) {
            const bool sd = solid && d == solid_degree;
            if (!qbar && !sd) continue;
            with_degree(bo.degree[d], [&](auto deg) {
                constexpr int L = decltype(deg)::value;
                auto go = [&](auto kernel) {
                    hipLaunchKernelGGL(kernel, dim3(nb), dim3(TPB), 0, s, pos_s, tag_s, bo.type_s, N, cell_off, box, nc, bo.ntypes, bo.rnb2, bo.r2_all,
                                       bo.clm + bo.off[d], bo.stride, bo.ql_s + d, bo.nl, qbar ? qbar + d : nullptr, threshold, min_conn, nconn, stats, er);
                };
                if (qbar && sd) go(k_bond_order_nb<L, EX, true, true>);
                else if (qbar) go(k_bond_order_nb<L, EX, true, false>);
                else go(k_bond_order_nb<L, EX, false, true>);
            });
        }
    });
    if (stats && !solid) hipLaunchKernelGGL(k_bond_order_members, dim3(nb), dim3(TPB), 0, s, bo.type_s, N, bo.ntypes, stats);
}

// Per-type histogram of one column of a caller-order array (pse_bond_order_histogram): `ncount` = ntypes nbins <=
// BOND_ORDER_MAX_COUNTERS unsigned words of dynamic LDS, zeroed before one barrier, added to by the lanes, and flushed behind ONE more
// barrier with global 64-bit integer atomics on the non-zero counters, as k_pair_hist does.  Neither the sort nor the cell list is
// read: the group member k is the caller index t = group[k] (k without a group), its type types[t] (0 for t >= n), its value
// values[t nl + column].  A value outside [lo, hi), NaN included, is not counted.  The bin is (v - lo) nbins / (hi - lo), evaluated in
// that order -- a subtraction, a product and an IEEE division, nothing to contract -- truncated and clamped to the last bin.
__global__ void __launch_bounds__(TPB)
k_bond_order_hist(const double *__restrict__ values, int nl, int column, const unsigned *__restrict__ group, int N, unsigned n_max,
                  const unsigned char *__restrict__ types, unsigned n, int nbins, int ncount, double lo, double hi,
                  unsigned long long *__restrict__ counts /* [ncount], added to */) {
    extern __shared__ unsigned bh_cnt[];   // [ncount]
    for (int c = threadIdx.x; c < ncount; c += TPB) bh_cnt[c] = 0u;
    __syncthreads();
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k < N) {
        const unsigned t = group ? group[k] : (unsigned)k;
        if (t < n_max) {
            const double v = values[(size_t)t * nl + column];
            if (v >= lo && v < hi) {
                const int a = t < n ? types[t] : 0;
                const int bin = min((int)((v - lo) * (double)nbins / (hi - lo)), nbins - 1);
                atomicAdd(bh_cnt + a * nbins + bin, 1u);
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < ncount; c += TPB) {
        const unsigned v = bh_cnt[c];
        if (v) atomicAdd(counts + c, (unsigned long long)v);
    }
}
void launch_bond_order_hist(const double *values, int nl, int column, const unsigned *group, int N, unsigned n_max, const BondOrder &bo,
                            int nbins, double lo, double hi, unsigned long long *counts, hipStream_t s) {
    static_assert((size_t)BOND_ORDER_MAX_COUNTERS * sizeof(unsigned) <= 32768, "the counters take at most 32 KB of LDS");
    const int ncount = bo.ntypes * nbins;
    hipLaunchKernelGGL(k_bond_order_hist, dim3(nblocks(N, TPB)), dim3(TPB), (size_t)ncount * sizeof(unsigned), s, values, nl, column, group, N,
                       n_max, bo.types, bo.n, nbins, ncount, lo, hi, counts);
}

}  // namespace pse
