// Launch wrappers of the bond-orientational order kernels (defined in pse_order.hip).  All take the stream explicitly.
#pragma once
#include <hip/hip_runtime.h>

#include "pse_forces.h"

namespace pse {

// bond-orientational order (pse_bond_order_compute): the device arrays, the neighbour distances and the degrees of one object.  types,
// type_s: as in PairHist.  rnb2: npt squares of the neighbour distances (0: off), r2_all the largest.  degree[d], d < nl: the even
// degrees; a sorted row's c_lm are ONE row of `stride` complex numbers at clm + i stride, the l + 1 values m = 0..l of degree d
// contiguous at offset off[d] -- 16-byte aligned, one or two cache lines per neighbour gather.  ql_s: the q_l of the sorted rows,
// row i at ql_s + i nl.  Both are rewritten by every call.  Two sorted rows are neighbours when 0 < r^2 < rnb2[p] and the pair is not
// in `ex`.  nnb, q, qbar and nconn are written by caller index (tag_s), stats (2 ntypes words) is overwritten; each may be null.
struct BondOrder {
    const unsigned char *types;
    unsigned char *type_s;
    unsigned n;
    int ntypes;
    const double *rnb2;
    double r2_all;
    int nl, stride;
    int degree[BOND_ORDER_MAX_DEGREES], off[BOND_ORDER_MAX_DEGREES];
    double2 *clm;
    double *ql_s;
};
void launch_bond_order(const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc, const BondOrder &bo,
                       unsigned *nnb, double *q, double *qbar, int solid_degree, double threshold, unsigned min_conn, unsigned *nconn,
                       unsigned long long *stats, hipStream_t s, const PairExclusions *ex = nullptr);
// per-type histogram of one column of a caller-order array of nl columns (pse_bond_order_histogram): the group member t of type a with
// lo <= v < hi, v = values[t nl + column], adds 1 to counts[a nbins + b], b = min((int)((v - lo) nbins / (hi - lo)), nbins - 1).
// A caller index >= n_max is skipped.
void launch_bond_order_hist(const double *values, int nl, int column, const unsigned *group, int N, unsigned n_max, const BondOrder &bo,
                            int nbins, double lo, double hi, unsigned long long *counts, hipStream_t s);

}  // namespace pse
