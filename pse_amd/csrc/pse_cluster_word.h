// What the host and the device share of the cluster analysis with percolation (pse_clusters_span, include/pse_amd.h): the 64-bit word
// of the union-find with image offsets, the bits of the status word, the fixed-point scale of the geometry and the ONE fp64 expression
// of the radius of gyration.  No HIP header: pse_host_api.cpp and the sanitizer build include it too.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PSE_HD __host__ __device__ __forceinline__
#else
#define PSE_HD inline
#endif

namespace pse {

// The word of row x: bits 0..27 the parent row, bits 28..39, 40..51, 52..63 the offset c_x - c_parent along a1, a2, a3 as 12-bit
// two's-complement fields.  A root is (x, 0, 0, 0), which is the number x.
constexpr int CLUSTER_WORD_PARENT_BITS = 28, CLUSTER_WORD_OFFSET_BITS = 12;
constexpr unsigned CLUSTER_WORD_MAX_ROWS = 1u << CLUSTER_WORD_PARENT_BITS;                 // n above this: CLUSTER_CAP_ROWS
constexpr int CLUSTER_WORD_MAX_OFFSET = (1 << (CLUSTER_WORD_OFFSET_BITS - 1)) - 1;          // 2047; beyond it: CLUSTER_CAP_OFFSET
// bits of the object's sticky status word: the two trip caps of pse_clusters_label, then the three caps of pse_clusters_span
constexpr unsigned CLUSTER_CAP_FIND_BIT = 1u, CLUSTER_CAP_UNITE_BIT = 2u, CLUSTER_CAP_OFFSET = 4u, CLUSTER_CAP_Q = 8u, CLUSTER_CAP_ROWS = 16u;

PSE_HD bool cluster_offset_fits(int cx, int cy, int cz) {
    const int m = CLUSTER_WORD_MAX_OFFSET;
    return cx >= -m && cx <= m && cy >= -m && cy <= m && cz >= -m && cz <= m;
}
// (the caller has checked parent < 2^28 and cluster_offset_fits)
PSE_HD unsigned long long cluster_word_pack(unsigned parent, int cx, int cy, int cz) {
    return (unsigned long long)parent | ((unsigned long long)((unsigned)cx & 0xfffu) << 28) | ((unsigned long long)((unsigned)cy & 0xfffu) << 40) |
           ((unsigned long long)((unsigned)cz & 0xfffu) << 52);
}
PSE_HD unsigned cluster_word_parent(unsigned long long w) { return (unsigned)(w & 0xfffffffull); }
PSE_HD int cluster_word_field(unsigned long long w, int shift) { return (int)(((unsigned)(w >> shift) & 0xfffu) ^ 0x800u) - 0x800; }
PSE_HD void cluster_word_unpack(unsigned long long w, unsigned &parent, int &cx, int &cy, int &cz) {
    parent = cluster_word_parent(w);
    cx = cluster_word_field(w, 28); cy = cluster_word_field(w, 40); cz = cluster_word_field(w, 52);
}

// Geometry: q = llrint(D 2^20) per component, |q| < 2^31 (D below 2048 length units; beyond it: CLUSTER_CAP_Q).
constexpr double CLUSTER_Q_SCALE = 1048576.0;                   // 2^20
constexpr long long CLUSTER_Q_LIMIT = 1ll << 31;
// Rg^2 of a cluster of s members from its integer sums: sq = sum q (three signed words), lo = sum of the low 32 bits of every q_k^2,
// hi = sum of q_k^2 >> 32.  ONE expression, evaluated in this order without contraction on the host and on the device:
//   S2 = (double)hi 2^32 + (double)lo;  M = ((sx sx + sy sy) + sz sz) / (s s);  Rg^2 = 2^-40 (S2 / s - M).
// Roundings while hi, lo, the components of sq and s s are below 2^53 (every conversion and s s exact; so at every size tested): the
// sum and the quotient of S2, 2 u; three squares, two sums and the quotient of M, at most 4 u; the difference, 1 u, u = 2^-53, each of
// a number that is at most sum q^2 / s (Cauchy-Schwarz: M <= S2 / s).  |error| <= 7 u 2^-40 sum q^2 / s.
PSE_HD double cluster_rg2(long long sx, long long sy, long long sz, unsigned long long lo, unsigned long long hi, unsigned s) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double n = (double)s;
    const double x = (double)sx, y = (double)sy, z = (double)sz;
    const double hi2 = (double)hi * 4294967296.0;
    const double S2 = hi2 + (double)lo;
    const double xx = x * x, yy = y * y, zz = z * z;
    const double xy = xx + yy;
    const double m2 = xy + zz;
    const double nn = n * n;
    const double M = m2 / nn;
    const double mean2 = S2 / n;
    const double diff = mean2 - M;
    return diff * (1.0 / 1099511627776.0);   // 2^-40: exact
}

}  // namespace pse
