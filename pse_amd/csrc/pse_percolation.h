// Launch wrapper of the cluster analysis with percolation (defined in pse_percolation.hip; pse_clusters_span).
#pragma once
#include <hip/hip_runtime.h>

#include "pse_analysis.h"
#include "pse_cluster_word.h"

namespace pse {

// The scratch of pse_clusters_span beside the ClusterLinks of its object (whose types, type_s, rlink2, csize and status it shares),
// n_max entries each, rewritten by every call: word, the union-find with offsets (pse_cluster_word.h); minkey, per root the smallest
// (caller index << 32 | sorted row) of its members; sums, per root five 64-bit words: sum q (three, two's complement), the sum of
// the low 32 bits of every q_k^2, the sum of q_k^2 >> 32; flag, per row the axes (bits 0, 1, 2) of the windings found at it, after
// the flatten complete at the roots.
struct ClusterSpan {
    unsigned long long *word, *minkey, *sums;
    unsigned *flag;
};
// pos: the CALLER's positions (images and geometry are stated for them; the sorted rows are their wrapped copies).  label .. hist as
// launch_clusters; span, image (3 per particle), rg2 by caller index, pstats eight words, overwritten; each may be null.
void launch_clusters_span(const double4 *pos, const double4 *pos_s, const unsigned *tag_s, int N, const int *cell_off, DBox box, DCells nc,
                          const ClusterLinks &cl, const ClusterSpan &sp, unsigned *label, unsigned *size, unsigned long long *stats,
                          unsigned long long *hist, unsigned nhist, unsigned *span, int *image, double *rg2, unsigned long long *pstats,
                          hipStream_t s, const PairExclusions *ex = nullptr);

}  // namespace pse
