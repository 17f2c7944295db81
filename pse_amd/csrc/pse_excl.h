// Pair exclusions as the kernels of the cell-list passes read them (pse_forces.hip, pse_analysis.hip, pse_order.hip): the rows, the lookup and the
// launch helper that instantiates a kernel with and without them.
#pragma once
#include <type_traits>

#include "pse_forces.h"

namespace pse {

// Pair exclusions of the cell-list passes (HOOMD's nlist.reset_exclusions): ExclRows is the device copy of the rows of
// pse_host_exclusion_rows -- a CSR over the first n CALLER-order particle indices, row t the partners excluded from t, sorted
// ascending, without duplicates, every pair in both rows.  The rows are indexed by tags (tag_s), never by sorted-order rows.
struct ExclRows {
    const unsigned *__restrict__ off;   // n + 1
    const unsigned *__restrict__ ent;   // off[n] partners
    unsigned n;
};
constexpr unsigned EXCL_LINEAR = 8;   // rows (or what the bisection leaves of one) up to this length are compared in one batch of loads
// The row bounds [eb, ee) of the particle with tag t: a tag >= n has no exclusions and reads nothing.
__device__ __forceinline__ void excl_row(const ExclRows &ex, unsigned t, unsigned &eb, unsigned &ee) {
    eb = ee = 0u;
    if (t < ex.n) { eb = ex.off[t]; ee = ex.off[t + 1]; }
}
// Is tag tj in the sorted row [eb, ee), eb < ee?  Called for a pair that has passed the distance test, a few per particle, and only
// by a lane whose row is not empty (the caller tests eb < ee before it loads tag_s[j]).  Search: rows are typically the 2-6 partners
// of a chain's 1-2, 1-3 and 1-4 neighbours, so a row of at most EXCL_LINEAR = 8 entries is compared whole: eight 4-byte loads along
// the row, indices past the end clamped to the last entry, issued back to back and waited for once -- one or two cache lines, ONE
// memory latency behind the load of tag_s[j].  (A scan in ascending order with an early exit at the first entry >= tj makes fewer
// loads but waits for each before it decides on the next: three to four latencies in a row per pair, measured 1.40x the plain table
// pass on six-entry rows against 1.28x for this form, docs/HISTORY.md.)  A longer row (a hub, a cross-linker) uses the sorted
// order: it is bisected until at most 8 candidates are left, log2(len / 8) dependent loads, and the same batch finishes -- a row of
// 500 costs 6 loads and a batch instead of 500 loads.  The lanes of a wave diverge here; the pass is bound by the position gathers.
__device__ __forceinline__ bool excl_has(const unsigned *__restrict__ ent, unsigned eb, unsigned ee, unsigned tj) {
    while (ee - eb > EXCL_LINEAR) {   // tj, if present, stays in [eb, ee)
        const unsigned mid = eb + ((ee - eb) >> 1);
        if (ent[mid] <= tj) eb = mid; else ee = mid;
    }
    const unsigned last = ee - 1u;
    bool hit = false;
#pragma unroll
    for (unsigned q = 0; q < EXCL_LINEAR; ++q) hit |= ent[min(eb + q, last)] == tj;
    return hit;
}

// The exclusion flag of a launch as a std::bool_constant: `launch` is instantiated for both.
template <class L>
static void launch_with_excl(const PairExclusions *ex, L &&launch) {
    if (ex) launch(std::true_type{}, ExclRows{ex->row_off, ex->entries, ex->n});
    else launch(std::false_type{}, ExclRows{nullptr, nullptr, 0u});
}

}  // namespace pse
