// Launch wrappers of the intermediate scattering functions (defined in pse_scatter.hip).  They take the stream explicitly.
#pragma once
#include <hip/hip_runtime.h>

#include "pse_analysis.h"

namespace pse {

constexpr int ISF_MAX_PAIRS = 64;   // pairs (slot, row) of one pse_isf_correlate (ISF_MAX_ORIGINS)
constexpr int ISF_UNIT = 256;       // a span of the self pass is a multiple of this many particles

// intermediate scattering functions (pse_isf_sample, pse_isf_store, pse_isf_correlate): the device arrays of one object.  sf: the
// types, the mode plan and the workspace of the structure-factor pass, which computes rho of every sample (pse_analysis.h).  A
// BUFFER is `buf` = 3 n_max + 2 ntypes nk doubles: three planes (s_x, s_y, s_z) of n_max fractional coordinates, indexed by the
// caller-order particle index, then rho (ntypes x nk x 2, (re, im), the caller's order of the modes).  cur: the current buffer;
// slots: norigins buffers, one after another.  part: the workspace of the self pass, one complex number per (span of `span`
// particles, listed pair, type, distinct mode): isf_workspace(n_max, ntypes, nk), sized for ISF_MAX_PAIRS pairs; span =
// isf_span(n_max, ntypes, nk), a multiple of ISF_UNIT, the smallest with which the workspace stays within 256 MB.
struct Scatter {
    StructureFactor sf;
    double *cur, *slots;
    size_t n_max, buf;
    double2 *part;
    int span;
};
// the pairs of one pse_isf_correlate, by value in the kernel arguments: slot[p] the origin, row[p] the row of self and coll
struct ScatterPairs {
    int npairs;
    unsigned char slot[ISF_MAX_PAIRS];
    int row[ISF_MAX_PAIRS];
};
int isf_span(unsigned n_max, int ntypes, int nk);
size_t isf_workspace(unsigned n_max, int ntypes, int nk);   // complex numbers
// s of the N group members into the planes of the current buffer, and rho of the sample into its tail by launch_structure_factor,
// which also adds to static_sums (npt x nk, may be null)
void launch_isf_sample(const double4 *pos, const unsigned *group, int N, DBox box, const Scatter &sc, double *static_sums, hipStream_t s);
// self (nrows x ntypes x nk x 2): the rows that `pairs` names are added to; the group and N of the sample in the current buffer
void launch_isf_self(const Scatter &sc, const unsigned *group, int N, const ScatterPairs &pairs, double *self, hipStream_t s);
// coll (nrows x ntypes x ntypes x nk): the rows that `pairs` names are added to
void launch_isf_coll(const Scatter &sc, const ScatterPairs &pairs, double *coll, hipStream_t s);

}  // namespace pse
