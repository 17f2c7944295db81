// Launch wrapper of the chain-conformation kernels (defined in pse_molecules.hip).  It takes the stream explicitly.
#pragma once
#include <hip/hip_runtime.h>

#include "pse_device.h"

namespace pse {

constexpr int MOL_TILE = 1024;   // members of one tile = lanes of its workgroup (PSE_MOL_TILE)
static_assert(MOL_TILE == 1024, "the packed words of a member hold 10-bit positions");
constexpr int MOL_HALF = MOL_TILE / 2;          // the most molecules of a tile (dimers)
constexpr int MOL_BUF = 3 * MOL_TILE + MOL_HALF;   // doubles of one pointer-jumping buffer: x, y, z and MOL_TILE ancestors (ints)

// chain conformations (pse_molecules_compute): the device arrays of one object, from the layout of pse_host_molecule_rows.  Per member
// slot s (molecule after molecule in breadth-first order, the slots of a tile consecutive): member[s] the caller index; word[s] =
// the slot of its parent inside the tile | its breadth-first position << 10 | (the size of its molecule - 1) << 20; mol[s] the
// molecule number.  Per molecule: info[mol] = the position of its lower end | the position of its higher end << 10 | its type << 20
// | 1 << 24 if it is linear (the ends are 0 otherwise).  Per tile t: tile_slot[t] .. tile_slot[t + 1) its slots, tile_mol[t] ..
// tile_mol[t + 1) its molecules, tile_word[t] = its rounds of pointer jumping | log2 of the power of two >= its largest molecule << 8
// | log2 of the power of two >= its number of molecules << 16.  part: the workspace, one row of MOL_COLS doubles per (tile, type).
// f_rg, f_ree: nbins / rg_max and nbins / ree_max, formed on the host.
struct Molecules {
    const unsigned *member, *word, *mol, *info, *tile_slot, *tile_mol, *tile_word;
    double *part;
    unsigned nmol, ntiles;
    int ntypes, nbins;
    double f_rg, f_ree;
};
// rows (nmol x MOL_COLS), unfolded (caller order), sums and sample (ntypes x MOL_COLS), hist (2 x ntypes x (nbins + 1)): each may be null
void launch_molecules(const double4 *pos, DBox box, const Molecules &mo, double *rows, double4 *unfolded, double *sums, double *sample,
                      unsigned long long *hist, hipStream_t s);

// k_mol_finish (pse_molecules.hip) on any workspace of ntiles rows of ncol doubles: one wave per column adds the tiles in a fixed order,
// writes `sample` and adds to `sums` (each may be null).
void launch_mol_finish(const double *part, unsigned ntiles, int ncol, double *sums, double *sample, hipStream_t s);

#ifdef __HIPCC__
// What one lane of a tile's workgroup knows of its member after the unfolding.
struct MolMember {
    bool active;       // the lane has a member
    unsigned idx;      // its caller index
    int p, m;          // its breadth-first position and the size of its molecule
    double4 r;         // its position as given
    double rx, ry, rz; // the position of its root
    double ux, uy, uz; // its offset from the root
};

// The unfolding that the kernels of a tile share (sh: 2 MOL_BUF doubles of LDS; word and member: the arrays of the slots from `start`,
// cnt of them; rounds: of the tile):
//  1. the lanes gather their positions through the member list, once, into LDS; a lane takes the minimum image of the bond vector to
//     its parent and the position of its root from there;
//  2. pointer jumping between two LDS buffers, one barrier a round: u += u[ancestor], ancestor = ancestor[ancestor].
// Ends behind a barrier with u in the registers and in the buffer sh + (rounds & 1) MOL_BUF, slot by slot.
__device__ __forceinline__ MolMember mol_unfold(double *sh, const double4 *__restrict__ pos, const DBox &box, const unsigned *__restrict__ word,
                                                const unsigned *__restrict__ member, unsigned start, unsigned cnt, int rounds) {
    const int l = threadIdx.x;
    MolMember q;
    q.active = (unsigned)l < cnt;
    q.idx = 0u;
    int par = 0;
    q.p = 0; q.m = 1;
    q.r = make_double4(0.0, 0.0, 0.0, 0.0);
    if (q.active) {
        const unsigned w = word[start + l];
        q.idx = member[start + l];
        par = (int)(w & 1023u); q.p = (int)((w >> 10) & 1023u); q.m = (int)((w >> 20) & 1023u) + 1;
        q.r = pos[q.idx];
    }
    double *b1 = sh + MOL_BUF;
    b1[l] = q.r.x; b1[MOL_TILE + l] = q.r.y; b1[2 * MOL_TILE + l] = q.r.z;
    __syncthreads();
    double ux = 0.0, uy = 0.0, uz = 0.0;
    q.rx = b1[l - q.p]; q.ry = b1[MOL_TILE + l - q.p]; q.rz = b1[2 * MOL_TILE + l - q.p];   // the root's position
    if (q.active && q.p != 0) {
        ux = q.r.x - b1[par]; uy = q.r.y - b1[MOL_TILE + par]; uz = q.r.z - b1[2 * MOL_TILE + par];
        min_image(box, ux, uy, uz);
    }
    __syncthreads();   // (round 0 writes the buffer the positions were in)
    int anc = q.active ? par : l;
    sh[l] = ux; sh[MOL_TILE + l] = uy; sh[2 * MOL_TILE + l] = uz;
    reinterpret_cast<int *>(sh + 3 * MOL_TILE)[l] = anc;
    __syncthreads();
    for (int k = 0; k < rounds; ++k) {
        const double *src = sh + (k & 1) * MOL_BUF;
        double *dst = sh + ((k + 1) & 1) * MOL_BUF;
        ux += src[anc]; uy += src[MOL_TILE + anc]; uz += src[2 * MOL_TILE + anc];
        anc = reinterpret_cast<const int *>(src + 3 * MOL_TILE)[anc];
        dst[l] = ux; dst[MOL_TILE + l] = uy; dst[2 * MOL_TILE + l] = uz;
        reinterpret_cast<int *>(dst + 3 * MOL_TILE)[l] = anc;
        __syncthreads();
    }
    q.ux = ux; q.uy = uy; q.uz = uz;
    return q;
}

// One level-by-level halving tree over the positions p = 0 .. m - 1 of every molecule of the tile at once, on NC arrays of MOL_TILE
// doubles: at stride s (the powers of two below the tile's largest molecule, descending) position p adds position p + s where
// p < s and p + s < m.  The order is a function of m alone; the sum ends at position 0.  Ends behind a barrier.
template <int NC>
__device__ __forceinline__ void member_tree(double *sh, int l, bool active, int p, int m, int lgS) {
    for (int s = (1 << lgS) >> 1; s > 0; s >>= 1) {
        if (active && p < s && p + s < m) {
#pragma unroll
            for (int c = 0; c < NC; ++c) sh[c * MOL_TILE + l] += sh[c * MOL_TILE + l + s];
        }
        __syncthreads();
    }
}
#endif

}  // namespace pse
