// Launch wrappers of the chain normal-mode passes (defined in pse_molmodes.hip).  They take the stream explicitly.
#pragma once
#include <hip/hip_runtime.h>

#include "pse_device.h"

namespace pse {

constexpr int MODE_CHUNK = 16;       // ranks of one chunk of the projection: one lane adds the terms of one (molecule, k, chunk)
constexpr int MODE_BLOCK = 256;      // linear molecules of one wave of the correlation pass: four per lane
constexpr int MODE_MAX_PAIRS = 64;   // pairs (slot, row) of one pse_chain_modes_correlate (MSD_MAX_ORIGINS)

// chain normal modes (pse_chain_modes_compute): the device arrays of one object, from the layout of pse_host_molecule_rows and the
// ranks of pse_host_chain_order.  Per member slot (as in MolPairs, pse_molpairs.h): member[s] the caller index, word[s] the packed
// parent, position and size, rank[s] = its rank in its molecule | the number of its molecule inside the tile << 10.  Per molecule:
// mol_word[mol] = its first slot inside the tile | (its size - 1) << 10 | its type << 20 | 1 << 24 if it is linear;
// mol_chunk[mol] = the number of the first chunk of a linear molecule among the chunks of its tile's linear molecules (a molecule of
// m members has ceil(m / MODE_CHUNK) of them); mol_lin[mol] = its number j among the linear molecules; mol_wt[mol] = where the weight
// table of its size begins in `weights`.  weights: per size a table of m x K doubles, TRANSPOSED against the caller's: entry
// q K + k is w_{k,q}, so that lanes with consecutive k read consecutive doubles.  Per tile: tile_slot and tile_mol as in Molecules,
// tile_word[t] = its rounds of pointer jumping | log2 of the power of two >= its largest molecule << 8 | the chunks of its linear
// molecules << 16 (at most MOL_TILE / 2).  lin_type: one byte per linear molecule.  cur: the current buffer, 3 K planes of nlin
// doubles, plane 3 k + axis; slots: norigins such buffers, one after another.  part_static: one row of ntypes x K x 6 doubles per
// tile; part_corr: one row of up to MODE_MAX_PAIRS x ntypes x K x 9 doubles per block of MODE_BLOCK linear molecules.
struct MolModes {
    const unsigned *member, *word, *rank, *mol_word, *mol_chunk, *mol_lin, *mol_wt, *tile_slot, *tile_mol, *tile_word;
    const unsigned char *lin_type;
    const double *weights;
    double *cur, *slots, *part_static, *part_corr;
    unsigned nmol, ntiles, nlin, nblocks;
    int ntypes, K;
};
// the pairs of one pse_chain_modes_correlate, by value in the kernel arguments: slot[p] the origin, row[p] the row of corr
struct ModePairs {
    int npairs;
    unsigned char slot[MODE_MAX_PAIRS];
    int row[MODE_MAX_PAIRS];
};
// modes (nlin x K x 3, written), sums (ntypes x K x 6, added to), sample (the same, written): each may be null; mm.cur is always written
void launch_chain_modes(const double4 *pos, DBox box, const MolModes &mm, double *modes, double *sums, double *sample, hipStream_t s);
// corr (nrows x ntypes x K x 9): the rows that `pairs` names are added to
void launch_chain_modes_correlate(const MolModes &mm, const ModePairs &pairs, double *corr, hipStream_t s);

}  // namespace pse
