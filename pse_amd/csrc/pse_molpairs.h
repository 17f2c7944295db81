// Launch wrapper of the chain-statistics pair pass (defined in pse_molpairs.hip).  It takes the stream explicitly.
#pragma once
#include <hip/hip_runtime.h>

#include "pse_device.h"

namespace pse {

// chain statistics (pse_molecule_pairs_compute): the device arrays of one object, from the layout of pse_host_molecule_rows and the
// ranks of pse_host_chain_order.  Per member slot (as in Molecules, pse_molecules.h): member[s] the caller index, word[s] the packed
// parent, position and size, rank[s] = its rank in its molecule | the number of its molecule inside the tile << 10.  Per molecule:
// mol_word[mol] = its first slot inside the tile | (its size - 1) << 10 | its type << 20 | 1 << 24 if it is linear.  Per tile:
// tile_slot, tile_mol and tile_word as in Molecules.  part_curves: one row of ntypes x ns x MOLPAIR_COLS doubles per tile;
// part_sums: one row of ntypes x MOLPAIR_SUMS doubles per tile.
struct MolPairs {
    const unsigned *member, *word, *rank, *mol_word, *tile_slot, *tile_mol, *tile_word;
    double *part_curves, *part_sums;
    unsigned nmol, ntiles;
    int ntypes, ns;
};
// inv_rh (nmol), curves (ntypes x ns x MOLPAIR_COLS, added to), sums (ntypes x MOLPAIR_SUMS, added to), sample (the same, written):
// each may be null
void launch_molecule_pairs(const double4 *pos, DBox box, const MolPairs &mp, double *inv_rh, double *curves, double *sums, double *sample,
                           hipStream_t s);

}  // namespace pse
