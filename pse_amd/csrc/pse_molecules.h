// Launch wrapper of the chain-conformation kernels (defined in pse_molecules.hip).  It takes the stream explicitly.
#pragma once
#include <hip/hip_runtime.h>

#include "pse_device.h"

namespace pse {

constexpr int MOL_TILE = 1024;   // members of one tile = lanes of its workgroup (PSE_MOL_TILE)

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

}  // namespace pse
