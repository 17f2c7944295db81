// Chain statistics (pse_molecule_pairs_compute, include/pse_amd.h): the sums over the pairs of one molecule's members -- 1/Rh of every
// molecule, the internal-distance curve and the bond-vector correlation of the linear ones -- on the offsets that the conformation
// pass unfolds.  Kernels only; the object and its entry points are in pse_objects.hip.
#include "pse_molpairs.h"
#include "pse_molecules.h"

namespace pse {

static_assert(7 * MOL_TILE <= 2 * MOL_BUF, "56 KB of LDS: the offsets and the bond vectors in rank order (six planes) and one plane of sums");

// k_molpair_tile: one workgroup of MOL_TILE lanes per tile, one lane per member (pse_molpairs.h documents the arrays).
//  1., 2. the unfolding of mol_unfold (pse_molecules.h): the offsets u have the bits of pse_molecules_compute;
//  3. u goes to LDS as three planes in RANK order per molecule, the bond vectors b_q = u_{q + 1} - u_q as three more;
//  4. the lane of rank q takes the separation s = q and walks c = 0 .. m - 1 - s in ascending order: consecutive lanes read consecutive
//     doubles u[c + s], u[c] is a broadcast.  H(s) += 1 / sqrt(r2) where r2 != 0; for a linear molecule and s < ns, D(s) += r2 and
//     C(s) += b_c . b_{c + s} (c <= m - 2 - s).  The lane of rank 0 finds r2 == 0 every time: H(0) = D(0) = +0.0, C(0) = D(1);
//  5. the sum of H(s) over the ranks by member_tree; the lane of the root writes 2 H / m^2;
//  6. per (type, s, column) one lane adds the linear molecules of the tile in ascending order, per (type, column of the sums) one lane
//     adds 1/Rh and its square over all molecules of the tile in ascending order: one partial row per tile into the workspaces.
// No floating-point atomics; every sum has an order that the layout alone fixes.
__global__ void __launch_bounds__(MOL_TILE, 8)
k_molpair_tile(const double4 *__restrict__ pos, DBox box, MolPairs mp, double *__restrict__ inv_rh, bool curves, bool reduce) {
    __shared__ double sh[2 * MOL_BUF];
    const int t = blockIdx.x, l = threadIdx.x;
    const unsigned start = mp.tile_slot[t], cnt = mp.tile_slot[t + 1] - start, tw = mp.tile_word[t];
    const int rounds = (int)(tw & 255u), lgS = (int)((tw >> 8) & 255u);
    const unsigned mol0 = mp.tile_mol[t];
    const int nmt = (int)(mp.tile_mol[t + 1] - mol0);
    const MolMember q = mol_unfold(sh, pos, box, mp.word, mp.member, start, cnt, rounds);
    const bool active = q.active;
    const int p = q.p, m = q.m, base = l - p;
    int s = 0, j = 0;
    bool linear = false;
    if (active) {
        const unsigned w = mp.rank[start + l];
        s = (int)(w & 1023u); j = (int)(w >> 10);
        linear = ((mp.mol_word[mol0 + j] >> 24) & 1u) != 0u;
    }
    double *X = sh + base, *Y = X + MOL_TILE, *Z = Y + MOL_TILE, *BX = Z + MOL_TILE, *BY = BX + MOL_TILE, *BZ = BY + MOL_TILE;
    if (active) { X[s] = q.ux; Y[s] = q.uy; Z[s] = q.uz; }   // (behind the last barrier of the unfolding: every lane holds its u)
    __syncthreads();
    if (active && s < m - 1) { BX[s] = X[s + 1] - X[s]; BY[s] = Y[s + 1] - Y[s]; BZ[s] = Z[s + 1] - Z[s]; }
    __syncthreads();
    double H = 0.0, D = 0.0, C = 0.0;
    if (active) {
        const bool cv = curves && linear && s < mp.ns;
        const int last = m - 1 - s;
        for (int c = 0; c <= last; ++c) {
            const double dx = X[c + s] - X[c], dy = Y[c + s] - Y[c], dz = Z[c + s] - Z[c];
            const double r2 = fma(dz, dz, fma(dy, dy, dx * dx));
            if (r2 != 0.0) H += 1.0 / sqrt(r2);
            if (cv) {
                D += r2;
                if (c < last) C += fma(BZ[c], BZ[c + s], fma(BY[c], BY[c + s], BX[c] * BX[c + s]));
            }
        }
    }
    __syncthreads();   // the planes have been read
    double *HP = sh + 6 * MOL_TILE, *IR = sh + 3 * MOL_TILE;
    if (active) { X[s] = D; Y[s] = C; HP[base + s] = H; }
    __syncthreads();
    member_tree<1>(HP, l, active, p, m, lgS);
    if (active && p == 0) {
        const double dm = (double)m, v = 2.0 * HP[l] / (dm * dm);
        if (inv_rh) inv_rh[mol0 + j] = v;
        IR[j] = v;
    }
    if (!curves && !reduce) return;   // (uniform)
    __syncthreads();
    if (reduce && l < mp.ntypes * MOLPAIR_SUMS) {
        const unsigned a = (unsigned)(l / MOLPAIR_SUMS);
        const bool square = (l % MOLPAIR_SUMS) != 0;
        double acc = 0.0;
        for (int k = 0; k < nmt; ++k) {
            if (((mp.mol_word[mol0 + k] >> 20) & 15u) != a) continue;
            const double v = IR[k];
            acc += square ? __dmul_rn(v, v) : v;
        }
        mp.part_sums[(size_t)t * mp.ntypes * MOLPAIR_SUMS + l] = acc;
    }
    if (curves) {
        const int ncol = mp.ntypes * mp.ns * MOLPAIR_COLS;
        for (int e = l; e < ncol; e += MOL_TILE) {
            const unsigned a = (unsigned)(e / (mp.ns * MOLPAIR_COLS));
            const int rem = e - (int)a * mp.ns * MOLPAIR_COLS, sep = rem / MOLPAIR_COLS, col = rem - sep * MOLPAIR_COLS;
            double acc = 0.0;
            if (sep < (1 << lgS)) {   // (no molecule of the tile is larger)
                for (int k = 0; k < nmt; ++k) {
                    const unsigned w = mp.mol_word[mol0 + k];
                    if (((w >> 24) & 1u) == 0u || ((w >> 20) & 15u) != a || sep > (int)((w >> 10) & 1023u)) continue;
                    acc += sh[col * MOL_TILE + (int)(w & 1023u) + sep];
                }
            }
            mp.part_curves[(size_t)t * ncol + e] = acc;
        }
    }
}

void launch_molecule_pairs(const double4 *pos, DBox box, const MolPairs &mp, double *inv_rh, double *curves, double *sums, double *sample,
                           hipStream_t s) {
    const bool reduce = sums || sample;
    hipLaunchKernelGGL(k_molpair_tile, dim3(mp.ntiles), dim3(MOL_TILE), 0, s, pos, box, mp, inv_rh, curves != nullptr, reduce);
    if (curves) launch_mol_finish(mp.part_curves, mp.ntiles, mp.ntypes * mp.ns * MOLPAIR_COLS, curves, nullptr, s);
    if (reduce) launch_mol_finish(mp.part_sums, mp.ntiles, mp.ntypes * MOLPAIR_SUMS, sums, sample, s);
}

}  // namespace pse
