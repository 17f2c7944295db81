// Chain conformations (pse_molecules_compute, include/pse_amd.h): the gyration tensor and the end-to-end vector of every molecule of a
// bond topology, unfolded along its own bonds.  Kernels only; the object and its entry points are in pse_objects.hip.
#include "pse_molecules.h"

namespace pse {

static_assert(2 * MOL_BUF * sizeof(double) == 57344 && MOL_COLS * MOL_HALF <= 2 * MOL_BUF && 6 * MOL_TILE <= 2 * MOL_BUF,
              "56 KB of LDS: two buffers of the pointer jumping, reused by the six member sums and by the MOL_COLS molecule sums");

// k_mol_tile: one workgroup of MOL_TILE lanes per tile, one lane per member (pse_molecules.h documents the arrays).
//  1., 2. the unfolding of mol_unfold (pse_molecules.h), which the pair pass of pse_molpairs.hip shares;
//  3. su = sum of u and then sum of v (x) v, v = u - su / m, by member_tree; the lane of the root writes the molecule's row, counts
//     its Rg and |R|, and keeps the MOL_COLS terms of its type's sums;
//  4. per type, the same halving tree over the molecules of the tile (a molecule of another type enters as +0.0), one partial row
//     per (tile, type) into the workspace.
// No floating-point atomics; every sum has an order that the layout alone fixes.
// (eight waves per SIMD: 64 VGPRs, so that two workgroups of sixteen waves share a CU and one's barriers hide behind the other)
__global__ void __launch_bounds__(MOL_TILE, 8)
k_mol_tile(const double4 *__restrict__ pos, DBox box, Molecules mo, double *__restrict__ rows, double4 *__restrict__ unfolded, bool reduce,
           unsigned long long *__restrict__ hist) {
    __shared__ double sh[2 * MOL_BUF];
    const int t = blockIdx.x, l = threadIdx.x;
    const unsigned start = mo.tile_slot[t], cnt = mo.tile_slot[t + 1] - start, tw = mo.tile_word[t];
    const int rounds = (int)(tw & 255u), lgS = (int)((tw >> 8) & 255u), lgM = (int)((tw >> 16) & 255u);
    const MolMember q = mol_unfold(sh, pos, box, mo.word, mo.member, start, cnt, rounds);
    const bool active = q.active;
    const unsigned idx = q.idx;
    const int p = q.p, m = q.m;
    const double rx = q.rx, ry = q.ry, rz = q.rz, ux = q.ux, uy = q.uy, uz = q.uz;
    const bool root = active && p == 0;
    // the ends of a linear molecule, read by the lane of its root before the buffers are reused
    unsigned molid = 0u, info = 0u;
    double Rx = 0.0, Ry = 0.0, Rz = 0.0;
    if (root || (active && unfolded)) molid = mo.mol[start + l];
    if (root) {
        info = mo.info[molid];
        const double *fin = sh + (rounds & 1) * MOL_BUF;
        const int lo = l + (int)(info & 1023u), hi = l + (int)((info >> 10) & 1023u);
        Rx = fin[hi] - fin[lo]; Ry = fin[MOL_TILE + hi] - fin[MOL_TILE + lo]; Rz = fin[2 * MOL_TILE + hi] - fin[2 * MOL_TILE + lo];
    }
    if (active && unfolded) unfolded[idx] = make_double4(rx + ux, ry + uy, rz + uz, (double)molid);
    __syncthreads();
    sh[l] = ux; sh[MOL_TILE + l] = uy; sh[2 * MOL_TILE + l] = uz;
    __syncthreads();
    member_tree<3>(sh, l, active, p, m, lgS);
    const double dm = (double)m;
    const double mx = sh[l - p] / dm, my = sh[MOL_TILE + l - p] / dm, mz = sh[2 * MOL_TILE + l - p] / dm;
    __syncthreads();
    const double vx = ux - mx, vy = uy - my, vz = uz - mz;
    sh[l] = vx * vx; sh[MOL_TILE + l] = vy * vy; sh[2 * MOL_TILE + l] = vz * vz;
    sh[3 * MOL_TILE + l] = vx * vy; sh[4 * MOL_TILE + l] = vx * vz; sh[5 * MOL_TILE + l] = vy * vz;
    __syncthreads();
    member_tree<6>(sh, l, active, p, m, lgS);
    double term[MOL_COLS];
#pragma unroll
    for (int c = 0; c < MOL_COLS; ++c) term[c] = 0.0;
    int type = -1, j = 0;
    if (root) {
        const bool linear = ((info >> 24) & 1u) != 0u;
        type = (int)((info >> 20) & 15u);
        j = (int)(molid - mo.tile_mol[t]);
#pragma unroll
        for (int c = 0; c < 6; ++c) term[c] = sh[c * MOL_TILE + l] / dm;
        const double rg2 = (term[0] + term[1]) + term[2];
        term[6] = rg2 * rg2;
        const double R2 = fma(Rz, Rz, fma(Ry, Ry, Rx * Rx));
        if (linear) {
            term[7] = Rx * Rx; term[8] = Ry * Ry; term[9] = Rz * Rz; term[10] = Rx * Ry; term[11] = Rx * Rz; term[12] = Ry * Rz;
            term[13] = R2 * R2;
        }
        if (rows) {
            double *row = rows + (size_t)molid * MOL_COLS;
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            row[0] = rx + mx; row[1] = ry + my; row[2] = rz + mz;
#pragma unroll
            for (int c = 0; c < 6; ++c) row[3 + c] = term[c];
            row[9] = rg2;
            row[10] = linear ? Rx : nan; row[11] = linear ? Ry : nan; row[12] = linear ? Rz : nan; row[13] = linear ? R2 : nan;
        }
        if (hist) {
            const size_t stride = (size_t)mo.nbins + 1;
            const double x = sqrt(rg2) * mo.f_rg;
            atomicAdd(hist + (size_t)type * stride + (x < (double)mo.nbins ? (int)x : mo.nbins), 1ull);   // (a NaN goes to the last counter)
            if (linear) {
                const double y = sqrt(R2) * mo.f_ree;
                atomicAdd(hist + (size_t)(mo.ntypes + type) * stride + (y < (double)mo.nbins ? (int)y : mo.nbins), 1ull);
            }
        }
    }
    if (!reduce) return;   // (uniform: behind it only the type sums)
    const int nmt = (int)(mo.tile_mol[t + 1] - mo.tile_mol[t]);
    for (int a = 0; a < mo.ntypes; ++a) {
        __syncthreads();   // the member sums, or the last type's, have been read
        if (root) {
#pragma unroll
            for (int c = 0; c < MOL_COLS; ++c) sh[c * MOL_HALF + j] = type == a ? term[c] : 0.0;
        }
        __syncthreads();
        for (int lgs = lgM - 1; lgs >= 0; --lgs) {
            const int s = 1 << lgs;
            for (int e = l; e < MOL_COLS * s; e += MOL_TILE) {
                const int c = e >> lgs, jj = e - (c << lgs);
                if (jj + s < nmt) sh[c * MOL_HALF + jj] += sh[c * MOL_HALF + jj + s];
            }
            __syncthreads();
        }
        if (l < MOL_COLS) mo.part[((size_t)t * mo.ntypes + a) * MOL_COLS + l] = sh[l * MOL_HALF];
    }
}

// k_mol_finish: one wave per column of the ntypes x MOL_COLS sums; a lane adds the tiles lane, lane + 64, ... in ascending order, the
// wave adds its lanes with the xor butterfly: a fixed order.  Writes this call's sums to `sample`, adds them to `sums`.
__global__ void __launch_bounds__(TPB)
k_mol_finish(const double *__restrict__ part, unsigned ntiles, int ncol, double *__restrict__ sums, double *__restrict__ sample) {
    const int q = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= ncol) return;   // (a whole wave)
    double v = 0.0;
    for (unsigned t = lane; t < ntiles; t += 64u) v += part[(size_t)t * ncol + q];
    v = wave_sum(v);
    if (lane == 0) {
        if (sample) sample[q] = v;
        if (sums) sums[q] += v;
    }
}

void launch_mol_finish(const double *part, unsigned ntiles, int ncol, double *sums, double *sample, hipStream_t s) {
    hipLaunchKernelGGL(k_mol_finish, dim3(nblocks(ncol, TPB / 64)), dim3(TPB), 0, s, part, ntiles, ncol, sums, sample);
}

void launch_molecules(const double4 *pos, DBox box, const Molecules &mo, double *rows, double4 *unfolded, double *sums, double *sample,
                      unsigned long long *hist, hipStream_t s) {
    const bool reduce = sums || sample;
    hipLaunchKernelGGL(k_mol_tile, dim3(mo.ntiles), dim3(MOL_TILE), 0, s, pos, box, mo, rows, unfolded, reduce, hist);
    const int ncol = mo.ntypes * MOL_COLS;
    if (reduce) launch_mol_finish(mo.part, mo.ntiles, ncol, sums, sample, s);
}

}  // namespace pse
