// Chain normal modes (pse_chain_modes_compute, pse_chain_modes_correlate; include/pse_amd.h): K linear functionals of every linear
// molecule on the offsets that the conformation pass unfolds, their static second moments per type, and their correlations with
// stored origins.  Kernels only; the object and its entry points are in pse_objects.hip.
#include "pse_molmodes.h"
#include "pse_molecules.h"

namespace pse {

constexpr int MODE_PLANE = MOL_TILE + MOL_TILE / MODE_CHUNK;   // doubles of one padded plane of offsets
constexpr int MODE_LDS_P = 3 * MODE_PLANE;                    // where the three planes of partial sums begin
constexpr int MODE_LDS_TAB = MODE_LDS_P + 3 * MOL_TILE;       // where the chunk table begins (MOL_HALF unsigned)
static_assert(MODE_LDS_TAB + MOL_HALF / 2 <= 2 * MOL_BUF,
              "56 KB of LDS: the offsets in rank order (three padded planes), three planes of partial sums and the chunk table");
static_assert(MODE_CHUNK >= 2 && MOL_TILE % MODE_CHUNK == 0 && MOL_TILE / MODE_CHUNK <= 64,
              "a molecule has at most 64 chunks (6 bits of a table entry) and never more chunks than half its members");

// the place of the offset of tile slot r in a padded plane: one double of padding behind every MODE_CHUNK, so that lanes that read
// the same rank of consecutive chunks (17 doubles apart) fall on different banks
__device__ __forceinline__ int mode_pad(int r) { return r + r / MODE_CHUNK; }

// k_modes_tile: one workgroup of MOL_TILE lanes per tile (pse_molmodes.h documents the arrays).
//  1., 2. the unfolding of mol_unfold (pse_molecules.h): the offsets u have the bits of pse_molecules_compute;
//  3. u goes to LDS as three padded planes in RANK order per molecule; the lane of every MODE_CHUNK-th rank of a linear molecule enters
//     its chunk into the tile's chunk table (the molecule inside the tile | the chunk << 10);
//  4. the K functionals in passes of kp = min(K, MOL_TILE / chunks of the tile) each, so that one pass has at most MOL_TILE items:
//     lane e takes the item (chunk g = e / kp, k = k0 + e % kp) and adds its ranks q in ascending order with one fma each from +0.0:
//     consecutive lanes read consecutive doubles of the transposed weight table, the lanes of one chunk read one u_q (a broadcast);
//  5. the lane of chunk 0 of a (molecule, k) adds the chunks in ascending order from +0.0: X_k, written to the current buffer and to `modes`;
//  6. per (type, k, column) one lane adds X_a X_b over the linear molecules of the tile in ascending order, one fma each from +0.0:
//     one partial row per tile into the workspace.
// No floating-point atomics; every sum has an order that the layout alone fixes.
__global__ void __launch_bounds__(MOL_TILE, 8)
k_modes_tile(const double4 *__restrict__ pos, DBox box, MolModes mm, double *__restrict__ modes, bool reduce) {
    __shared__ double sh[2 * MOL_BUF];
    const int t = blockIdx.x, l = threadIdx.x;
    const unsigned start = mm.tile_slot[t], cnt = mm.tile_slot[t + 1] - start, tw = mm.tile_word[t];
    const int rounds = (int)(tw & 255u), C = (int)(tw >> 16), K = mm.K;
    const unsigned mol0 = mm.tile_mol[t];
    const int nmt = (int)(mm.tile_mol[t + 1] - mol0);
    const MolMember u = mol_unfold(sh, pos, box, mm.word, mm.member, start, cnt, rounds);
    double *UX = sh, *UY = UX + MODE_PLANE, *UZ = UY + MODE_PLANE, *P = sh + MODE_LDS_P;
    unsigned *tab = reinterpret_cast<unsigned *>(sh + MODE_LDS_TAB);
    if (u.active) {   // (behind the last barrier of the unfolding: every lane holds its u)
        const unsigned w = mm.rank[start + l];
        const int s = (int)(w & 1023u), j = (int)(w >> 10), at = mode_pad(l - u.p + s);
        UX[at] = u.ux; UY[at] = u.uy; UZ[at] = u.uz;
        if (s % MODE_CHUNK == 0 && ((mm.mol_word[mol0 + j] >> 24) & 1u) != 0u)
            tab[mm.mol_chunk[mol0 + j] + s / MODE_CHUNK] = (unsigned)j | ((unsigned)(s / MODE_CHUNK) << 10);
    }
    const size_t prow = (size_t)t * mm.ntypes * K * 6;
    if (C == 0) {   // (uniform: a tile without a linear molecule)
        if (reduce) for (int e = l; e < mm.ntypes * K * 6; e += MOL_TILE) mm.part_static[prow + e] = 0.0;
        return;
    }
    __syncthreads();
    const int KP = min(K, MOL_TILE / C);
    for (int k0 = 0; k0 < K; k0 += KP) {
        const int kp = min(KP, K - k0);
        const bool item = l < C * kp;
        int k = 0, c = 0, m = 1;
        unsigned mol = mol0;
        if (item) {
            const int g = l / kp;
            const unsigned e = tab[g];
            k = k0 + (l - g * kp); c = (int)(e >> 10); mol = mol0 + (e & 1023u);
            const unsigned mw = mm.mol_word[mol];
            const int b = (int)(mw & 1023u);
            m = (int)((mw >> 10) & 1023u) + 1;
            const double *__restrict__ wt = mm.weights + mm.mol_wt[mol] + k;
            const int q1 = min((c + 1) * MODE_CHUNK, m);
            double ax = 0.0, ay = 0.0, az = 0.0;
            for (int q = c * MODE_CHUNK; q < q1; ++q) {
                const double w = wt[(size_t)q * K];
                const int at = mode_pad(b + q);
                ax = fma(w, UX[at], ax); ay = fma(w, UY[at], ay); az = fma(w, UZ[at], az);
            }
            P[l] = ax; P[MOL_TILE + l] = ay; P[2 * MOL_TILE + l] = az;
        }
        __syncthreads();
        const bool head = item && c == 0;
        double x = 0.0, y = 0.0, z = 0.0;
        if (head) {
            const int nch = (m + MODE_CHUNK - 1) / MODE_CHUNK;
            for (int cc = 0; cc < nch; ++cc) { x += P[l + cc * kp]; y += P[MOL_TILE + l + cc * kp]; z += P[2 * MOL_TILE + l + cc * kp]; }
        }
        __syncthreads();   // the partial sums have been read
        if (head) {
            const size_t jl = mm.mol_lin[mol], nl = mm.nlin;
            P[l] = x; P[MOL_TILE + l] = y; P[2 * MOL_TILE + l] = z;
            mm.cur[(size_t)(3 * k) * nl + jl] = x; mm.cur[(size_t)(3 * k + 1) * nl + jl] = y; mm.cur[(size_t)(3 * k + 2) * nl + jl] = z;
            if (modes) { double *o = modes + (jl * K + k) * 3; o[0] = x; o[1] = y; o[2] = z; }
        }
        if (!reduce) continue;   // (uniform; the next pass writes P only behind its readers' second barrier)
        __syncthreads();
        for (int e = l; e < mm.ntypes * kp * 6; e += MOL_TILE) {
            const unsigned a = (unsigned)(e / (kp * 6));
            const int rem = e - (int)a * kp * 6, kk = rem / 6, col = rem - kk * 6;
            const int ia = col < 3 ? col : (col == 5 ? 1 : 0), ib = col < 3 ? col : (col == 3 ? 1 : 2);
            double acc = 0.0;
            for (int j = 0; j < nmt; ++j) {
                const unsigned mw = mm.mol_word[mol0 + j];
                if (((mw >> 24) & 1u) == 0u || ((mw >> 20) & 15u) != a) continue;
                const int at = (int)mm.mol_chunk[mol0 + j] * kp + kk;
                acc = fma(P[ia * MOL_TILE + at], P[ib * MOL_TILE + at], acc);
            }
            mm.part_static[prow + ((size_t)a * K + k0 + kk) * 6 + col] = acc;
        }
        __syncthreads();   // the X of this pass have been read
    }
}

// k_modes_corr: one wave per (block of MODE_BLOCK consecutive linear molecules, k).  Lane l holds the molecules l, l + 64, l + 128,
// l + 192 of the block; per pair and type it adds X_a(now) X_b(slot) over those of the type in that order, one fma each from +0.0
// (a lane without one keeps +0.0), the wave adds its lanes with the xor butterfly, and lane 0 writes the nine sums as the partial row
// of (block, pair, type, k).  The type comes from the byte array lin_type; a type that the block does not hold is written as +0.0
// without the butterfly (a branch of the whole wave).
__global__ void __launch_bounds__(TPB)
k_modes_corr(MolModes mm, ModePairs pairs) {
    constexpr int NI = MODE_BLOCK / 64;
    const int W = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63, K = mm.K;
    if (W >= (int)mm.nblocks * K) return;   // (a whole wave)
    const int blk = W / K, k = W - blk * K;
    const size_t nl = mm.nlin, plane = (size_t)(3 * k) * nl, buf = (size_t)3 * K * nl;
    double cx[NI], cy[NI], cz[NI];
    int ty[NI];
    unsigned present = 0u;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const size_t j = (size_t)blk * MODE_BLOCK + i * 64 + lane;
        const bool in = j < nl;
        cx[i] = in ? mm.cur[plane + j] : 0.0; cy[i] = in ? mm.cur[plane + nl + j] : 0.0; cz[i] = in ? mm.cur[plane + 2 * nl + j] : 0.0;
        ty[i] = in ? (int)mm.lin_type[j] : -1;
        if (in) present |= 1u << ty[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) present |= (unsigned)__shfl_xor((int)present, o, 64);
    for (int p = 0; p < pairs.npairs; ++p) {
        const double *__restrict__ org = mm.slots + (size_t)pairs.slot[p] * buf + plane;
        double ox[NI], oy[NI], oz[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const size_t j = (size_t)blk * MODE_BLOCK + i * 64 + lane;
            const bool in = j < nl;
            ox[i] = in ? org[j] : 0.0; oy[i] = in ? org[nl + j] : 0.0; oz[i] = in ? org[2 * nl + j] : 0.0;
        }
        for (int a = 0; a < mm.ntypes; ++a) {
            double *dst = mm.part_corr + ((((size_t)blk * pairs.npairs + p) * mm.ntypes + a) * K + k) * 9;
            if (((present >> a) & 1u) == 0u) {   // (uniform)
                if (lane < 9) dst[lane] = 0.0;
                continue;
            }
            double acc[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) acc[e] = 0.0;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                if (ty[i] != a) continue;
                acc[0] = fma(cx[i], ox[i], acc[0]); acc[1] = fma(cx[i], oy[i], acc[1]); acc[2] = fma(cx[i], oz[i], acc[2]);
                acc[3] = fma(cy[i], ox[i], acc[3]); acc[4] = fma(cy[i], oy[i], acc[4]); acc[5] = fma(cy[i], oz[i], acc[5]);
                acc[6] = fma(cz[i], ox[i], acc[6]); acc[7] = fma(cz[i], oy[i], acc[7]); acc[8] = fma(cz[i], oz[i], acc[8]);
            }
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                const double v = wave_sum(acc[e]);
                if (lane == 0) dst[e] = v;
            }
        }
    }
}

// k_modes_corr_finish: one wave per column of the npairs x ntypes x K x 9 partial sums, by the order rule of k_mol_finish: a lane adds
// the blocks lane, lane + 64, ... in ascending order, the wave adds its lanes with the xor butterfly; lane 0 adds to the row of corr
// that the pair names.
__global__ void __launch_bounds__(TPB)
k_modes_corr_finish(const double *__restrict__ part, unsigned nblk, int ncol, int percorr, ModePairs pairs, double *__restrict__ corr) {
    const int q = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= ncol) return;   // (a whole wave)
    double v = 0.0;
    for (unsigned b = lane; b < nblk; b += 64u) v += part[(size_t)b * ncol + q];
    v = wave_sum(v);
    if (lane == 0) {
        const int p = q / percorr;
        corr[(size_t)pairs.row[p] * percorr + (q - p * percorr)] += v;
    }
}

void launch_chain_modes(const double4 *pos, DBox box, const MolModes &mm, double *modes, double *sums, double *sample, hipStream_t s) {
    const bool reduce = sums || sample;
    hipLaunchKernelGGL(k_modes_tile, dim3(mm.ntiles), dim3(MOL_TILE), 0, s, pos, box, mm, modes, reduce);
    if (reduce) launch_mol_finish(mm.part_static, mm.ntiles, mm.ntypes * mm.K * 6, sums, sample, s);
}

void launch_chain_modes_correlate(const MolModes &mm, const ModePairs &pairs, double *corr, hipStream_t s) {
    const int percorr = mm.ntypes * mm.K * 9, ncol = pairs.npairs * percorr;
    hipLaunchKernelGGL(k_modes_corr, dim3(nblocks((long)mm.nblocks * mm.K, TPB / 64)), dim3(TPB), 0, s, mm, pairs);
    hipLaunchKernelGGL(k_modes_corr_finish, dim3(nblocks(ncol, TPB / 64)), dim3(TPB), 0, s, mm.part_corr, mm.nblocks, ncol, percorr, pairs, corr);
}

}  // namespace pse
