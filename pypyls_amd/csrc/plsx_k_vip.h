// plsx_k_vip.h -- VIP scores of the SIMPLS resamples: the feature pass of the bootstraps k_vip_prod and the moments of its
// series; the feature pass of the permutation test k_vip_perm_prod (counts and maxima, no score stored), k_vip_perm_count.
// Included through plsx_kernels.h (which documents the operand layouts and lists the kernel headers in order).  gfx950 only.
#pragma once
#include "plsx_common.h"
#include "plsx_k_coefci.h"

// ---------------------------------------------------------------------------
// out[f][b] = sqrt(B . sum_a (sum_s Xc[s][f] . G[b][a][s])^2): every bootstrap's VIP of every feature of one chunk,
// one contiguous series of n bootstraps per feature -- what the selection kernels and k_vip_moments read.  G is the
// kept stack of plsx_simpls_vip_keep: row a of bootstrap b is the dual weight of component a in subject space, scaled
// by sqrt(ssq_a / (|w_a|^2 sum ssq)), so that the contraction of a row is the share of component a in VIP_b[f]^2 / B.
// The square root of a sum of squares over the components is no quadratic form of the stack: the block contracts
// k_coef_prod's tile (the cp_* pieces of plsx_k_coefci.h, which describes it) once per component, in one loop of its own:
//   * per component the accumulator tile (32 doubles per lane) takes the full contraction over s in ascending order;
//     it is then squared into a second register tile (32 more doubles per lane) and cleared;
//   * the first stage of the next component is fetched while the last stage of the current one is multiplied;
//   * after the last component sqrt(B . sum) goes out.  Every entry is one block's work, ascending s inside ascending
//     a: no partial tiles, no atomics, the same bits run to run and whatever the chunking of the features.
// Grid: x = 128-feature blocks of the chunk (fastest: the blocks in flight share a stack tile), y = 64-bootstrap
// tiles.  No z.
// ---------------------------------------------------------------------------
struct VipProdArgs {
    const double* Xc; int ldx;   // centred features (S, ldx), ldx a multiple of 128, columns >= B zero or unused
    const double* G;             // kept stack [n][c][S]
    int S, c, n, B;
    int f0, fc;                  // features f0 .. f0 + fc - 1 (f0 a multiple of 128)
    double* out;                 // [fc][n]
};

static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_vip_prod(VipProdArgs a)
{
    __shared__ __attribute__((aligned(16))) double sX[CP_KB * CP_XLD];
    __shared__ __attribute__((aligned(16))) double sA[64 * CP_ALD];
    const int lane = threadIdx.x & 63;
    const int fb = a.f0 + blockIdx.x * 128;         // (fb + 127 < ldx: both multiples of 128, fb < B <= ldx)
    const int b0 = blockIdx.y * 64;
    const int S = a.S, nc = a.c;
    const CpTile tl{a.Xc, a.ldx, S, a.n, fb, b0, cp_aligned(a.G, S)};
    auto row = [&](int comp) { return [&a, comp](int b) { return a.G + ((size_t)b * a.c + comp) * a.S; }; };

    d4 acc[2][4], sq[2][4];
    cp_clear(acc);
    cp_clear(sq);
    CpStage g;
    cp_fetch(g, tl, 0, row(0));
    // one loop over the (component, stage) pairs: a single fetch site, whose next pair is the next stage of the
    // component or the first stage of the next one
    int comp = 0, kk = 0;
    while (comp < nc) {
        cp_store(g, sX, sA);
        __syncthreads();
        const bool last = kk + CP_KB >= S;
        const int ncomp = last ? comp + 1 : comp, nkk = last ? 0 : kk + CP_KB;
        if (ncomp < nc) cp_fetch(g, tl, nkk, row(ncomp));
        cp_mma(sX, sA, acc);
        __syncthreads();
        if (last) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) sq[r][nt][i] += acc[r][nt][i] * acc[r][nt][i];
            cp_clear(acc);
        }
        comp = ncomp; kk = nkk;
    }
    const int fend = min(a.B, a.f0 + a.fc);
    const double nfeat = (double)a.B;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = cp_feature(fb, fend, r, i);
            if (f < 0) continue;
            double* row_out = a.out + (size_t)(f - a.f0) * a.n;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int b = b0 + nt * 16 + (lane & 15);
                if (b < a.n) row_out[b] = sqrt(nfeat * sq[r][nt][i]);
            }
        }
}

// ---------------------------------------------------------------------------
// The test statistics of one piece of n permutations (or any stack G [n][c][S]) against the observed VIP scores,
// without storing a score.  v[f][b] = sqrt(B . sum_a (sum_s Xc[s][f] . G[b][a][s])^2) is k_vip_prod's value through
// k_vip_prod's own loop over the (component, stage) pairs -- the same pieces, ascending s inside ascending a, so the same
// bits -- but a block owns 128 features and walks a run of `tpb` consecutive 64-permutation tiles of the piece, as
// k_coef_perm_prod walks all of them.  (The whole piece per block leaves ceil(B / 128) blocks: 5 on the chip at B = 600,
// and at B = 100 000 a second round of 782 blocks that fills half of it; the host picks tpb so that the grid is many
// rounds deep, plsx_simpls_api.hip.)  The loop runs over the (tile, component, stage) triples with a single fetch site:
// the first stage of the next tile is fetched under the last multiply of the current one.  Its lanes keep, per row of
// their accumulators (cp_feature: 8 rows per lane), the observed score and an integer count.  After the last component
// of a tile:
//   * count += (v >= observed) for the tile's valid (f, b) -- one-sided: VIP is non-negative and large means important;
//   * the tile's per-permutation maximum over the block's 128 features: over the lane's 8 rows in registers, over the
//     four row groups of a wave with __shfl_xor 16 / 32, over the four waves through LDS; stored to the partial
//     pmax[feature block][b] (a maximum has no order: any grouping gives the same bits).  Rows f >= fend enter as 0,
//     the identity of the chain; a NaN score (a degenerate fit: 0 / 0 in k_sd_vip) compares false and is dropped by
//     fmax, so such a permutation counts nowhere and leaves its maximum at 0 -- below every real fit's, which is >= 1
//     since sum_f v^2 = B.
// After the block's last tile the counts of a row are summed over its 16 lanes and stored to pcount[run][f] by this
// block alone: every (run, f) has one owner, no atomics; k_vip_perm_count adds the runs of a feature to count[f].
// Integers: the sum has no order either.  Grid: x = 128-feature blocks of the chunk (fastest: the blocks in flight
// share a stack tile), y = runs of tpb tiles.
// ---------------------------------------------------------------------------
struct VipPermArgs {
    const double* Xc; int ldx;   // centred features (S, ldx), ldx a multiple of 128, columns >= B zero or unused
    const double* G;             // stack [n][c][S]
    int S, c, n, B;
    int f0, fc;                  // features f0 .. f0 + fc - 1 (f0 a multiple of 128)
    const double* obs;           // (B,) observed VIP scores
    int tpb;                     // 64-permutation tiles per block: block y owns permutations 64 tpb y .. 64 tpb (y + 1) - 1 (those < n)
    int* pcount;                 // [runs][ldx] = #{b of the run : v[f][b] >= obs[f]}, features of the chunk
    double* pmax;                // [feature blocks of the chunk][n]
};

static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_vip_perm_prod(VipPermArgs a)
{
    __shared__ __attribute__((aligned(16))) double sX[CP_KB * CP_XLD];
    __shared__ __attribute__((aligned(16))) double sA[64 * CP_ALD];
    __shared__ double sM[4 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fb = a.f0 + blockIdx.x * 128;         // (fb + 127 < ldx: both multiples of 128, fb < B <= ldx)
    const int fend = min(a.B, a.f0 + a.fc);
    const int S = a.S, nc = a.c;
    const int bfirst = blockIdx.y * a.tpb * 64, n = min(a.n, bfirst + a.tpb * 64);   // the run's permutations bfirst .. n - 1
    const bool al2 = cp_aligned(a.G, S);
    const double nfeat = (double)a.B;
    auto tile = [&](int b0) { return CpTile{a.Xc, a.ldx, S, n, fb, b0, al2}; };   // (n: nothing beyond the run is fetched)
    auto row = [&](int comp) { return [&a, comp](int b) { return a.G + ((size_t)b * a.c + comp) * a.S; }; };

    // the lane's 8 rows: observed score, whether the row is a feature of the chunk, count
    double ob[2][4];
    bool live[2][4];
    int cnt[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = cp_feature(fb, fend, r, i);
            live[r][i] = f >= 0;
            ob[r][i] = f >= 0 ? a.obs[f] : 0.0;
            cnt[r][i] = 0;
        }

    double* pm = a.pmax + (size_t)blockIdx.x * a.n;
    d4 acc[2][4], sq[2][4];
    cp_clear(acc);
    cp_clear(sq);
    CpStage g;
    cp_fetch(g, tile(bfirst), 0, row(0));
    int b0 = bfirst, comp = 0, kk = 0;
    while (b0 < n) {
        cp_store(g, sX, sA);
        __syncthreads();
        const bool last = kk + CP_KB >= S;                    // the component's last stage
        const bool done = last && comp + 1 == nc;             // ... and the tile's
        const int nb0 = done ? b0 + 64 : b0, ncomp = done ? 0 : (last ? comp + 1 : comp), nkk = last ? 0 : kk + CP_KB;
        if (nb0 < n) cp_fetch(g, tile(nb0), nkk, row(ncomp));
        cp_mma(sX, sA, acc);
        __syncthreads();
        if (last) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) sq[r][nt][i] += acc[r][nt][i] * acc[r][nt][i];
            cp_clear(acc);
        }
        if (done) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const bool bok = b0 + nt * 16 + (lane & 15) < n;
                double m = 0.0;
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const double v = sqrt(nfeat * sq[r][nt][i]);
                        cnt[r][i] += (bok && live[r][i] && v >= ob[r][i]) ? 1 : 0;
                        m = fmax(m, live[r][i] ? v : 0.0);
                    }
                m = fmax(m, __shfl_xor(m, 16));
                m = fmax(m, __shfl_xor(m, 32));
                if (lane < 16) sM[wave * 64 + nt * 16 + lane] = m;
            }
            cp_clear(sq);
            // (sM was last read before the barriers of this tile's stages: at least one, S >= 1 and c >= 1)
            __syncthreads();
            if (tid < 64 && b0 + tid < n)
                pm[b0 + tid] = fmax(fmax(sM[tid], sM[64 + tid]), fmax(sM[128 + tid], sM[192 + tid]));
        }
        b0 = nb0; comp = ncomp; kk = nkk;
    }
    // the counts of a row over its 16 lanes; one owner per (run, feature)
    int* pc = a.pcount + (size_t)blockIdx.y * a.ldx;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int c = cnt[r][i];
            c += __shfl_xor(c, 1);
            c += __shfl_xor(c, 2);
            c += __shfl_xor(c, 4);
            c += __shfl_xor(c, 8);
            const int f = cp_feature(fb, fend, r, i);
            if ((lane & 15) == 0 && f >= 0) pc[f] = c;
        }
}

// count[f] += sum over the runs of pcount[run][f], features f0 .. fend - 1 of a chunk.  One thread per feature.
static __global__ __launch_bounds__(256)
void k_vip_perm_count(const int* __restrict__ pcount, int ldx, int runs, int f0, int fend, int* __restrict__ count)
{
    const int f = f0 + blockIdx.x * 256 + threadIdx.x;
    if (f >= fend) return;
    int c = 0;
    for (int y = 0; y < runs; ++y) c += pcount[(size_t)y * ldx + f];
    count[f] += c;
}

// ---------------------------------------------------------------------------
// sd[series] = sqrt(sum_b (v_b - mean)^2 / (n - 1)) of nseries contiguous series of n values -- np.std(ddof = 1); n = 1
// gives 0 / 0 = NaN as numpy does.  Two passes over a series that is in memory anyway: the mean first, then the
// squared deviations from it (no cancellation of large sums).  One block per series; a thread adds its values b = tid,
// tid + 256, ... in ascending order, the 64 lanes of a wave are folded by xor shuffles and the four wave sums are
// added in wave order: one fixed order, the same bits run to run and whatever the chunking.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double vip_block_sum(double v, double* red)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    __syncthreads();                                   // (red may still be read from the call before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

static __global__ __launch_bounds__(256)
void k_vip_moments(const double* __restrict__ data, int n, double* __restrict__ sd)
{
    __shared__ double red[4];
    const double* v = data + (size_t)blockIdx.x * n;
    double s = 0.0;
    for (int b = threadIdx.x; b < n; b += 256) s += v[b];
    const double mean = vip_block_sum(s, red) / n;
    double q = 0.0;
    for (int b = threadIdx.x; b < n; b += 256) {
        const double d = v[b] - mean;
        q += d * d;
    }
    q = vip_block_sum(q, red);
    if (threadIdx.x == 0) sd[blockIdx.x] = sqrt(q / (double)(n - 1));
}
