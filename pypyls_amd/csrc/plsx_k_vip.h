// plsx_k_vip.h -- VIP scores of the SIMPLS bootstraps: the feature pass k_vip_prod and the moments of its series.
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
