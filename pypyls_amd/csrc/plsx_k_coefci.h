// plsx_k_coefci.h -- percentile intervals of the SIMPLS model coefficients: the feature pass k_coef_prod.
// Included through plsx_kernels.h (which documents the operand layouts and lists the kernel headers in order).  gfx950 only.
#pragma once
#include "plsx_common.h"

// ---------------------------------------------------------------------------
// out[f][t][b] = sum_s Xc[s][f] . A[b][t][s]: every bootstrap's coefficient of every (feature, behaviour) of one
// chunk of features, laid out one contiguous series of n bootstraps per (f, t) -- what the selection kernels
// (k_percentile_sel / k_percentile2) read.  A "TN" product on v_mfma_f64_16x16x4_f64 with M = features, N = the
// bootstraps of one behaviour, K = subjects:
//   * Xc (S, ldx) is read in place, lanes along the feature index (a wave loads one 1 KB row piece per instruction),
//     and staged [k][feature] so that the A fragment of lane l, Xc[k = l >> 4][m = l & 15], is a b64 LDS read whose
//     two 16-lane rows of a 32-lane group fall on different halves of the 64 banks (pitch 144 = 128 + 16 doubles);
//   * the kept stack A [n][T][S] (plsx_simpls_coef_keep) is read along s, 16 threads per 256 B row piece, and staged
//     [bootstrap][k] with k_nt_gemm's pitch of 34 doubles (conflict-free b64 reads of the B fragment);
//   * a block owns 128 features x 64 bootstraps of one behaviour, a wave 32 x 64: two A fragments against four B
//     fragments per k-step, 8 MFMAs per 6 LDS reads (k_nt_gemm<2>'s ratio); the next stage's operands are fetched
//     into registers while the current one is multiplied;
//   * every output entry is one block's full contraction over s in ascending order: no partial tiles, no atomics,
//     the same bits whatever the chunking of the features.  D[m = (l >> 4) + 4 i][n = l & 15]: the 16 lanes of a row
//     store 128 contiguous bytes of a series.
// Grid: x = 128-feature blocks of the chunk (fastest: the blocks in flight share a stack tile), y = 64-bootstrap
// tiles, z = behaviour.
// The tile is shared: k_vip_prod (plsx_k_vip.h) and k_coef_perm_prod (plsx_k_coefperm.h) contract theirs through the
// cp_* pieces below, with their own stack row per resample, their own loop and their own epilogue -- one staging, one
// ascending-s order, so the same bits for the same operands in all three.
// ---------------------------------------------------------------------------
#define CP_KB 32                 // subjects per LDS stage
#define CP_XLD 144               // pitch of the feature stage (doubles)
#define CP_ALD 34                // pitch of the stack stage (doubles)
// The operands of one tile, the same in every thread of the block.
struct CpTile {
    const double* Xc; int ldx;   // centred features (S, ldx)
    int S, n;                    // subjects; resamples of the stack
    int fb, b0;                  // features fb .. fb + 127 (fb + 127 < ldx), resamples b0 .. b0 + 63 (those < n)
    bool al2;                    // cp_aligned of the stack
};
struct CpStage { d2 rx[8], ra[4]; };   // a thread's share of one stage of CP_KB subjects, in registers

// pairs of doubles of a stack row are 16-byte aligned when S is even and the stack itself is
__device__ __forceinline__ bool cp_aligned(const double* stack, int S)
{
    return (S & 1) == 0 && (reinterpret_cast<size_t>(stack) & 15) == 0;
}

// Subjects kk .. kk + CP_KB - 1 into registers, zeros beyond S and n.  Features: row (tid >> 6) + 4 i, one d2 of the
// 128.  Stack: resample (tid >> 4) + 16 i, d2 slot tid & 15 of the 32 subjects; row(b) is the start of resample b's
// S-long stack row.
template <class Row>
__device__ __forceinline__ void cp_fetch(CpStage& g, const CpTile tl, int kk, Row row)
{
    const int tid = threadIdx.x;
    // (the thread's place in a stage as one 32-bit offset, at most 3 ldx + 126; the rows' own addresses stay uniform)
    static_assert(3ull * PLSX_MAX_BPAD + 126 < (1ull << 32), "cp_fetch: the per-thread feature offset is 32 bits");
    const unsigned xoff = (unsigned)(tid >> 6) * (unsigned)tl.ldx + (tid & 63) * 2;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int s = kk + (tid >> 6) + 4 * i;
        d2 v = (d2){0, 0};
        if (s < tl.S) v = *reinterpret_cast<const d2*>(tl.Xc + (size_t)(kk + 4 * i) * tl.ldx + tl.fb + xoff);
        g.rx[i] = v;
    }
    const int c = kk + (tid & 15) * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = tl.b0 + (tid >> 4) + 16 * i;
        d2 v = (d2){0, 0};
        if (b < tl.n) {
            const double* p = row(b) + c;
            if (c + 1 < tl.S) v = tl.al2 ? *reinterpret_cast<const d2*>(p) : (d2){p[0], p[1]};
            else if (c < tl.S) v = (d2){p[0], 0.0};
        }
        g.ra[i] = v;
    }
}

// the registers of cp_fetch into sX [k][feature] and sA [resample][k]
__device__ __forceinline__ void cp_store(const CpStage& g, double* sX, double* sA)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 8; ++i) *reinterpret_cast<d2*>(&sX[((tid >> 6) + 4 * i) * CP_XLD + (tid & 63) * 2]) = g.rx[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<d2*>(&sA[((tid >> 4) + 16 * i) * CP_ALD + (tid & 15) * 2]) = g.ra[i];
}

// acc += the staged CP_KB subjects, s ascending: wave w's features 32 w + 16 r + (0 .. 15) against resamples 16 nt + (0 .. 15)
__device__ __forceinline__ void cp_mma(const double* sX, const double* sA, d4 (&acc)[2][4])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int ks = 0; ks < CP_KB / 4; ++ks) {
        const int kr = ks * 4 + (lane >> 4);
        double fx[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) fx[r] = sX[kr * CP_XLD + wave * 32 + r * 16 + (lane & 15)];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const double fa = sA[(nt * 16 + (lane & 15)) * CP_ALD + kr];
#pragma unroll
            for (int r = 0; r < 2; ++r) acc[r][nt] = mfma_f64(fx[r], fa, acc[r][nt]);
        }
    }
}

// acc += the tile's full contraction over s: the next stage is fetched while the current one is multiplied
template <class Row>
__device__ __forceinline__ void cp_contract(const CpTile tl, Row row, double* sX, double* sA, d4 (&acc)[2][4])
{
    CpStage g;
    cp_fetch(g, tl, 0, row);
    for (int kk = 0; kk < tl.S; kk += CP_KB) {
        cp_store(g, sX, sA);
        __syncthreads();
        if (kk + CP_KB < tl.S) cp_fetch(g, tl, kk + CP_KB, row);
        cp_mma(sX, sA, acc);
        __syncthreads();
    }
}

__device__ __forceinline__ void cp_clear(d4 (&acc)[2][4])
{
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[r][i] = (d4){0, 0, 0, 0};
}

// The feature of a lane's accumulator row acc[r][.][i] (D[m = (l >> 4) + 4 i][n = l & 15]; the resample is
// b0 + 16 nt + (l & 15)), or -1 when it lies beyond fend.
__device__ __forceinline__ int cp_feature(int fb, int fend, int r, int i)
{
    const int f = fb + (threadIdx.x >> 6) * 32 + r * 16 + ((threadIdx.x & 63) >> 4) + 4 * i;
    return f < fend ? f : -1;
}

struct CoefProdArgs {
    const double* Xc; int ldx;   // centred features (S, ldx), ldx a multiple of 128, columns >= B zero or unused
    const double* A;             // kept stack [n][T][S]
    int S, T, n, B;
    int f0, fc;                  // features f0 .. f0 + fc - 1 (f0 a multiple of 128)
    double* out;                 // [fc][T][n]
};

static __global__ __launch_bounds__(256)
void k_coef_prod(CoefProdArgs a)
{
    __shared__ __attribute__((aligned(16))) double sX[CP_KB * CP_XLD];
    __shared__ __attribute__((aligned(16))) double sA[64 * CP_ALD];
    const int lane = threadIdx.x & 63;
    const int fb = a.f0 + blockIdx.x * 128;         // (fb + 127 < ldx: both multiples of 128, fb < B <= ldx)
    const int b0 = blockIdx.y * 64;
    const int t = blockIdx.z;
    const CpTile tl{a.Xc, a.ldx, a.S, a.n, fb, b0, cp_aligned(a.A, a.S)};

    d4 acc[2][4];
    cp_clear(acc);
    cp_contract(tl, [&](int b) { return a.A + ((size_t)b * a.T + t) * a.S; }, sX, sA, acc);
    const int fend = min(a.B, a.f0 + a.fc);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = cp_feature(fb, fend, r, i);
            if (f < 0) continue;
            double* row = a.out + ((size_t)(f - a.f0) * a.T + t) * a.n;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int b = b0 + nt * 16 + (lane & 15);
                if (b < a.n) row[b] = acc[r][nt][i];
            }
        }
}
