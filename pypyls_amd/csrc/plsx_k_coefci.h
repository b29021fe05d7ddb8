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
// ---------------------------------------------------------------------------
#define CP_KB 32                 // subjects per LDS stage
#define CP_XLD 144               // pitch of the feature stage (doubles)
#define CP_ALD 34                // pitch of the stack stage (doubles)
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
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fb = a.f0 + blockIdx.x * 128;         // (fb + 127 < ldx: both multiples of 128, fb < B <= ldx)
    const int b0 = blockIdx.y * 64;
    const int t = blockIdx.z;
    const int S = a.S;
    // pairs of doubles of a stack row are 16-byte aligned when S is even and the stack itself is
    const bool al2 = (S & 1) == 0 && (reinterpret_cast<size_t>(a.A) & 15) == 0;

    d4 acc[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[r][i] = (d4){0, 0, 0, 0};

    const int xcol = (tid & 63) * 2, xrow = tid >> 6;       // feature stage: row xrow + 4 i, one d2 of the 128 features
    const int seg = tid & 15, rbase = tid >> 4;             // stack stage: bootstrap rbase + 16 i, d2 slot seg of 32 subjects
    d2 rx[8], ra[4];
    auto fetch = [&](int kk) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int s = kk + xrow + 4 * i;
            d2 v = (d2){0, 0};
            if (s < S) v = *reinterpret_cast<const d2*>(a.Xc + (size_t)s * a.ldx + fb + xcol);
            rx[i] = v;
        }
        const int c = kk + seg * 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = b0 + rbase + 16 * i;
            d2 v = (d2){0, 0};
            if (b < a.n) {
                const double* p = a.A + ((size_t)b * a.T + t) * S + c;
                if (c + 1 < S) v = al2 ? *reinterpret_cast<const d2*>(p) : (d2){p[0], p[1]};
                else if (c < S) v = (d2){p[0], 0.0};
            }
            ra[i] = v;
        }
    };
    fetch(0);
    for (int kk = 0; kk < S; kk += CP_KB) {
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<d2*>(&sX[(xrow + 4 * i) * CP_XLD + xcol]) = rx[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<d2*>(&sA[(rbase + 16 * i) * CP_ALD + seg * 2]) = ra[i];
        __syncthreads();
        if (kk + CP_KB < S) fetch(kk + CP_KB);
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
        __syncthreads();
    }
    const int fend = min(a.B, a.f0 + a.fc);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = fb + wave * 32 + r * 16 + (lane >> 4) + 4 * i;
            if (f >= fend) continue;
            double* row = a.out + ((size_t)(f - a.f0) * a.T + t) * a.n;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int b = b0 + nt * 16 + (lane & 15);
                if (b < a.n) row[b] = acc[r][nt][i];
            }
        }
}
