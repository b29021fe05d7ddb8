// plsx_k_weightsci.h -- percentile intervals of the PLS-C x_weights (plsx_boot_keep / plsx_boot_weights_ci): the kept
// rotation operands, the dual weights rebuilt from them, the scale table of the correlation mode and the feature pass
// k_weights_prod.
// Included through plsx_kernels.h (which documents the operand layouts and lists the kernel headers in order).  gfx950 only.
#pragma once
#include "plsx_common.h"
#include "plsx_k_prep.h"
#include "plsx_k_coefci.h"

// ---------------------------------------------------------------------------
// With A_b (T' x S) the cross-product operand of bootstrap b in subject space (k_build_A_behav / k_build_A_mc, dense)
// and M_b (T' x L) the rotation operand the small solver hands to k_urot, W_b = M_b^T A_b (L x S) and
//   U_b[f][l] = sum_g sigma_{b,g}(f) . sum_{s in cell g} W_b[l][s] . Xc[s][f]
// is what plsx_boot_batch adds into usum for bootstrap b.  sigma = 1 in the unscaled modes; in correlation mode it is
// 1 / std (ddof 1) of the feature over the rows the bootstrap draws into cell g, from the raw moments as the
// cross-product epilogues form it (plsx_k_xprod.h, EPI 4), 0 for a cell-constant feature (raw_ss_live).  Rows of a
// cell are contiguous, so "cell g" is a segment of the contraction axis.
// ---------------------------------------------------------------------------

// M_r of the resamples a solver batch just finished, from k_urot's fragment order (mfrag_index) to the caller's dense
// stack [resample][mk][T'].  grid (n_resamples), block 256.
static __global__ __launch_bounds__(256)
void k_keep_M(const double* __restrict__ Mfrag, int nks_t, int LT, int Tp, int mk, double* __restrict__ out)
{
    const int r = blockIdx.x;
    const double* M = Mfrag + (size_t)r * nks_t * LT * 64;
    double* o = out + (size_t)r * mk * Tp;
    for (int idx = threadIdx.x; idx < mk * Tp; idx += blockDim.x) {
        const int l = idx / Tp, t = idx - l * Tp;
        o[idx] = M[mfrag_index(t, l, nks_t, LT)];
    }
}

// W[r][l][i] = sum_t M[r][l][t] . A[r][t][i] (t ascending) from the dense stack M [n][mk][T'] and the dense operands
// A [n][T'][ld]: k_build_Vd's product and layout, with the stack in place of the solver's fragments.
// grid (n_resamples), block 256; dynamic LDS mk * T' doubles.
static __global__ __launch_bounds__(256)
void k_weights_W(const double* __restrict__ Adense, int ld, int S, int Tp, int mk, const double* __restrict__ Mstack,
                 double* __restrict__ W)
{
    extern __shared__ __attribute__((aligned(16))) double sMw[];     // [mk][Tp]
    const int r = blockIdx.x, tid = threadIdx.x;
    const double* M = Mstack + (size_t)r * mk * Tp;
    for (int idx = tid; idx < mk * Tp; idx += blockDim.x) sMw[idx] = M[idx];
    __syncthreads();
    const double* A = Adense + (size_t)r * Tp * ld;
    double* out = W + (size_t)r * mk * S;
    for (int i = tid; i < S; i += blockDim.x)
        for (int l0 = 0; l0 < mk; l0 += 8) {
            double w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int t = 0; t < Tp; ++t) {
                const double a = A[(size_t)t * ld + i];
#pragma unroll
                for (int u = 0; u < 8; ++u) w[u] += a * sMw[min(l0 + u, mk - 1) * Tp + t];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (l0 + u < mk) out[(size_t)(l0 + u) * S + i] = w[u];
        }
}

// cnt[r][s] = how often bootstrap r draws source row s (integer adds; the caller zeroed cnt).  Indices outside
// 0 .. S - 1 are not counted.  grid (n_resamples), block 256.
static __global__ __launch_bounds__(256)
void k_weights_counts(const int* __restrict__ idx, int S, int* __restrict__ cnt)
{
    const int r = blockIdx.x;
    for (int p = threadIdx.x; p < S; p += blockDim.x) {
        const int xi = idx[(size_t)r * S + p];
        if (xi >= 0 && xi < S) atomicAdd(&cnt[(size_t)r * S + xi], 1);
    }
}

// The scale table of one chunk of features: sc[g][f - f0][b] = sigma_{b,g}(f), one thread per feature (lanes along the
// feature index: a wave reads one 512 B row piece of Xc per source row) and WS_NB bootstraps per thread, whose counts
// are uniform loads -- a row of Xc is read once for WS_NB bootstraps.  m1 = sum_s c X, m2 = sum_s c X^2 over the
// cell's rows in ascending order, nn = sum_s c.  grid (ceil(fc / 128), ceil(n / WS_NB)), block 128.
#define WS_NB 16
static __global__ __launch_bounds__(128)
void k_weights_scale(const double* __restrict__ Xc, int ldx, int B, int J, const int* __restrict__ cell_start,
                     const int* __restrict__ cell_len, const int* __restrict__ cnt, int S, int n, int f0, int fc,
                     double* __restrict__ sc)
{
    const int fl = blockIdx.x * 128 + threadIdx.x;
    const int f = f0 + fl;
    const int b0 = blockIdx.y * WS_NB;
    if (fl >= fc || f >= B) return;
    for (int g = 0; g < J; ++g) {
        const int s0 = cell_start[g], s1 = s0 + cell_len[g];
        double m1[WS_NB], m2[WS_NB];
        int nn[WS_NB];
#pragma unroll
        for (int u = 0; u < WS_NB; ++u) { m1[u] = 0.0; m2[u] = 0.0; nn[u] = 0; }
        for (int s = s0; s < s1; ++s) {
            const double x = Xc[(size_t)s * ldx + f];
            const double x2 = x * x;
#pragma unroll
            for (int u = 0; u < WS_NB; ++u) {
                const int b = min(b0 + u, n - 1);
                const int ci = cnt[(size_t)b * S + s];
                const double c = (double)ci;
                nn[u] += ci;
                m1[u] = __builtin_fma(c, x, m1[u]);
                m2[u] = __builtin_fma(c, x2, m2[u]);
            }
        }
        double* o = sc + ((size_t)g * fc + fl) * n;
#pragma unroll
        for (int u = 0; u < WS_NB; ++u) {
            if (b0 + u >= n) continue;
            const double nd = (double)nn[u];
            const double ss = m2[u] - m1[u] * m1[u] / nd;
            const double var = ss / (nd - 1.0);
            o[b0 + u] = (nn[u] > 1 && raw_ss_live(ss, nd, m2[u])) ? sd_rsqrt(var) : 0.0;
        }
    }
}

// ---------------------------------------------------------------------------
// k_weights_prod: out[f - f0][l][b] = U_b[f][l], one contiguous series of n bootstraps per (feature, LV) -- what the
// selection kernels read.  k_coef_prod's tile (cp_fetch / cp_store / cp_mma of plsx_k_coefci.h: M = 128 features, N =
// 64 bootstraps of one LV, K = subjects) with the K loop run cell segment by cell segment:
//   * WP_CELLS (correlation mode, several cells): a segment [s0, s1) is contracted into its own accumulator set,
//     multiplied by sigma[g][f][b] and added to the tile's total: two sets of 32 accumulator doubles a lane, which
//     costs the second block per CU (profiles/weights_ci_resources.txt).  The first stage of a segment starts at s0
//     rounded down to the 4-subject k-step; the subjects below s0 are masked out of the stack's registers and those
//     from s1 on by cp_fetch's own bound (tile.S = s1), so neither Xc nor the stack is padded.
//   * WP_ONE_CELL (correlation mode, one cell: the headline's design): cp_contract over all subjects and sigma as an
//     epilogue multiply -- one accumulator set, the unscaled variant's registers; the bits WP_CELLS gives for J = 1.
//   * WP_UNSCALED (sc == nullptr: mean-centred PLS, covariance mode): cp_contract over all subjects, k_coef_prod's loop.
// Every entry is one block's contraction in a fixed order -- cells ascending, subjects ascending: the same bits run to
// run and whatever the chunking of the features.  No partial tiles, no atomics.
// Grid: x = 128-feature blocks of the chunk, y = 64-bootstrap tiles, z = LV.
// ---------------------------------------------------------------------------
struct WeightsProdArgs {
    const double* Xc; int ldx;   // centred features (S, ldx), ldx a multiple of 128
    const double* W;             // dual weights [n][mk][S] (k_weights_W)
    const double* sc;            // scale table [J][fc][n] of this chunk, or nullptr (unscaled)
    const int* cell_start; const int* cell_len; int J;
    int S, mk, n, B;
    int f0, fc;                  // features f0 .. f0 + fc - 1 (f0 a multiple of 128)
    double* out;                 // [fc][mk][n]
};

// zero what a segment's first stage fetched of the stack below subject s0 (the stage starts at kk <= s0)
__device__ __forceinline__ void wp_mask_low(CpStage& g, int kk, int s0)
{
    const int c = kk + (threadIdx.x & 15) * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (c < s0) g.ra[i].x = 0.0;
        if (c + 1 < s0) g.ra[i].y = 0.0;
    }
}

enum { WP_UNSCALED = 0, WP_ONE_CELL = 1, WP_CELLS = 2 };

template <int MODE>
static __global__ __launch_bounds__(256)
void k_weights_prod(WeightsProdArgs a)
{
    __shared__ __attribute__((aligned(16))) double sX[CP_KB * CP_XLD];
    __shared__ __attribute__((aligned(16))) double sA[64 * CP_ALD];
    const int lane = threadIdx.x & 63;
    const int fb = a.f0 + blockIdx.x * 128;         // (fb + 127 < ldx: both multiples of 128, fb < B <= ldx)
    const int b0 = blockIdx.y * 64;
    const int l = blockIdx.z;
    const bool al2 = cp_aligned(a.W, a.S);
    const auto row = [&](int b) { return a.W + ((size_t)b * a.mk + l) * a.S; };
    const int fend = min(a.B, a.f0 + a.fc);

    d4 acc[2][4];
    cp_clear(acc);
    if constexpr (MODE != WP_CELLS) {
        cp_contract(CpTile{a.Xc, a.ldx, a.S, a.n, fb, b0, al2}, row, sX, sA, acc);
    } else {
        for (int g = 0; g < a.J; ++g) {
            const int s0 = a.cell_start[g], s1 = s0 + a.cell_len[g];
            const CpTile tl{a.Xc, a.ldx, s1, a.n, fb, b0, al2};
            d4 seg[2][4];
            cp_clear(seg);
            CpStage st;
            const int kk0 = s0 & ~3;
            cp_fetch(st, tl, kk0, row);
            wp_mask_low(st, kk0, s0);
            for (int kk = kk0; kk < s1; kk += CP_KB) {
                cp_store(st, sX, sA);
                __syncthreads();
                if (kk + CP_KB < s1) cp_fetch(st, tl, kk + CP_KB, row);
                cp_mma(sX, sA, seg);
                __syncthreads();
            }
            const double* scg = a.sc + (size_t)g * a.fc * a.n;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int f = cp_feature(fb, fend, r, i);
                    if (f < 0) continue;
                    const double* srow = scg + (size_t)(f - a.f0) * a.n;
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        const int b = b0 + nt * 16 + (lane & 15);
                        if (b < a.n) acc[r][nt][i] = __builtin_fma(srow[b], seg[r][nt][i], acc[r][nt][i]);
                    }
                }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = cp_feature(fb, fend, r, i);
            if (f < 0) continue;
            double* orow = a.out + ((size_t)(f - a.f0) * a.mk + l) * a.n;
            const double* srow = MODE == WP_ONE_CELL ? a.sc + (size_t)(f - a.f0) * a.n : nullptr;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int b = b0 + nt * 16 + (lane & 15);
                if (b < a.n) orow[b] = MODE == WP_ONE_CELL ? srow[b] * acc[r][nt][i] : acc[r][nt][i];
            }
        }
}
