// plsx_k_coefperm.h -- permutation test of the SIMPLS model coefficients: the feature pass k_coef_perm_prod, the
// reduction of its per-block maxima (k_coef_perm_max), the column scale of the bound features (k_col_sd).
// Included through plsx_kernels.h (which documents the operand layouts and lists the kernel headers in order).  gfx950 only.
#pragma once
#include "plsx_common.h"
#include "plsx_k_coefci.h"

// ---------------------------------------------------------------------------
// sd[f] = sqrt(sum_s Xc[s][f]^2 / (nx - 1)): the standard deviation of every bound, centred feature over the nx usable
// rows (masked rows are bound as zeros).  One thread per feature, s ascending: one fixed order.  Columns B .. ldx - 1
// get 0.
// ---------------------------------------------------------------------------
static __global__ __launch_bounds__(256)
void k_col_sd(const double* __restrict__ Xc, int ldx, int S, int B, double nx, double* __restrict__ sd)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= ldx) return;
    double s = 0.0;
    if (f < B)
        for (int r = 0; r < S; ++r) {
            const double x = Xc[(size_t)r * ldx + f];
            s += x * x;
        }
    sd[f] = f < B ? sqrt(s / (nx - 1.0)) : 0.0;
}

// ---------------------------------------------------------------------------
// The test statistics of one piece of n permutations (or any stack A [n][T][S]) against the observed coefficients,
// without storing a product.  coef_b[f][t] = sum_s Xc[s][f] . A[b][t][s] is k_coef_prod's product through k_coef_prod's
// own contraction (cp_contract of plsx_k_coefci.h, which describes the tile), so the same bits -- but a block owns 128
// features of ONE behaviour and walks ALL the 64-permutation tiles of the piece.  Its lanes keep, per row of their
// accumulators (cp_feature: 8 rows per lane), the scale s_f, the observed statistic s_f |obs[f][t]| and an integer
// count.  After each tile:
//   * v = s_f |coef_b[f][t]|; count += (v >= observed) for the tile's valid (f, b);
//   * the tile's per-permutation maximum over the block's 128 features: over the lane's 8 rows in registers, over the
//     four row groups of a wave with __shfl_xor 16 / 32, over the four waves through LDS; stored to the partial
//     pmax[feature block][t][b] (a maximum has no order: any grouping gives the same bits).
// After the last tile the counts of a row are summed over its 16 lanes and added to count[f][t] by this block alone:
// every (f, t) has one owner, no atomics.  Grid: x = 128-feature blocks of the chunk, y = behaviour.
// ---------------------------------------------------------------------------
struct CoefPermArgs {
    const double* Xc; int ldx;   // centred features (S, ldx), ldx a multiple of 128, columns >= B zero or unused
    const double* A;             // stack [n][T][S]
    int S, T, n, B;
    int f0, fc;                  // features f0 .. f0 + fc - 1 (f0 a multiple of 128)
    const double* obs;           // (B, T) observed coefficients
    const double* sd;            // [ldx] feature scale s_f, or nullptr: 1
    int* count;                  // (B, T) += #{b < n : s_f |coef_b| >= s_f |obs|}
    double* pmax;                // [feature blocks of the chunk][T][n]
};

static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_coef_perm_prod(CoefPermArgs a)
{
    __shared__ __attribute__((aligned(16))) double sX[CP_KB * CP_XLD];
    __shared__ __attribute__((aligned(16))) double sA[64 * CP_ALD];
    __shared__ double sM[4 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fb = a.f0 + blockIdx.x * 128;         // (fb + 127 < ldx: both multiples of 128, fb < B <= ldx)
    const int t = blockIdx.y;
    const int fend = min(a.B, a.f0 + a.fc);
    const bool al2 = cp_aligned(a.A, a.S);

    // the lane's 8 rows: scale, observed statistic, count
    double sf[2][4], ob[2][4];
    int cnt[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = cp_feature(fb, fend, r, i);
            sf[r][i] = f >= 0 ? (a.sd ? a.sd[f] : 1.0) : 0.0;
            ob[r][i] = f >= 0 ? sf[r][i] * fabs(a.obs[(size_t)f * a.T + t]) : 0.0;
            cnt[r][i] = 0;
        }

    double* pm = a.pmax + ((size_t)blockIdx.x * a.T + t) * a.n;
    const double* At = a.A + (size_t)t * a.S;       // row t of permutation 0; a permutation further on is T S doubles on
    const size_t pitch = (size_t)a.T * a.S;
    for (int b0 = 0; b0 < a.n; b0 += 64) {
        d4 acc[2][4];
        cp_clear(acc);
        cp_contract(CpTile{a.Xc, a.ldx, a.S, a.n, fb, b0, al2},
                    [&](int b) { return At + b * pitch; }, sX, sA, acc);
        // compare and count; the tile's maximum over the lane's rows (rows f >= fend carry s_f = 0: the identity of a
        // maximum of magnitudes)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const bool bok = b0 + nt * 16 + (lane & 15) < a.n;
            double m = 0.0;
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double v = sf[r][i] * fabs(acc[r][nt][i]);
                    cnt[r][i] += (bok && v >= ob[r][i]) ? 1 : 0;
                    m = fmax(m, v);
                }
            m = fmax(m, __shfl_xor(m, 16));
            m = fmax(m, __shfl_xor(m, 32));
            if (lane < 16) sM[wave * 64 + nt * 16 + lane] = m;
        }
        // (sM was last read before the barriers of this tile's stages: at least one, S >= 1)
        __syncthreads();
        if (tid < 64 && b0 + tid < a.n)
            pm[b0 + tid] = fmax(fmax(sM[tid], sM[64 + tid]), fmax(sM[128 + tid], sM[192 + tid]));
    }
    // the counts of a row over its 16 lanes; one owner per (f, t)
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
            if ((lane & 15) == 0 && f >= 0) a.count[(size_t)f * a.T + t] += c;
        }
}

// ---------------------------------------------------------------------------
// out[b][t] = max over the nfb feature blocks of a chunk of pmax[block][t][b], and over what an earlier chunk left
// there (first = 0).  One thread per (b, t).
// ---------------------------------------------------------------------------
static __global__ __launch_bounds__(256)
void k_coef_perm_max(const double* __restrict__ pmax, int nfb, int T, int n, int first, double* __restrict__ out)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)T * n) return;
    const int t = (int)(idx / n), b = (int)(idx % n);
    double m = first ? 0.0 : out[(size_t)b * T + t];
    for (int j = 0; j < nfb; ++j) m = fmax(m, pmax[((size_t)j * T + t) * n + b]);
    out[(size_t)b * T + t] = m;
}
