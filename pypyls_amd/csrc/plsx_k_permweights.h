// plsx_k_permweights.h -- permutation test of the PLS-C x_weights: the subject-space operands W_p of the null
// Z_p = R_p^T V0 = W_p . Xf (k_perm_W_behav; k_perm_VA + k_perm_W_mc) and the reciprocal feature scale (k_col_rsd).  The
// feature pass itself is k_coef_perm_prod / k_coef_perm_max (plsx_k_coefperm.h), unchanged.
// Included by plsx_permweights.hip alone (after plsx_kernels.h).  gfx950 only.
#pragma once
#include "plsx_common.h"
#include "plsx_k_prep.h"

// ---------------------------------------------------------------------------
// Behavioural PLS.  Permutation r places row ysrc[p] of Y at position p; X stays.  Row j T + t of R_r is, over the
// positions p of cell j, sum_p z_r(p, t) Xf[p][.] with z_r(p, t) = (Y[ysrc[p]][t] - mean) * rstd / (n_j - 1), the
// moments over the cell's positions exactly as k_build_A_behav / k_build_A_proj form them for a permutation (rstd = 1
// with `covariance`), so
//   W[r][l][p] = sum_t V[j T + t][l] * z_r(p, t),   t ascending: a fixed summation order, one writer per entry.
// This is k_build_A_proj with a dense output and m <= T' columns of V (T' x m, row-major): the same moment loops in
// the same order, the cell's rows through LDS in chunks of build_A_proj_chunk(T, m) rows, the cell's T x m block of V
// in LDS (VLDS) or, where it is too large, in global memory.  Every (l, p) of W is written, whatever the index rows
// hold: no zeroing by the caller.
// grid (n, J), block 256; dynamic LDS: build_A_proj_lds(T, m) bytes.
// ---------------------------------------------------------------------------
template <bool VLDS>
static __global__ __launch_bounds__(256)
void k_perm_W_behav(const double* __restrict__ Y, int T, int S,
                    const int* __restrict__ cell_start, const int* __restrict__ cell_len,
                    const int* __restrict__ ysrc, const double* __restrict__ V, int m, int covariance,
                    double* __restrict__ W)
{
    extern __shared__ double sm_b[];
    const int r = blockIdx.x, j = blockIdx.y;
    const int start = cell_start[j], len = cell_len[j];
    const int* ys = ysrc + (size_t)r * S;
    const int ch = build_A_proj_chunk(T, m);
    double* mean = sm_b;            // [T]
    double* rstd = sm_b + T;        // [T]
    double* sZ = sm_b + 2 * T;      // [ch][T]: (y - mean) * rstd / (n_j - 1) of the chunk's rows
    double* sV = sZ + ch * T;       // [T][m]: rows j T .. j T + T - 1 of V (T' x m)
    const double* Vj = V + (size_t)j * T * m;
    const int tid = threadIdx.x;
    if (VLDS)
        for (int i = tid; i < T * m; i += blockDim.x) sV[i] = Vj[i];
    for (int t = tid; t < T; t += blockDim.x) {
        double s = 0.0;
        for (int p = start; p < start + len; ++p) s += Y[(size_t)ys[p] * T + t];
        const double mu = s / (double)len;
        double q = 0.0;
        for (int p = start; p < start + len; ++p) {
            const double d = Y[(size_t)ys[p] * T + t] - mu;
            q += d * d;
        }
        mean[t] = mu;
        rstd[t] = covariance ? 1.0 : 1.0 / sqrt(q / (double)(len - 1));
    }
    __syncthreads();
    double* Wr = W + (size_t)r * m * S;
    const double inv_nm1 = 1.0 / (double)(len - 1);
    const double* Vs = VLDS ? sV : Vj;
    for (int c0 = 0; c0 < len; c0 += ch) {
        const int nr = min(ch, len - c0);
        for (int idx = tid; idx < nr * T; idx += blockDim.x) {
            const int pl = idx / T, t = idx - pl * T;
            sZ[idx] = (Y[(size_t)ys[start + c0 + pl] * T + t] - mean[t]) * rstd[t] * inv_nm1;
        }
        __syncthreads();
        // rows 4 q .. 4 q + 3 of the chunk, entry l; the rows of the last four beyond nr read what an earlier chunk
        // left (or nothing yet) inside sZ and are not stored
        const int nq = (nr + 3) >> 2;
        for (int idx = tid; idx < nq * m; idx += blockDim.x) {
            const int l = idx / nq, q = idx - l * nq;       // (q fastest: neighbouring threads store neighbouring rows)
            const double* z = sZ + (size_t)q * 4 * T;
            double v[4] = {0.0, 0.0, 0.0, 0.0};
            for (int t = 0; t < T; ++t) {
                const double w = Vs[(size_t)t * m + l];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = __builtin_fma(z[i * T + t], w, v[i]);
            }
            const int p0 = start + c0 + q * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (q * 4 + i < nr) Wr[(size_t)l * S + p0 + i] = v[i];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Mean-centred PLS.  R_r = A . X[perm_r] with A (J x S) the design's averaging weights (k_build_A_mc on the identity:
// the cell sizes do not move under a permutation).  VA[l][p] = sum_j V[j][l] * A[j][p], j ascending, is the same for
// every permutation: one thread per (l, p).  grid (ceil(S / 256), m), block 256.
// ---------------------------------------------------------------------------
static __global__ __launch_bounds__(256)
void k_perm_VA(const double* __restrict__ Adense, int ld, int S, int J, const double* __restrict__ V, int m,
               double* __restrict__ VA)
{
    const int p = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
    if (p >= S) return;
    double v = 0.0;
    for (int j = 0; j < J; ++j) v = __builtin_fma(V[(size_t)j * m + l], Adense[(size_t)j * ld + p], v);
    VA[(size_t)l * S + p] = v;
}

// ---------------------------------------------------------------------------
// ... and W_r is VA scattered by the permutation: position p holds row src[p] of X, so
//   W[r][l][s] = sum over the positions p with src[p] == s, p ascending, of VA[l][p]
// -- one term for a permutation, none (0) or several for index rows that skip or repeat a row.  The thread of subject s
// owns column s of W_r: one writer per entry, a fixed order.  How often s occurs and where first come from integer
// counters in the block's own slice of `ws` ([n][2][S] ints; integer adds and minima have no order); only a repeated row
// makes its thread walk the positions.  grid (n), block 256.
// ---------------------------------------------------------------------------
static __global__ __launch_bounds__(256)
void k_perm_W_mc(const int* __restrict__ src, int S, const double* __restrict__ VA, int m, int* __restrict__ ws,
                 double* __restrict__ W)
{
    const int r = blockIdx.x, tid = threadIdx.x;
    const int* xs = src + (size_t)r * S;
    int* cnt = ws + (size_t)r * 2 * S;
    int* pos = cnt + S;
    for (int s = tid; s < S; s += blockDim.x) { cnt[s] = 0; pos[s] = S; }
    __syncthreads();
    for (int p = tid; p < S; p += blockDim.x) {
        const int s = xs[p];
        atomicAdd(&cnt[s], 1);
        atomicMin(&pos[s], p);
    }
    __syncthreads();
    double* Wr = W + (size_t)r * m * S;
    for (int s = tid; s < S; s += blockDim.x) {
        const int c = cnt[s], p0 = pos[s];
        for (int l = 0; l < m; ++l) {
            const double* va = VA + (size_t)l * S;
            double v = 0.0;
            if (c == 1) v = va[p0];
            else if (c > 1)
                for (int p = p0; p < S; ++p)
                    if (xs[p] == s) v += va[p];
            Wr[(size_t)l * S + s] = v;
        }
    }
}

// ---------------------------------------------------------------------------
// rsd[f] = 1 / s_f, s_f = sqrt(sum_s Xc[s][f]^2 / (S - 1)) the standard deviation of the bound, centred feature over all
// S rows -- k_col_sd's sum in k_col_sd's order -- and 0 where the feature has no variance: s_f = 0, or every row holds
// the bits of the first (the rounded mean of S equal numbers usually misses them by an ulp and the sum comes out near
// 1e-34 c^2, not 0: k_cell_scale's rule).  One thread per feature, s ascending.  Columns B .. ldx - 1 get 0.
// ---------------------------------------------------------------------------
static __global__ __launch_bounds__(256)
void k_col_rsd(const double* __restrict__ Xc, int ldx, int S, int B, double* __restrict__ rsd)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= ldx) return;
    double s = 0.0;
    bool same = true;
    if (f < B) {
        const long long first = __double_as_longlong(Xc[f]);
        for (int r = 0; r < S; ++r) {
            const double x = Xc[(size_t)r * ldx + f];
            s += x * x;
            same = same && __double_as_longlong(x) == first;
        }
    }
    const double sd = sqrt(s / ((double)S - 1.0));
    rsd[f] = (f < B && !same && sd > 0.0) ? 1.0 / sd : 0.0;
}
