// plsx_k_cvperm.h -- permutation null of the behavioural cross-validation in dual space (plsx_crossval_perm_batch):
// the per-split moment tables (k_cvp_moments), the scaled Gram product (k_cvp_gram, k_cvp_reduce), the A operand of a
// (permutation, split) fit (k_cvp_build_A), its scores (k_cvp_final) and the score correlations of its latent variables (k_cvp_lv).
// Included by plsx_cvperm.hip after plsx_kernels.h.  gfx950 only.
//
// A permutation of Y leaves the feature side of a cross-validated fit untouched: under split s, with c(i) the cell of
// row i and mu / sigma the training mean / std (ddof = 1) of every feature per cell,
//     xc_i = x_i - mu_c(i)                        every row, training or test
//     M_s[i][t] = sum_f a_if xc_if . b_tf xc_tf   (S x S)
// with a = b = 1 / sigma_c(.) in correlation mode (M_s symmetric: Z Z^T) and, with covariance, b = 1 and a = 1 for
// a training row i, 1 / sigma_c(i) for a test row i: ONE matrix whose training rows hold Kgram = Xc Xc^T and whose
// test rows hold Kpred = Z Xc^T (only the columns t of training rows are ever used: A is 0 at test positions).  Then
//     W' = A M_s^T  (T' x S):  training columns = A Kgram (G = W' A^T), test columns = (Kpred A^T)^T = Q^T.
// 1 / sigma := 0 for a feature whose training rows of the cell all hold the bits of the first (k_cell_scale's rule).
#pragma once
#include "plsx_common.h"
#include "plsx_k_gram.h"

#define CVP_SB 8                 // splits per block of k_cvp_moments: one read of a row serves 8 tables

// mu[s][j][b], inv[s][j][b] (pitch ldt) of the training rows of cell j under masks[s] (1 = training row).  One thread
// per feature, rows in order; the two-pass variance and the bit-constancy rule of k_cell_scale.
// grid (ceil(B / 256), ceil(ns / CVP_SB)), block 256.
static __global__ __launch_bounds__(256)
void k_cvp_moments(const double* __restrict__ Xc, int ldx, int B, int J, const int* __restrict__ cell_start,
                   const int* __restrict__ cell_len, const uint8_t* __restrict__ masks, int S, int ns,
                   double* __restrict__ mu, double* __restrict__ inv, int ldt)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int s0 = blockIdx.y * CVP_SB;
    if (b >= B) return;
    const int nu = min(CVP_SB, ns - s0);
    for (int j = 0; j < J; ++j) {
        const int r0 = cell_start[j], n = cell_len[j];
        double s[CVP_SB], q[CVP_SB];
        long long first[CVP_SB];
        int cnt[CVP_SB];
        bool same[CVP_SB];
#pragma unroll
        for (int u = 0; u < CVP_SB; ++u) { s[u] = 0.0; q[u] = 0.0; first[u] = 0; cnt[u] = 0; same[u] = true; }
        for (int i = r0; i < r0 + n; ++i) {
            const double x = Xc[(size_t)i * ldx + b];
            const long long xb = __double_as_longlong(x);
#pragma unroll
            for (int u = 0; u < CVP_SB; ++u) {
                if (u < nu && masks[(size_t)(s0 + u) * S + i]) {
                    if (cnt[u] == 0) first[u] = xb;
                    same[u] = same[u] && xb == first[u];
                    s[u] += x;
                    ++cnt[u];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < CVP_SB; ++u) s[u] = s[u] / (double)cnt[u];
        for (int i = r0; i < r0 + n; ++i) {
            const double x = Xc[(size_t)i * ldx + b];
#pragma unroll
            for (int u = 0; u < CVP_SB; ++u) {
                if (u < nu && masks[(size_t)(s0 + u) * S + i]) { const double d = x - s[u]; q[u] += d * d; }
            }
        }
#pragma unroll
        for (int u = 0; u < CVP_SB; ++u) {
            if (u >= nu) continue;
            const double var = q[u] / (double)(cnt[u] - 1);
            const size_t o = ((size_t)(s0 + u) * J + j) * ldt + b;
            mu[o] = s[u];
            inv[o] = (!same[u] && var > 0.0) ? 1.0 / sqrt(var) : 0.0;
        }
    }
}

struct CvpGramArgs {
    const double* X; int ldx; int S; int K;            // the bound features (S x K live columns, pitch ldx)
    const double* mu; const double* inv; int ldt; int J;   // tables [split][J][ldt]
    const int* cell_of_row;                            // [S]
    const uint8_t* masks;                              // [split][S], 1 = training row
    int cov;
    int kchunk, nchunk;                                // columns per block (multiple of NT_KB), blocks along the contraction
    int mtiles;                                        // 64-tiles of S (the output is mtiles x mtiles tiles)
    double* part;                                      // [split][chunk][tile][64 * 64]
};

// The scaled Gram product M_s (above) of a batch of splits on v_mfma_f64_16x16x4_f64, tiled as k_nt_gemm<2>: a block
// owns 128 x 64 of one split's output over one chunk of the contraction, a wave 32 x 64 (two A fragments against
// four B fragments per k-step), 32 contraction columns per LDS stage at the conflict-free pitch NT_LD, the next
// stage's operands fetched into registers while the current one is multiplied.  The centring and the scales are
// applied to the fetched values on their way into LDS: no S x B scaled copy of X exists.  Partial tiles go to `part`
// and are summed in chunk order by k_cvp_reduce (no atomics).
// grid (nchunk, ceil(mtiles / 2) * mtiles, splits), block 256.
static __global__ __launch_bounds__(256)
void k_cvp_gram(CvpGramArgs a)
{
    __shared__ __attribute__((aligned(16))) double sA[2 * 64 * NT_LD];
    __shared__ __attribute__((aligned(16))) double sB[64 * NT_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x, split = blockIdx.z;
    const int tmb = blockIdx.y / a.mtiles, tn = blockIdx.y % a.mtiles;
    const int k0 = chunk * a.kchunk;
    const int k1 = min(a.K, k0 + a.kchunk);
    const int seg = tid & 15, rbase = tid >> 4;
    const uint8_t* mk = a.masks + (size_t)split * a.S;
    const double* mus = a.mu + (size_t)split * a.J * a.ldt;
    const double* invs = a.inv + (size_t)split * a.J * a.ldt;

    // rows of this thread: 8 of the A side, 4 of the B side; row < 0: past S.  toff = cell * ldt; bit i of `scl`: the
    // row takes 1 / sigma (A side bits 0..7, B side bits 8..11)
    int rowA[8], rowB[4], toffA[8], toffB[4];
    unsigned scl = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = tmb * 128 + rbase + 16 * i;
        rowA[i] = r < a.S ? r : -1;
        toffA[i] = r < a.S ? a.cell_of_row[r] * a.ldt : 0;
        if (r < a.S && (!a.cov || !mk[r])) scl |= 1u << i;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = tn * 64 + rbase + 16 * i;
        rowB[i] = r < a.S ? r : -1;
        toffB[i] = r < a.S ? a.cell_of_row[r] * a.ldt : 0;
        if (r < a.S && !a.cov) scl |= 1u << (8 + i);
    }

    d4 acc[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[r][i] = (d4){0, 0, 0, 0};

    d2 ra[8], rb[4];
    auto operand = [&](int row, int toff, bool scaled, int c) -> d2 {
        d2 v = (d2){0, 0};
        if (row < 0 || c >= k1) return v;
        const double* px = a.X + (size_t)row * a.ldx + c;
        const double* pm = mus + toff + c;
        const double* pi = invs + toff + c;
        if (c + 1 < k1) {
            const d2 x = *reinterpret_cast<const d2*>(px), m = *reinterpret_cast<const d2*>(pm);
            v = x - m;
            if (scaled) v = v * *reinterpret_cast<const d2*>(pi);
        } else {
            v[0] = px[0] - pm[0];
            if (scaled) v[0] = v[0] * pi[0];
        }
        return v;
    };
    auto fetch = [&](int kk) {
        const int c = kk + seg * 2;
#pragma unroll
        for (int i = 0; i < 8; ++i) ra[i] = operand(rowA[i], toffA[i], (scl >> i) & 1u, c);
#pragma unroll
        for (int i = 0; i < 4; ++i) rb[i] = operand(rowB[i], toffB[i], (scl >> (8 + i)) & 1u, c);
    };
    if (k0 < k1) fetch(k0);
    for (int kk = k0; kk < k1; kk += NT_KB) {
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<d2*>(&sA[(rbase + 16 * i) * NT_LD + seg * 2]) = ra[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<d2*>(&sB[(rbase + 16 * i) * NT_LD + seg * 2]) = rb[i];
        __syncthreads();
        if (kk + NT_KB < k1) fetch(kk + NT_KB);
#pragma unroll
        for (int ks = 0; ks < NT_KB / 4; ++ks) {
            const int off = (lane & 15) * NT_LD + ks * 4 + (lane >> 4);
            double fa[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) fa[r] = sA[(wave * 2 + r) * 16 * NT_LD + off];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const double fb = sB[nt * 16 * NT_LD + off];
#pragma unroll
                for (int r = 0; r < 2; ++r) acc[r][nt] = mfma_f64(fa[r], fb, acc[r][nt]);
            }
        }
        __syncthreads();
    }
    const size_t tiles = (size_t)a.mtiles * a.mtiles;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int rowb = (wave * 2 + r) * 16;                  // row of the block
        const int tm = tmb * 2 + rowb / 64;                    // 64-row output tile
        if (tm >= a.mtiles) continue;
        double* out = a.part + (((size_t)split * a.nchunk + chunk) * tiles + (size_t)tm * a.mtiles + tn) * 4096;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = (rowb & 63) + (lane >> 4) + 4 * i, n = nt * 16 + (lane & 15);
                out[m * 64 + n] = acc[r][nt][i];
            }
    }
}

// M[split][m][n] (pitch ldk) = sum over the chunks, in chunk order, of the partial tiles.
// grid (ceil(S * S / 256), splits), block 256.
static __global__ void k_cvp_reduce(const double* __restrict__ part, int nchunk, int mtiles, int S,
                                    double* __restrict__ M, int ldk)
{
    const int split = blockIdx.y;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)S * S) return;
    const int m = (int)(idx / S), n = (int)(idx % S);
    const size_t tiles = (size_t)mtiles * mtiles;
    const size_t off = ((size_t)(m / 64) * mtiles + n / 64) * 4096 + (m % 64) * 64 + (n % 64);
    const double* p = part + (size_t)split * nchunk * tiles * 4096 + off;
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += p[(size_t)c * tiles * 4096];
    M[((size_t)split * S + m) * ldk + n] = s;
}

// The A operand (T' x ld, dense, zeroed by the caller) of permutation r under one training mask, cell j:
//   A[r][j T + t][p] = zscore(Y[perm_r[p]][t]) / (n_j - 1)   for the training positions p of cell j, 0 elsewhere,
// mean / std (ddof = 1; covariance: centred only) over the n_j training positions of the cell in position order --
// the arithmetic of k_build_A_behav with the mask selecting the rows and the count.
// y_stride (here and in k_cvp_final / k_cvp_lv; 0 on every route but the fold-wise confound regression): permutation r
// reads Y + r * y_stride, the fold's Y_{s,p} already in position order, through an identity index row.
// grid (permutations, J), block 256, dynamic LDS 2 T doubles.
static __global__ void k_cvp_build_A(const double* __restrict__ Y, int T, int S, const int* __restrict__ cell_start,
                                     const int* __restrict__ cell_len, const uint8_t* __restrict__ mask,
                                     const int* __restrict__ perm, int Tp, int covariance,
                                     double* __restrict__ A, int ld, long long y_stride = 0)
{
    extern __shared__ double sm_cvp[];
    const int r = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
    Y += (size_t)r * y_stride;                         // (y_stride != 0: every permutation reads a Y of its own)
    const int start = cell_start[j], len = cell_len[j];
    const int* ys = perm + (size_t)r * S;
    double* mean = sm_cvp;
    double* rstd = sm_cvp + T;
    __shared__ int s_cnt;
    if (tid == 0) {
        int c = 0;
        for (int p = start; p < start + len; ++p) c += mask[p] != 0;
        s_cnt = c;
    }
    __syncthreads();
    const int cnt = s_cnt;
    for (int t = tid; t < T; t += blockDim.x) {
        double s = 0.0;
        for (int p = start; p < start + len; ++p)
            if (mask[p]) s += Y[(size_t)ys[p] * T + t];
        const double m = s / (double)cnt;
        double q = 0.0;
        for (int p = start; p < start + len; ++p)
            if (mask[p]) { const double d = Y[(size_t)ys[p] * T + t] - m; q += d * d; }
        mean[t] = m;
        rstd[t] = covariance ? 1.0 : 1.0 / sqrt(q / (double)(cnt - 1));
    }
    __syncthreads();
    const double inv_nm1 = 1.0 / (double)(cnt - 1);
    for (int idx = tid; idx < len * T; idx += blockDim.x) {
        const int pl = idx / T, t = idx - pl * T, p = start + pl;
        if (!mask[p]) continue;
        A[((size_t)r * Tp + j * T + t) * ld + p] = (Y[(size_t)ys[p] * T + t] - mean[t]) * rstd[t] * inv_nm1;
    }
}

// Predictions and scores of permutation r under one split (block = permutation): k_cv_final's arithmetic, term by
// term in its order, with the observed rows read through the permutation and q = column p of W' (already centred: no
// offset vector).
//   z_l = q^T v_l / d_l over the live LVs;  y_pred = z V_j^T + mean_train_j(Y[perm]);  r, r^2 per behaviour over the test rows
// k_cv_final gives one thread a whole test row (T' L + L T dependent steps on a quarter of the block's threads: 4.3 ms
// per launch of 1000 permutations at S = 500, T' = L = 50, a third of the whole null).  Here the three stages are
// spread over (row, LV), (row, behaviour) and behaviour; z passes through `zbuf`.
// out_r / out_r2: entry (r, t) at r * out_stride + t.
static __global__ __launch_bounds__(256)
void k_cvp_final(const double* __restrict__ W /* [m][Tp][ld] */, int ld,
                 const double* __restrict__ V /* [m][Tp][L] */, const double* __restrict__ d /* [m][L] */,
                 const double* __restrict__ Y, const uint8_t* __restrict__ mk, const int* __restrict__ perm,
                 const int* __restrict__ cell_of_pos, int S, int T, int J, int Tp, int L,
                 double* __restrict__ ybar /* scratch [m][J][T] */, double* __restrict__ zbuf /* scratch [m][S][L] */,
                 double* __restrict__ pred /* [m][S][T] */,
                 double* __restrict__ out_r, double* __restrict__ out_r2, long long out_stride, long long y_stride = 0)
{
    const int i = blockIdx.x, tid = threadIdx.x;
    Y += (size_t)i * y_stride;
    const int* ys = perm + (size_t)i * S;
    double* yb = ybar + (size_t)i * J * T;
    double* zb = zbuf + (size_t)i * S * L;
    double* pr = pred + (size_t)i * S * T;
    const double* Wi = W + (size_t)i * Tp * ld;
    const double* Vi = V + (size_t)i * Tp * L;
    const double* di = d + (size_t)i * L;
    // training means of the permuted Y per cell
    for (int idx = tid; idx < J * T; idx += blockDim.x) {
        const int j = idx / T, t = idx % T;
        double s = 0.0; int n = 0;
        for (int p = 0; p < S; ++p)
            if (mk[p] && cell_of_pos[p] == j) { s += Y[(size_t)ys[p] * T + t]; ++n; }
        yb[idx] = s / (double)n;
    }
    // z[p][l] of the test rows, u ascending; a dead LV contributes nothing
    const double dmax = di[0];
    for (long long idx = tid; idx < (long long)S * L; idx += blockDim.x) {
        const int p = (int)(idx / L), l = (int)(idx % L);
        if (mk[p]) continue;
        double z = 0.0;
        if (di[l] > PLSX_RANK_RTOL * dmax) {
            for (int u = 0; u < Tp; ++u) z += Wi[(size_t)u * ld + p] * Vi[(size_t)u * L + l];
            z /= di[l];
        }
        zb[idx] = z;
    }
    __syncthreads();
    // predictions, l ascending over the live LVs
    for (long long idx = tid; idx < (long long)S * T; idx += blockDim.x) {
        const int p = (int)(idx / T), t = (int)(idx % T);
        if (mk[p]) continue;
        const int j = cell_of_pos[p];
        const double* zp = zb + (size_t)p * L;
        const double* vr = Vi + (size_t)(j * T + t) * L;
        double y = yb[j * T + t];
        for (int l = 0; l < L; ++l)
            if (di[l] > PLSX_RANK_RTOL * dmax) y += zp[l] * vr[l];
        pr[idx] = y;
    }
    __syncthreads();
    for (int t = tid; t < T; t += blockDim.x) {
        double sy = 0, sp = 0, syy = 0, spp = 0, syp = 0, sres = 0; int n = 0;
        for (int p = 0; p < S; ++p) {
            if (mk[p]) continue;
            const double y = Y[(size_t)ys[p] * T + t], q = pr[(size_t)p * T + t];
            sy += y; sp += q; syy += y * y; spp += q * q; syp += y * q; sres += (y - q) * (y - q); ++n;
        }
        const double nn = (double)n;
        const double cov = syp - sy * sp / nn, vy = syy - sy * sy / nn, vp = spp - sp * sp / nn;
        double r = cov / sqrt(vy * vp);
        out_r[(size_t)i * out_stride + t] = (r > 1.0) ? 1.0 : ((r < -1.0) ? -1.0 : r);
        out_r2[(size_t)i * out_stride + t] = 1.0 - sres / vy;
    }
}

// Out-of-sample score correlations of the latent variables of permutation r under one split (block = permutation),
// after k_cvp_final of the same (pass, split): the x_scores are the z that kernel left in `zbuf` (0 for a dead LV), the
// y_scores (plsx_k_finish.h has the definition and the three shared stages) are formed here over (row, LV) into `ybuf`.
// No S x S or feature-sized work.  out_lv: entry (r, l) at r * out_stride + l.
// grid (permutations of the pass), block 256, dynamic LDS 2 J T doubles.
static __global__ __launch_bounds__(256)
void k_cvp_lv(const double* __restrict__ V /* [m][Tp][L] */, const double* __restrict__ d /* [m][L] */,
              const double* __restrict__ Y, const uint8_t* __restrict__ mk, const int* __restrict__ perm,
              const int* __restrict__ cell_of_pos, const int* __restrict__ cell_start, const int* __restrict__ cell_len,
              int S, int T, int J, int Tp, int L, int covariance, const double* zbuf /* [m][S][L] */,
              double* ybuf /* scratch [m][S][L] */, double* __restrict__ out_lv, long long out_stride,
              long long y_stride = 0)
{
    extern __shared__ double sm_cvlv[];
    double* mean = sm_cvlv;
    double* rstd = sm_cvlv + J * T;
    const int i = blockIdx.x, tid = threadIdx.x;
    Y += (size_t)i * y_stride;
    const int* ys = perm + (size_t)i * S;
    const double* Vi = V + (size_t)i * Tp * L;
    const double* di = d + (size_t)i * L;
    double* yi = ybuf + (size_t)i * S * L;
    cvlv_y_moments(Y, ys, mk, cell_start, cell_len, T, J, covariance, mean, rstd);
    __syncthreads();
    for (long long idx = tid; idx < (long long)S * L; idx += blockDim.x) {
        const int p = (int)(idx / L), l = (int)(idx % L);
        if (mk[p]) continue;
        yi[idx] = cvlv_y_score(Y + (size_t)ys[p] * T, mean, rstd, Vi, cell_of_pos[p], T, L, l);
    }
    __syncthreads();
    cvlv_pearson(zbuf + (size_t)i * S * L, yi, mk, di, S, L, out_lv + (size_t)i * out_stride);
}
