// plsx_k_confound.h -- confound regression of the SIMPLS front end (plsx_simpls_set_confounds and the two fold entries,
// plsx_simpls_crossval_confound_batch / plsx_simpls_crossval_confound_perm_batch).
//
// Z~ = [1, Z - zbar] (S x q', q' = q + 1 <= 16) over the usable rows, zero rows elsewhere, stored [CF_Q][S] (row j =
// column j of Z~, rows q' .. 15 zero) so that lanes over positions read contiguous bytes.
//     bound data:   X_r = M X, Y_r = M Y,  M = I - Z~ (Z~^T Z~)^-1 Z~^T                         k_cf_resid
//     split s:      P_s = (Z~^T D Z~)^-1 Z~^T D   (q' x S, D = its training rows)               k_cf_fold_prep
//                   C_s = P_s K_r                 (one product for all the splits of a group)   k_nt_gemm
//                   E_s = P_s C_s^T,  F_s = C_s - 1/2 E_s Z~        (stored [q'][S] like Z~)    k_cf_fold_F
//                   K_s = K_r - Z~^T F_s - F_s^T Z~ = M_s K_r M_s^T                             k_cf_fold_K
//                   Y_s = Y_r[perm] - Z~^T (P_s Y_r[perm])                                      k_cf_fold_Y
// M_s = I - Z~^T P_s residualises EVERY row by the regression of the training rows; M_s Z~^T = 0, so the fold-wise
// residuals of the raw data are those of the bound, residualised data.  The solver and k_sd_cv_score then run on
// (K_s, Y_s) as they run on (K, Y).  Small matrices (q' x q') live in a wave's LDS slice padded to 16 x 16 with the
// identity, so that every loop over them has compile-time bounds; reductions are wave_sum in fixed order, no atomics.
#pragma once
#include "plsx_simpls.h"

#define CF_Q 16

// Z~ of the bound rows.  grid (q'), one block per column: its mean over the usable rows (a fixed tree), then the column.
static __global__ __launch_bounds__(256)
void k_cf_ztilde(const double* __restrict__ Z, int q, int S, const uint8_t* __restrict__ okx,
                 const uint8_t* __restrict__ oky, double* __restrict__ Zt)
{
    __shared__ double red_s[256], red_c[256];
    const int j = blockIdx.x, tid = threadIdx.x;
    auto ok = [&](int p) { return (!okx || okx[p]) && (!oky || oky[p]); };
    double* row = Zt + (size_t)j * S;
    if (j == 0) {
        for (int p = tid; p < S; p += 256) row[p] = ok(p) ? 1.0 : 0.0;
        return;
    }
    double s = 0.0, c = 0.0;
    for (int p = tid; p < S; p += 256)
        if (ok(p)) { s += Z[(size_t)p * q + (j - 1)]; c += 1.0; }
    red_s[tid] = s; red_c[tid] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { red_s[tid] += red_s[tid + o]; red_c[tid] += red_c[tid + o]; }
        __syncthreads();
    }
    const double mean = red_s[0] / red_c[0];
    for (int p = tid; p < S; p += 256) row[p] = ok(p) ? Z[(size_t)p * q + (j - 1)] - mean : 0.0;
}

// G = Z~ D Z~^T (q' x q'; d: the training mask of a split, nullptr: every row) and its Cholesky factor, in place, in
// the wave's LDS slice G [CF_Q][CF_Q], padded with the identity.  false: a pivot at or below 1e-10 of its diagonal
// entry -- the columns are linearly dependent on these rows (the factor is then not usable).  Called by a whole wave.
__device__ __forceinline__ bool cf_gram_chol(const double* __restrict__ Zt, const uint8_t* __restrict__ d, int S, int qp,
                                             int lane, double* G)
{
    for (int i = lane; i < CF_Q * CF_Q; i += 64) G[i] = (i / CF_Q == i % CF_Q) ? 1.0 : 0.0;
    wave_sync();
    for (int i = 0; i < qp; ++i)
        for (int j = 0; j <= i; ++j) {
            const double* zi = Zt + (size_t)i * S;
            const double* zj = Zt + (size_t)j * S;
            double part = 0.0;
            for (int p = lane; p < S; p += 64) part += (!d || d[p]) ? zi[p] * zj[p] : 0.0;
            const double v = wave_sum(part);
            if (lane == 0) G[i * CF_Q + j] = v;
        }
    wave_sync();
    int good = 1;
    if (lane == 0) {
        for (int j = 0; j < qp; ++j) {
            const double diag = G[j * CF_Q + j];
            double v = diag;
            for (int m = 0; m < j; ++m) v -= G[j * CF_Q + m] * G[j * CF_Q + m];
            if (!(v > 1e-10 * diag)) { good = 0; v = 1.0; }
            const double l = sqrt(v);
            G[j * CF_Q + j] = l;
            for (int i = j + 1; i < qp; ++i) {
                double w = G[i * CF_Q + j];
                for (int m = 0; m < j; ++m) w -= G[i * CF_Q + m] * G[j * CF_Q + m];
                G[i * CF_Q + j] = w / l;
            }
        }
    }
    wave_sync();
    return __shfl(good, 0) != 0;
}

// Inv = (L L^T)^-1 from the padded factor of cf_gram_chol, both [CF_Q][CF_Q] in the wave's LDS slice (rows beyond q':
// the identity).  Lane c < 16 solves for column c, which no other lane touches.  Called by a whole wave.
__device__ __noinline__ void cf_chol_inverse(const double* L, double* Inv, int lane)
{
    if (lane < CF_Q) {
        const int c = lane;
#pragma nounroll
        for (int i = 0; i < CF_Q; ++i) {
            double v = i == c ? 1.0 : 0.0;
#pragma nounroll
            for (int m = 0; m < i; ++m) v -= L[i * CF_Q + m] * Inv[m * CF_Q + c];
            Inv[i * CF_Q + c] = v / L[i * CF_Q + i];
        }
#pragma nounroll
        for (int i = CF_Q - 1; i >= 0; --i) {
            double v = Inv[i * CF_Q + c];
#pragma nounroll
            for (int m = i + 1; m < CF_Q; ++m) v -= L[m * CF_Q + i] * Inv[m * CF_Q + c];
            Inv[i * CF_Q + c] = v / L[i * CF_Q + i];
        }
    }
    wave_sync();
}

// y = Inv x for a 16-vector in registers (compile-time bounds; the entries of Inv are LDS broadcasts)
__device__ __forceinline__ void cf_apply_inverse(const double* Inv, const double (&x)[CF_Q], double (&y)[CF_Q])
{
#pragma unroll
    for (int j = 0; j < CF_Q; ++j) {
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < CF_Q; ++i) v += Inv[j * CF_Q + i] * x[i];
        y[j] = v;
    }
}

// (Z~ Z~^T)^-1 of the bound rows (plsx_simpls_set_confounds): one wavefront.  Iout [CF_Q][CF_Q], padded with the
// identity; status[0] = 1: rank deficient.
static __global__ __launch_bounds__(64)
void k_cf_chol(const double* __restrict__ Zt, int S, int qp, double* __restrict__ Iout, int* __restrict__ status)
{
    __shared__ double G[CF_Q * CF_Q], Inv[CF_Q * CF_Q];
    const int lane = threadIdx.x;
    const bool good = cf_gram_chol(Zt, nullptr, S, qp, lane, G);
    cf_chol_inverse(G, Inv, lane);
    for (int i = lane; i < CF_Q * CF_Q; i += 64) Iout[i] = Inv[i];
    if (lane == 0) status[0] = good ? 0 : 1;
}

// A <- M A for the columns of A ([S][lda], ncols of them: the bound Xc, then Y), lanes over the columns so that a row
// is read and written in full lines.  One thread per column: Z~ a over the S rows in ascending order (the entries of
// Z~ are wave-uniform), the normal equations through (Z~ Z~^T)^-1, then the subtraction; rows that are not usable
// (row 0 of Z~ is their indicator) are written as zeros.  gout (q, ldg) or nullptr: the slopes on Z - zbar.
static __global__ __launch_bounds__(256)
void k_cf_resid(double* __restrict__ A, int lda, int ncols, int S, const double* __restrict__ Zt, int qp,
                const double* __restrict__ Ig, double* __restrict__ gout, int ldg)
{
    __shared__ double Inv[CF_Q * CF_Q];
    for (int i = threadIdx.x; i < CF_Q * CF_Q; i += 256) Inv[i] = Ig[i];
    __syncthreads();
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= ncols) return;
    double za[CF_Q], g[CF_Q];
#pragma unroll
    for (int j = 0; j < CF_Q; ++j) za[j] = 0.0;
#pragma unroll 4
    for (int p = 0; p < S; ++p) {
        const double a = A[(size_t)p * lda + f];
#pragma unroll
        for (int j = 0; j < CF_Q; ++j) za[j] += Zt[(size_t)j * S + p] * a;
    }
    cf_apply_inverse(Inv, za, g);
    if (gout) {
#pragma unroll
        for (int j = 1; j < CF_Q; ++j)
            if (j < qp) gout[(size_t)(j - 1) * ldg + f] = g[j];
    }
#pragma unroll 4
    for (int p = 0; p < S; ++p) {
        double v = A[(size_t)p * lda + f];
#pragma unroll
        for (int j = 0; j < CF_Q; ++j) v -= Zt[(size_t)j * S + p] * g[j];
        A[(size_t)p * lda + f] = Zt[p] != 0.0 ? v : 0.0;
    }
}

// P_s of the splits of a group: one wavefront per split.  masks [ns][S], 1 = training row; P [ns][q'][S] (every entry
// written); nte [ns]: the usable test rows of the split; status [ns]: 1 = Z~ is rank deficient on its training rows.
static __global__ __launch_bounds__(256)
void k_cf_fold_prep(const double* __restrict__ Zt, const uint8_t* __restrict__ masks, int S, int qp, int ns,
                    double* __restrict__ P, double* __restrict__ nte, int* __restrict__ status)
{
    __shared__ double sm[4][2][CF_Q * CF_Q];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s = blockIdx.x * 4 + wave;
    if (s >= ns) return;
    const uint8_t* d = masks + (size_t)s * S;
    double* L = sm[wave][0];
    double* Inv = sm[wave][1];
    const bool good = cf_gram_chol(Zt, d, S, qp, lane, L);
    cf_chol_inverse(L, Inv, lane);
    double cnt = 0.0;
    for (int p = lane; p < S; p += 64) cnt += (!d[p] && Zt[p] != 0.0) ? 1.0 : 0.0;
    cnt = wave_sum(cnt);
    if (lane == 0) { nte[s] = cnt; status[s] = good ? 0 : 1; }
    double* Ps = P + (size_t)s * qp * S;
    for (int p = lane; p < S; p += 64) {
        double z[CF_Q];
        const bool tr = d[p] != 0;
#pragma unroll
        for (int j = 0; j < CF_Q; ++j) z[j] = tr ? Zt[(size_t)j * S + p] : 0.0;
#pragma unroll
        for (int j = 0; j < CF_Q; ++j)
            if (j < qp) {
                double v = 0.0;
#pragma unroll
                for (int i = 0; i < CF_Q; ++i) v += Inv[j * CF_Q + i] * z[i];
                Ps[(size_t)j * S + p] = v;
            }
    }
}

// E_s = P_s C_s^T (q' x q', symmetric: the lower triangle is formed and mirrored) and F_s = C_s - 1/2 E_s Z~, one
// wavefront per split.  P, C, F [ns][q'][S].
static __global__ __launch_bounds__(256)
void k_cf_fold_F(const double* __restrict__ Zt, const double* __restrict__ P, const double* __restrict__ C, int S, int qp,
                 int ns, double* __restrict__ F)
{
    __shared__ double sm[4][CF_Q * CF_Q];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int s = blockIdx.x * 4 + wave;
    if (s >= ns) return;
    double* E = sm[wave];
    const double* Ps = P + (size_t)s * qp * S;
    const double* Cs = C + (size_t)s * qp * S;
    double* Fs = F + (size_t)s * qp * S;
    for (int i = lane; i < CF_Q * CF_Q; i += 64) E[i] = 0.0;
    wave_sync();
    for (int i = 0; i < qp; ++i)
        for (int j = 0; j <= i; ++j) {
            double part = 0.0;
            for (int p = lane; p < S; p += 64) part += Ps[(size_t)i * S + p] * Cs[(size_t)j * S + p];
            const double v = wave_sum(part);
            if (lane == 0) { E[i * CF_Q + j] = v; E[j * CF_Q + i] = v; }
        }
    wave_sync();
    for (int p = lane; p < S; p += 64) {
        double z[CF_Q];
#pragma unroll
        for (int i = 0; i < CF_Q; ++i) z[i] = Zt[(size_t)i * S + p];
#pragma unroll
        for (int j = 0; j < CF_Q; ++j)
            if (j < qp) {
                double v = 0.0;
#pragma unroll
                for (int i = 0; i < CF_Q; ++i) v += E[i * CF_Q + j] * z[i];
                Fs[(size_t)j * S + p] = Cs[(size_t)j * S + p] - 0.5 * v;
            }
    }
}

// K_s = K_r - Z~^T F_s - F_s^T Z~ of a group of splits: 64 x 64 tiles, grid (tile, tile, split), the four 16 x 64
// panels (Z~ and F_s at the tile's rows and at its columns; rows beyond q' zero) in LDS.  A lane owns one column of the
// tile and keeps its two panel columns in registers; a wave walks 16 rows, whose panel entries are LDS broadcasts, and
// stores 512 contiguous bytes per row.  Plain stores, every entry of Ks [ns][S][S] written.
static __global__ __launch_bounds__(256)
void k_cf_fold_K(const double* __restrict__ Kr, const double* __restrict__ Zt, const double* __restrict__ F, int S, int qp,
                 double* __restrict__ Ks)
{
    __shared__ double za[CF_Q][64], fa[CF_Q][64], zb[CF_Q][64], fb[CF_Q][64];
    const int b0 = blockIdx.x * 64, a0 = blockIdx.y * 64, s = blockIdx.z;
    const double* Fs = F + (size_t)s * qp * S;
    for (int i = threadIdx.x; i < CF_Q * 64; i += 256) {
        const int j = i >> 6, c = i & 63;
        const bool ina = j < qp && a0 + c < S, inb = j < qp && b0 + c < S;
        za[j][c] = ina ? Zt[(size_t)j * S + a0 + c] : 0.0;
        fa[j][c] = ina ? Fs[(size_t)j * S + a0 + c] : 0.0;
        zb[j][c] = inb ? Zt[(size_t)j * S + b0 + c] : 0.0;
        fb[j][c] = inb ? Fs[(size_t)j * S + b0 + c] : 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = b0 + lane;
    double zc[CF_Q], fc[CF_Q];
#pragma unroll
    for (int j = 0; j < CF_Q; ++j) { zc[j] = zb[j][lane]; fc[j] = fb[j][lane]; }
    double* out = Ks + (size_t)s * S * S;
    for (int i = 0; i < 16; ++i) {
        const int ar = wave * 16 + i, a = a0 + ar;
        if (a >= S) break;
        double v = b < S ? Kr[(size_t)a * S + b] : 0.0;
#pragma unroll
        for (int j = 0; j < CF_Q; ++j) v -= za[j][ar] * fc[j] + fa[j][ar] * zc[j];
        if (b < S) out[(size_t)a * S + b] = v;
    }
}

// The Y of a fit's own, into the solver's `ystack` layout [fit][S][T]: fit f of the batch is split f / mb of the group
// under permutation f % mb of the chunk (perm [mb][S], or nullptr: the identity, mb = 1),
//     Y_s = Y_r[perm] - Z~^T (P_s Y_r[perm]).
// One wavefront per fit, lanes over positions; per behaviour the q' coefficients are wave sums in fixed order.
static __global__ __launch_bounds__(256)
void k_cf_fold_Y(const double* __restrict__ Yr, const double* __restrict__ Zt, const double* __restrict__ P,
                 const int* __restrict__ perm, int S, int T, int qp, int mb, int nfit, double* __restrict__ Ys)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f = blockIdx.x * 4 + wave;
    if (f >= nfit) return;
    const double* Ps = P + (size_t)(f / mb) * qp * S;
    const int* pr = perm ? perm + (size_t)(f % mb) * S : nullptr;
    double* out = Ys + (size_t)f * S * T;
    for (int t = 0; t < T; ++t) {
        double c[CF_Q];
#pragma unroll
        for (int j = 0; j < CF_Q; ++j) {
            c[j] = 0.0;
            if (j < qp) {
                double part = 0.0;
                for (int p = lane; p < S; p += 64) part += Ps[(size_t)j * S + p] * Yr[(size_t)(pr ? pr[p] : p) * T + t];
                c[j] = wave_sum(part);
            }
        }
        for (int p = lane; p < S; p += 64) {
            double v = Yr[(size_t)(pr ? pr[p] : p) * T + t];
#pragma unroll
            for (int j = 0; j < CF_Q; ++j)
                if (j < qp) v -= Zt[(size_t)j * S + p] * c[j];
            out[(size_t)p * T + t] = v;
        }
    }
}

// The training mask of every fit of such a batch (fit f: split f / mb of the group).  grid (ceil(S / 256), fits).
static __global__ __launch_bounds__(256)
void k_cf_expand_masks(const uint8_t* __restrict__ masks, int S, int mb, uint8_t* __restrict__ pmask)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S) return;
    pmask[(size_t)blockIdx.y * S + p] = masks[(size_t)(blockIdx.y / mb) * S + p];
}

// The reduction over the splits of plsx_simpls_crossval_confound_perm_batch: the fits of a batch are [ngc][mb] (split
// of the group, permutation of the chunk); permutation p adds its scores SPLIT BY SPLIT in ascending order to what the
// earlier groups left in the output (which starts from zero) and, after the call's last split, divides by n.  One
// thread per output entry, no atomics.  mse of a fit: its squared errors summed over the behaviours in ascending t,
// over the usable test rows of its split.  grid (ceil(E / 256), mb), E = 2 k T + k + 1.
static __global__ __launch_bounds__(256)
void k_cf_cvp_acc(const double* __restrict__ r, const double* __restrict__ r2, const double* __restrict__ sse,
                  const double* __restrict__ nte, int k, int T, int ngc, int mb, int n, int last,
                  double* __restrict__ out_r, double* __restrict__ out_r2, double* __restrict__ out_mse)
{
    const int kT = k * T, e = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (e >= 2 * kT + k + 1) return;
    if (e < 2 * kT) {
        const double* src = e < kT ? r + e : r2 + (e - kT);
        double* dst = e < kT ? out_r + (size_t)p * kT + e : out_r2 + (size_t)p * kT + (e - kT);
        double acc = *dst;
        for (int s = 0; s < ngc; ++s) acc += src[((size_t)s * mb + p) * kT];
        *dst = last ? acc / n : acc;
    } else {
        const int c = e - 2 * kT;
        double* dst = out_mse + (size_t)p * (k + 1) + c;
        double acc = *dst;
        for (int s = 0; s < ngc; ++s) {
            const double* row = sse + (((size_t)s * mb + p) * (k + 1) + c) * T;
            double v = 0.0;
            for (int t = 0; t < T; ++t) v += row[t];
            acc += v / nte[s];
        }
        *dst = last ? acc / n : acc;
    }
}
