// plsx_k_confound_behav.h -- confound regression of the behavioural PLS-C front end: the feature-space side of the
// fold-wise regression (plsx_crossval_confound_batch / plsx_crossval_confound_perm_batch).
//
// PLS-C in correlation mode scales every feature by its per-cell training standard deviation, so the rank-2 q' update
// of K that the regression front end uses (plsx_k_confound.h) does not carry over: the fold's X has to exist.  With
// Z~ [CF_Q][S], P_s [q'][S] (k_cf_fold_prep) and X_r the bound residuals (pitch ldx = Bpad),
//     B_s = P_s X_r                (q' x B)      pass 1
//     X_s = X_r - Z~^T B_s         (S x Bpad)    pass 2, one copy per split of the group
// for CFB_G splits per launch: X_r is read twice per GROUP and each copy written once, (2 / g + 1) 8 S Bpad bytes per
// split against 3 x 8 S Bpad for k_cf_resid once per split.
#pragma once
#include "plsx_k_confound.h"

#define CFB_G 4                  // splits per launch: 4 x 16 double accumulators = 128 VGPR a lane (4 x 8 for q' <= 8)

// grid (ceil(ldx / 256)), block 256: a thread owns one feature column (lanes over the features: a row of X_r is read
// and a row of every copy written in full lines); the entries of P_s and Z~ are wave-uniform.  The CFB_G x QC
// accumulators have compile-time indices (QC = 8 or CF_Q >= q': the loops over the padded q' are unrolled, rows
// j >= q' skipped by a wave-uniform test), rows in ascending order, no atomics: the bits of a split's copy depend
// neither on the group it is formed in nor on QC.  UNR: rows of pass 1 in flight.  Compiler's resource output
// (gfx950): <8, 8> 87 VGPR, 5 waves / SIMD; <16, 4> 161 VGPR, 3 waves / SIMD; no scratch memory, no LDS.
// P [ng][q'][S]; Xf [ng][S][ldx], every entry written, the padding columns B .. ldx-1 as zeros.
template <int QC, int UNR>
static __global__ __launch_bounds__(256)
void k_cfb_fold_X(const double* __restrict__ Xr, int ldx, int B, int S, const double* __restrict__ Zt,
                  const double* __restrict__ P, int qp, int ng, double* __restrict__ Xf)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= ldx) return;
    const size_t copy = (size_t)S * ldx;
    if (f >= B) {
        for (int g = 0; g < ng; ++g)
            for (int p = 0; p < S; ++p) Xf[g * copy + (size_t)p * ldx + f] = 0.0;
        return;
    }
    double b[CFB_G][QC];
#pragma unroll
    for (int g = 0; g < CFB_G; ++g)
#pragma unroll
        for (int j = 0; j < QC; ++j) b[g][j] = 0.0;
#pragma unroll UNR
    for (int p = 0; p < S; ++p) {
        const double x = Xr[(size_t)p * ldx + f];
#pragma unroll
        for (int g = 0; g < CFB_G; ++g)
            if (g < ng) {
                const double* Pg = P + (size_t)g * qp * S + p;
#pragma unroll
                for (int j = 0; j < QC; ++j)
                    if (j < qp) b[g][j] += Pg[(size_t)j * S] * x;
            }
    }
#pragma unroll 2
    for (int p = 0; p < S; ++p) {
        const double x = Xr[(size_t)p * ldx + f];
        double z[QC];
#pragma unroll
        for (int j = 0; j < QC; ++j) z[j] = j < qp ? Zt[(size_t)j * S + p] : 0.0;
#pragma unroll
        for (int g = 0; g < CFB_G; ++g)
            if (g < ng) {
                double v = x;
#pragma unroll
                for (int j = 0; j < QC; ++j)
                    if (j < qp) v -= z[j] * b[g][j];
                Xf[g * copy + (size_t)p * ldx + f] = v;
            }
    }
}

// rows [n][S] of the identity index 0 .. S-1 (the fold's Y of a permutation is already in position order)
static __global__ __launch_bounds__(256)
void k_cfb_identity(int* __restrict__ idx, int S, int n)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S || (int)blockIdx.y >= n) return;
    idx[(size_t)blockIdx.y * S + p] = p;
}
