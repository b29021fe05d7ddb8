// plsx_confound.hip -- confound regression of the SIMPLS front end: plsx_simpls_set_confounds and what the fold
// entries (plsx_simpls_api.hip) launch per group of splits (plsx_k_confound.h)
// Part of libplsx.so (plsx_internal.h has the map of translation units).  gfx950 only.
#include "plsx_internal.h"
#include "plsx_k_confound.h"
using namespace plsxi;

namespace plsxi {

// P_s, C_s = P_s K_r, F_s and K_s of the ns splits d_masks [ns][S] (the call's splits s0 ..), into ctx->cfK [ns][S][S];
// the usable test rows of every split into ctx->cfnte.  A split on whose training rows Z~ is rank deficient is
// refused by name (PLSX_ERR_ARG) before K_s is formed.
int cf_fold_prepare(plsx_ctx* ctx, const uint8_t* d_masks, int s0, int ns, hipStream_t st)
{
    const int S = ctx->S, qp = ctx->cf_q + 1;
    const size_t pbytes = (size_t)ns * qp * S * 8;
    if (int e = ensure(ctx, ctx->cfP, pbytes)) return e;
    if (int e = ensure(ctx, ctx->cfC, pbytes)) return e;
    if (int e = ensure(ctx, ctx->cfF, pbytes)) return e;
    if (int e = ensure(ctx, ctx->cfnte, (size_t)ns * 8)) return e;
    if (int e = ensure(ctx, ctx->cfstat, (size_t)std::max(ns, 1) * sizeof(int))) return e;
    if (int e = ensure(ctx, ctx->cfK, (size_t)ns * S * S * 8)) return e;
    const double* Zt = ptr<double>(ctx->cfZ);
    {
        KTimer tm(ctx, KC_CFPREP, st);
        hipLaunchKernelGGL(k_cf_fold_prep, dim3(ceil_div(ns, 4)), dim3(256), 0, st, Zt, d_masks, S, qp, ns,
                           ptr<double>(ctx->cfP), ptr<double>(ctx->cfnte), ptr<int>(ctx->cfstat));
        LAUNCHCHK();
    }
    std::vector<int> bad(ns);
    HIPCHK(hipMemcpyAsync(bad.data(), ctx->cfstat.p, (size_t)ns * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int s = 0; s < ns; ++s)
        if (bad[s]) {
            char msg[200];
            snprintf(msg, sizeof msg, "the confounds (with the intercept) are rank deficient on the training rows of "
                     "split %d", s0 + s);
            return fail(ctx, PLSX_ERR_ARG, msg);
        }
    // C_s = P_s K_r (K_r symmetric) for every split of the group: ONE product
    if (int e = run_nt(ctx, ptr<double>(ctx->cfP), 0, S, ns * qp, ptr<double>(ctx->Kmat), 0, S, S, nullptr, 0, 0, 0, S, 1,
                       ptr<double>(ctx->cfC), 0, S, nullptr, 0, 0, st, false, false, true))
        return e;
    {
        KTimer tm(ctx, KC_CFPREP, st);
        hipLaunchKernelGGL(k_cf_fold_F, dim3(ceil_div(ns, 4)), dim3(256), 0, st, Zt, ptr<double>(ctx->cfP),
                           ptr<double>(ctx->cfC), S, qp, ns, ptr<double>(ctx->cfF));
        LAUNCHCHK();
    }
    const int nt = ceil_div(S, 64);
    KTimer tm(ctx, KC_CFK, st);
    hipLaunchKernelGGL(k_cf_fold_K, dim3(nt, nt, ns), dim3(256), 0, st, ptr<double>(ctx->Kmat), Zt, ptr<double>(ctx->cfF),
                       S, qp, ptr<double>(ctx->cfK));
    LAUNCHCHK();
    return 0;
}

// The fits' own Y of a batch: ngc splits of the prepared group x mb permutations (d_perm [mb][S], or nullptr: the
// identity, mb = 1), into Ys [ngc mb][S][T]
int cf_fold_Y(plsx_ctx* ctx, int ngc, const int32_t* d_perm, int mb, double* Ys, hipStream_t st)
{
    const int nfit = ngc * mb;
    KTimer tm(ctx, KC_CFY, st);
    hipLaunchKernelGGL(k_cf_fold_Y, dim3(ceil_div(nfit, 4)), dim3(256), 0, st, ptr<double>(ctx->Y),
                       ptr<double>(ctx->cfZ), ptr<double>(ctx->cfP), d_perm, ctx->S, ctx->T, ctx->cf_q + 1, mb, nfit, Ys);
    LAUNCHCHK();
    return 0;
}

// The training masks of the fits of such a batch: fit f takes the mask of split f / mb of the group
int cf_expand_masks(plsx_ctx* ctx, const uint8_t* d_masks, int mb, int nfit, uint8_t* pmask, hipStream_t st)
{
    KTimer tm(ctx, KC_CFY, st);
    hipLaunchKernelGGL(k_cf_expand_masks, dim3(ceil_div(ctx->S, 256), nfit), dim3(256), 0, st, d_masks, ctx->S, mb, pmask);
    LAUNCHCHK();
    return 0;
}

// The scores [ngc][mb] of a batch, added split by split to the mb permutations' outputs (k_cf_cvp_acc)
int cf_cvp_acc(plsx_ctx* ctx, const double* r, const double* r2, const double* sse, int ngc, int mb, int n, bool last,
               double* out_r, double* out_r2, double* out_mse, hipStream_t st)
{
    const int k = ctx->ncomp, T = ctx->T;
    hipLaunchKernelGGL(k_cf_cvp_acc, dim3(ceil_div(2 * k * T + k + 1, 256), mb), dim3(256), 0, st, r, r2, sse,
                       ptr<double>(ctx->cfnte), k, T, ngc, mb, n, last ? 1 : 0, out_r, out_r2, out_mse);
    LAUNCHCHK();
    return 0;
}

}  // namespace plsxi

extern "C" {

int plsx_simpls_set_confounds(plsx_ctx* ctx, const double* d_Z, int q, double* d_gx, double* d_gy, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_set_confounds: data not bound for regression");
    if (!d_Z || q < 1 || q > CF_Q - 1)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_set_confounds: null confounds or q outside 1 .. 15");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    const int S = ctx->S, T = ctx->T, qp = q + 1;
    ctx->cf_q = 0;
    if (int e = ensure(ctx, ctx->cfZ, (size_t)CF_Q * S * 8)) return e;
    if (int e = ensure(ctx, ctx->cfL, (size_t)CF_Q * CF_Q * 8)) return e;
    if (int e = ensure(ctx, ctx->cfstat, sizeof(int))) return e;
    HIPCHK(hipMemsetAsync(ctx->cfZ.p, 0, (size_t)CF_Q * S * 8, st));
    double* Zt = ptr<double>(ctx->cfZ);
    int bad = 0;
    {
        KTimer tm(ctx, KC_CFRESID, st);
        hipLaunchKernelGGL(k_cf_ztilde, dim3(qp), dim3(256), 0, st, d_Z, q, S,
                           ctx->has_okx ? ptr<uint8_t>(ctx->okx) : nullptr, ctx->has_oky ? ptr<uint8_t>(ctx->oky) : nullptr,
                           Zt);
        LAUNCHCHK();
        hipLaunchKernelGGL(k_cf_chol, dim3(1), dim3(64), 0, st, Zt, S, qp, ptr<double>(ctx->cfL), ptr<int>(ctx->cfstat));
        LAUNCHCHK();
    }
    HIPCHK(hipMemcpyAsync(&bad, ctx->cfstat.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bad)                                           // (nothing of the binding has been touched yet)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_set_confounds: the confounds (with the intercept) are rank deficient "
                                       "on the usable rows");
    {
        KTimer tm(ctx, KC_CFRESID, st);
        hipLaunchKernelGGL(k_cf_resid, dim3(ceil_div(ctx->B, 256)), dim3(256), 0, st, ptr<double>(ctx->Xc), ctx->Bpad,
                           ctx->B, S, Zt, qp, ptr<double>(ctx->cfL), d_gx, ctx->B);
        LAUNCHCHK();
        hipLaunchKernelGGL(k_cf_resid, dim3(ceil_div(T, 256)), dim3(256), 0, st, ptr<double>(ctx->Y), T, T, S, Zt, qp,
                           ptr<double>(ctx->cfL), d_gy, T);
        LAUNCHCHK();
    }
    // K_r from X_r itself: an update of K would cancel where the confounds carry most of the variance
    if (int e = simpls_form_K(ctx, st)) return e;
    ctx->has_shrsum = 0;                               // (the row sums of Xc belong to the data as they were)
    HIPCHK(hipStreamSynchronize(st));
    ctx->cf_q = q;
    return PLSX_OK;
} PLSX_CATCH(ctx)

}  // extern "C"
