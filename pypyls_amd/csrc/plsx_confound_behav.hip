// plsx_confound_behav.hip -- confound regression of the behavioural PLS-C front end: plsx_residualize,
// plsx_set_confounds, and what the two fold entries (plsx_crossval_confound_batch / plsx_crossval_confound_perm_batch,
// bodies in plsx_cvperm.hip) launch per group of splits (plsx_k_confound_behav.h)
// Part of libplsx.so (plsx_internal.h has the map of translation units).  gfx950 only.
#include "plsx_internal.h"
#include "plsx_k_confound_behav.h"
using namespace plsxi;

namespace {

// device memory of one stateless call
struct Scratch {
    Buf Zt, Inv, stat;
    ~Scratch() { for (Buf* b : {&Zt, &Inv, &stat}) release(*b); }
};

// Z~ = [1, Z - zbar] over all S rows into Zt [CF_Q][S] (zero rows beyond q'), (Z~ Z~^T)^-1 into Inv; *bad = 1: rank
// deficient
int ztilde_and_inverse(plsx_ctx* ctx, const double* d_Z, int q, int S, double* Zt, double* Inv, int* stat, int* bad,
                       hipStream_t st)
{
    HIPCHK(hipMemsetAsync(Zt, 0, (size_t)CF_Q * S * 8, st));
    {
        KTimer tm(ctx, KC_CFRESID, st);
        hipLaunchKernelGGL(k_cf_ztilde, dim3(q + 1), dim3(256), 0, st, d_Z, q, S, (const uint8_t*)nullptr,
                           (const uint8_t*)nullptr, Zt);
        LAUNCHCHK();
        hipLaunchKernelGGL(k_cf_chol, dim3(1), dim3(64), 0, st, (const double*)Zt, S, q + 1, Inv, stat);
        LAUNCHCHK();
    }
    HIPCHK(hipMemcpyAsync(bad, stat, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

namespace plsxi {

// P_s and the usable test rows of ALL n splits of a call (ctx->cfP [n][q'][S], ctx->cfnte); a split on whose training
// rows Z~ is rank deficient is refused by index (PLSX_ERR_ARG) before anything feature-sized is formed
int cfb_prepare(plsx_ctx* ctx, const char* who, const uint8_t* d_masks, int n, hipStream_t st)
{
    const int S = ctx->S, qp = ctx->cf_q + 1;
    if (int e = ensure(ctx, ctx->cfP, (size_t)n * qp * S * 8)) return e;
    if (int e = ensure(ctx, ctx->cfnte, (size_t)n * 8)) return e;
    if (int e = ensure(ctx, ctx->cfstat, (size_t)n * sizeof(int))) return e;
    {
        KTimer tm(ctx, KC_CFPREP, st);
        hipLaunchKernelGGL(k_cf_fold_prep, dim3(ceil_div(n, 4)), dim3(256), 0, st, ptr<double>(ctx->cfZ), d_masks, S, qp, n,
                           ptr<double>(ctx->cfP), ptr<double>(ctx->cfnte), ptr<int>(ctx->cfstat));
        LAUNCHCHK();
    }
    std::vector<int> bad(n);
    HIPCHK(hipMemcpyAsync(bad.data(), ctx->cfstat.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int s = 0; s < n; ++s)
        if (bad[s]) {
            char msg[240];
            snprintf(msg, sizeof msg, "%s: the confounds (with the intercept) are rank deficient on the training rows of "
                     "split %d", who, s);
            return fail(ctx, PLSX_ERR_ARG, msg);
        }
    return 0;
}

// X_s = M_s X_r of the g splits s0 .. of the call, into Xf [g][S][Bpad], CFB_G splits a launch
int cfb_fold_X(plsx_ctx* ctx, int s0, int g, double* Xf, hipStream_t st)
{
    const int S = ctx->S, qp = ctx->cf_q + 1, ldx = ctx->Bpad;
    KTimer tm(ctx, KC_CFBX, st);
    for (int a = 0; a < g; a += CFB_G) {
        const int ng = std::min(CFB_G, g - a);
        // q' <= 8: half the accumulators and twice the rows in flight (the same sums in the same order)
        auto kern = qp <= 8 ? k_cfb_fold_X<8, 8> : k_cfb_fold_X<CF_Q, 4>;
        hipLaunchKernelGGL(kern, dim3(ceil_div(ldx, 256)), dim3(256), 0, st, ptr<double>(ctx->Xc), ldx, ctx->B, S,
                           ptr<double>(ctx->cfZ), ptr<double>(ctx->cfP) + (size_t)(s0 + a) * qp * S, qp, ng,
                           Xf + (size_t)a * S * ldx);
        LAUNCHCHK();
    }
    return 0;
}

// The fits' own Y, into Ys [nfit][S][T]: fit f is split s + f / mb of the call under permutation f % mb (d_perm [mb][S]),
// Y_{s,p} = M_s (Y_r[perm_p]); d_perm == nullptr, mb = 1: the identity, Y_s of nfit consecutive splits
int cfb_fold_Y(plsx_ctx* ctx, int s, const int32_t* d_perm, int mb, int nfit, double* Ys, hipStream_t st)
{
    const int S = ctx->S, qp = ctx->cf_q + 1;
    KTimer tm(ctx, KC_CFY, st);
    hipLaunchKernelGGL(k_cf_fold_Y, dim3(ceil_div(nfit, 4)), dim3(256), 0, st, ptr<double>(ctx->Y), ptr<double>(ctx->cfZ),
                       ptr<double>(ctx->cfP) + (size_t)s * qp * S, d_perm, S, ctx->T, qp, mb, nfit, Ys);
    LAUNCHCHK();
    return 0;
}

int cfb_identity(plsx_ctx* ctx, int* idx, int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_cfb_identity, dim3(ceil_div(ctx->S, 256), n), dim3(256), 0, st, idx, ctx->S, n);
    LAUNCHCHK();
    return 0;
}

}  // namespace plsxi

extern "C" {

int plsx_residualize(plsx_ctx* ctx, double* d_A, int lda, int ncols, int S, const double* d_Z, int q, double* d_slopes,
                     int ld, void* stream)
try {
    if (!ctx) return PLSX_ERR_ARG;
    if (!d_A || !d_Z || S < 1 || ncols < 1 || lda < ncols || (d_slopes && ld < ncols))
        return fail(ctx, PLSX_ERR_ARG, "plsx_residualize: bad arguments");
    if (q < 1 || q > CF_Q - 1) return fail(ctx, PLSX_ERR_ARG, "plsx_residualize: q outside 1 .. 15");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    Scratch sc;
    if (int e = ensure(ctx, sc.Zt, (size_t)CF_Q * S * 8)) return e;
    if (int e = ensure(ctx, sc.Inv, (size_t)CF_Q * CF_Q * 8)) return e;
    if (int e = ensure(ctx, sc.stat, sizeof(int))) return e;
    int bad = 0;
    if (int e = ztilde_and_inverse(ctx, d_Z, q, S, ptr<double>(sc.Zt), ptr<double>(sc.Inv), ptr<int>(sc.stat), &bad, st))
        return e;
    if (bad)                                           // (nothing has been written)
        return fail(ctx, PLSX_ERR_ARG, "plsx_residualize: the confounds (with the intercept) are rank deficient");
    {
        KTimer tm(ctx, KC_CFRESID, st);
        hipLaunchKernelGGL(k_cf_resid, dim3(ceil_div(ncols, 256)), dim3(256), 0, st, d_A, lda, ncols, S,
                           (const double*)ptr<double>(sc.Zt), q + 1, (const double*)ptr<double>(sc.Inv), d_slopes, ld);
        LAUNCHCHK();
    }
    HIPCHK(hipStreamSynchronize(st));                  // the call's own scratch goes when it returns
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_set_confounds(plsx_ctx* ctx, const double* d_Z, int q, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_BEHAVIORAL)
        return fail(ctx, PLSX_ERR_ARG, "plsx_set_confounds: the fold-wise confound regression is defined for behavioral PLS");
    if (!d_Z || q < 1 || q > CF_Q - 1)
        return fail(ctx, PLSX_ERR_ARG, "plsx_set_confounds: null confounds or q outside 1 .. 15");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    ctx->cf_q = 0;
    if (int e = ensure(ctx, ctx->cfZ, (size_t)CF_Q * ctx->S * 8)) return e;
    if (int e = ensure(ctx, ctx->cfL, (size_t)CF_Q * CF_Q * 8)) return e;
    if (int e = ensure(ctx, ctx->cfstat, sizeof(int))) return e;
    int bad = 0;
    if (int e = ztilde_and_inverse(ctx, d_Z, q, ctx->S, ptr<double>(ctx->cfZ), ptr<double>(ctx->cfL), ptr<int>(ctx->cfstat),
                                   &bad, st))
        return e;
    if (bad)
        return fail(ctx, PLSX_ERR_ARG, "plsx_set_confounds: the confounds (with the intercept) are rank deficient");
    ctx->cf_q = q;
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_crossval_confound_group(plsx_ctx* ctx)
try {
    return ctx ? ctx->cfb_group_l : 0;
} PLSX_CATCH(ctx)

int plsx_crossval_confound_batch(plsx_ctx* ctx, const uint8_t* d_masks, int m, double* d_r, double* d_r2, double* d_lv,
                                 void* stream)
try {
    NEED_DATA();
    return cvperm_fold_entry(ctx, "plsx_crossval_confound_batch", d_masks, m, nullptr, 1, d_r, d_r2, d_lv, nullptr, true,
                             stream);
} PLSX_CATCH(ctx)

int plsx_crossval_confound_perm_batch(plsx_ctx* ctx, const uint8_t* d_masks, int n, const int32_t* d_perm_idx, int m,
                                      double* d_r, double* d_r2, double* d_lv, double* d_lv_pairs, void* stream)
try {
    NEED_DATA();
    return cvperm_fold_entry(ctx, "plsx_crossval_confound_perm_batch", d_masks, n, d_perm_idx, m, d_r, d_r2, d_lv,
                             d_lv_pairs, false, stream);
} PLSX_CATCH(ctx)

}  // extern "C"
