// plsx_cvperm.hip -- permutation null of the behavioural cross-validation in dual space (plsx_crossval_perm_batch)
// Part of libplsx.so (plsx_internal.h has the map of translation units).  gfx950 only.
//
// One S x S matrix per SPLIT (plsx_k_cvperm.h has the algebra) serves every permutation: the feature pass runs once
// per split of a call, never per (permutation, split), and each fit is S x S work -- A (k_cvp_build_A), W' = A M^T
// and G = W' A^T (run_nt), the small solver returning V and d, the scores (k_cvp_final) and, for
// plsx_crossval_perm_lv_batch, the score correlations of the latent variables (k_cvp_lv, on the z k_cvp_final left).
// The fold-wise confound regression (plsx_crossval_confound_batch / _perm_batch, entries in plsx_confound_behav.hip)
// runs the same body on a fold copy X_s per split and a Y_{s,p} per (permutation, split).
// The caller hands ALL of its permutations to one call: a split's matrix lives for the group of splits it was formed
// with and is not kept between calls.
#include "plsx_internal.h"
#include "plsx_k_cvperm.h"

using namespace plsxi;

namespace {

// what the call maps for itself and gives back when it returns: the context's own buffers keep their owners
struct CvpScratch {
    Buf M, mu, inv, part, r, r2, z, ysc, lv;
    Buf Xf, Ys, ident;                                  // fold-wise confound regression: X_s of a group, Y_{s,p} and the identity rows of a pass
    ~CvpScratch() { for (Buf* b : {&M, &mu, &inv, &part, &r, &r2, &z, &ysc, &lv, &Xf, &Ys, &ident}) release(*b); }
};

// Blocks along the contraction of k_cvp_gram: about 1024 blocks per split, at least 512 columns each -- a function
// of (S, B) alone, so a split's bits follow neither the batch, the scratch budget nor the way the call is cut.
void cvp_chunks(int S, int B, int* kchunk, int* nchunk)
{
    const int mt = ceil_div(S, 64);
    int nc = std::max(1, ceil_div(1024, ceil_div(mt, 2) * mt));
    nc = std::min(nc, std::max(1, B / 512));
    *kchunk = round_up(ceil_div(B, nc), NT_KB);
    *nchunk = ceil_div(B, *kchunk);
}

// d_lv (m, L) != nullptr: also the score correlations of the latent variables, their split means to d_lv and the
// (permutation, split) values to d_lv_pairs (m, n, L) when given (else to scratch of the call).
// fold != 0 (the fold-wise confound regression, Z~ bound): split s works on X_s = M_s X_r, a copy of its own formed for
// a group of splits at a time (cfb_fold_X), and permutation p on Y_{s,p} = M_s (Y_r[perm_p]) (cfb_fold_Y), read in
// position order through the kernels' y_stride; fold == 2 (the observed entry): d_perm_idx is nullptr, m = 1, and the
// outputs are the scores of every split, d_r / d_r2 (n, T) and d_lv (n, L), not their mean.  fold == 0 passes every
// kernel exactly what it passed before the argument existed.
int cvperm_impl(plsx_ctx* ctx, const char* who, const uint8_t* d_masks, int n, const int32_t* d_perm_idx, int m,
                double* d_r, double* d_r2, double* d_lv, double* d_lv_pairs, hipStream_t st, int fold = 0)
{
    const int S = ctx->S, B = ctx->B, T = ctx->T, J = ctx->J, Tp = ctx->Tp, L = ctx->L;
    const int Sd = round_up(S, 8), ldt = ctx->Bpad, mt = ceil_div(S, 64);
    int kchunk = 0, nchunk = 0;
    cvp_chunks(S, B, &kchunk, &nchunk);
    const double tiles = (double)mt * mt;
    // bytes of one split (matrix, tables, partial tiles), of one permutation (A, W', G, V, d, z, predictions) and of
    // the scores of the whole call; with the LV correlations one more (S, L) per permutation (the y-scores) and their
    // (m, n, L) values
    const double per_split = (double)S * Sd * 8 + 2.0 * J * ldt * 8 + (double)nchunk * tiles * 4096 * 8 +
                             (fold ? (double)S * ldt * 8 : 0.0) + (fold == 2 ? (double)S * T * 8 : 0.0);
    const size_t mfrag = (size_t)ctx->nks_t * ctx->LT * 64 * 8;     // (the solver also leaves its rotation operand)
    const double per_perm = 2.0 * Tp * Sd * 8 + (double)Tp * Tp * 8 + (double)Tp * L * 8 + (double)L * 8 +
                            (double)S * T * 8 + (double)S * L * 8 + (double)J * T * 8 + (double)mfrag +
                            (d_lv ? (double)S * L * 8 : 0.0) + (fold ? (double)S * T * 8 + (double)S * 4 : 0.0);
    const double fixed = 2.0 * m * (double)n * T * 8 + (d_lv ? (double)m * n * L * 8 : 0.0);
    size_t fre = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fre, &tot));
    const double limit = std::min(ctx->scratch_gb * 1073741824.0, 0.9 * (double)fre);
    if (fixed + per_split + per_perm > limit || (long long)ceil_div(mt, 2) * mt > 65535 ||
        (double)J * ldt >= 2147483648.0) {
        char msg[448];
        snprintf(msg, sizeof msg,
                 "%s: one split (S = %d, B = %d: %.1f MB of matrix, tables and partial tiles%s), one "
                 "permutation's operands (T' = %d: %.1f MB) and the scores of %d x %d fits (%.1f MB) do not fit %.1f MB "
                 "of free device memory and scratch budget",
                 who, S, B, per_split / 1048576.0, fold ? " and its fold copy of X" : "", Tp, per_perm / 1048576.0, m, n, fixed / 1048576.0, limit / 1048576.0);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    // splits per group: half of what is left, 4 GB at most; permutations per pass: the rest, within the operand and
    // grid bounds of the tiled products (as perm_dual)
    const double room = limit - fixed;
    int gs = (int)std::max(1.0, std::min((double)n, std::floor(std::min(0.5 * room, 4294967296.0) / per_split)));
    gs = std::min(gs, 65535);
    long long mb = (long long)std::max(1.0, std::floor((room - gs * per_split) / per_perm));
    mb = std::min<long long>(mb, std::min<long long>(32768, (2LL << 30) / ((long long)Tp * Sd * 8)));
    mb = std::min<long long>(mb, 60000LL * 64 / ((long long)Tp * mt));
    mb = std::max<long long>(1, std::min<long long>(mb, m));

    CvpScratch sc;
    if (fold) {
        // P_s of every split of the call first: a deficient split is refused by index before anything else runs
        if (int e = cfb_prepare(ctx, who, d_masks, n, st)) return e;
        ctx->cfb_group_l = gs;
        if (int e = ensure(ctx, sc.Xf, (size_t)gs * S * ldt * 8)) return e;
        if (int e = ensure(ctx, sc.Ys, (size_t)std::max<long long>(mb, fold == 2 ? gs : 1) * S * T * 8)) return e;
        if (int e = ensure(ctx, sc.ident, (size_t)mb * S * sizeof(int))) return e;
        if (int e = cfb_identity(ctx, ptr<int>(sc.ident), (int)mb, st)) return e;
    }
    const long long ystride = fold ? (long long)S * T : 0;
    if (int e = ensure(ctx, sc.M, (size_t)gs * S * Sd * 8)) return e;
    if (int e = ensure(ctx, sc.mu, (size_t)gs * J * ldt * 8)) return e;
    if (int e = ensure(ctx, sc.inv, (size_t)gs * J * ldt * 8)) return e;
    if (int e = ensure(ctx, sc.part, (size_t)gs * nchunk * mt * mt * 4096 * 8)) return e;
    if (int e = ensure(ctx, sc.r, (size_t)m * n * T * 8)) return e;
    if (int e = ensure(ctx, sc.r2, (size_t)m * n * T * 8)) return e;
    if (int e = ensure(ctx, sc.z, (size_t)mb * S * L * 8)) return e;
    double* lv_pairs = fold == 2 ? d_lv : d_lv_pairs;
    if (d_lv) {
        if (int e = ensure(ctx, sc.ysc, (size_t)mb * S * L * 8)) return e;
        if (!lv_pairs) {
            if (int e = ensure(ctx, sc.lv, (size_t)m * n * L * 8)) return e;
            lv_pairs = ptr<double>(sc.lv);
        }
    }
    const size_t abytes = (size_t)mb * Tp * Sd * 8;
    if (int e = ensure(ctx, ctx->Ad, abytes)) return e;
    if (int e = ensure(ctx, ctx->Wd, abytes)) return e;
    if (int e = ensure(ctx, ctx->Gm, (size_t)mb * Tp * Tp * 8)) return e;
    if (int e = ensure(ctx, ctx->Vs, (size_t)mb * Tp * L * 8)) return e;
    if (int e = ensure(ctx, ctx->ds, (size_t)mb * L * 8)) return e;
    if (int e = ensure(ctx, ctx->Mfrag, (size_t)mb * mfrag + 1024)) return e;
    if (int e = ensure(ctx, ctx->ybar, (size_t)mb * J * T * 8)) return e;
    if (int e = ensure(ctx, ctx->pred, (size_t)mb * S * T * 8)) return e;

    for (int s0 = 0; s0 < n; s0 += gs) {
        const int g = std::min(gs, n - s0);
        const uint8_t* mk = d_masks + (size_t)s0 * S;
        if (fold) {
            // the group's fold copies, then the tables and the matrix of every split from its own copy
            if (int e = cfb_fold_X(ctx, s0, g, ptr<double>(sc.Xf), st)) return e;
            CvpGramArgs a;
            a.ldx = ctx->Bpad; a.S = S; a.K = B; a.ldt = ldt; a.J = J;
            a.cell_of_row = ptr<int>(ctx->cell_of_row); a.cov = ctx->cov;
            a.kchunk = kchunk; a.nchunk = nchunk; a.mtiles = mt;
            for (int s = 0; s < g; ++s) {
                const double* Xs = ptr<double>(sc.Xf) + (size_t)s * S * ldt;
                double* mus = ptr<double>(sc.mu) + (size_t)s * J * ldt;
                double* invs = ptr<double>(sc.inv) + (size_t)s * J * ldt;
                {
                    KTimer tm(ctx, KC_CVPMOM, st);
                    hipLaunchKernelGGL(k_cvp_moments, dim3(ceil_div(B, 256), 1), dim3(256), 0, st, Xs, ctx->Bpad, B, J,
                                       ptr<int>(ctx->cell_start), ptr<int>(ctx->cell_len), mk + (size_t)s * S, S, 1, mus,
                                       invs, ldt);
                    LAUNCHCHK();
                }
                a.X = Xs; a.mu = mus; a.inv = invs; a.masks = mk + (size_t)s * S;
                a.part = ptr<double>(sc.part) + (size_t)s * nchunk * mt * mt * 4096;
                KTimer tm(ctx, KC_CVPGRAM, st);
                hipLaunchKernelGGL(k_cvp_gram, dim3(nchunk, ceil_div(mt, 2) * mt, 1), dim3(256), 0, st, a);
                LAUNCHCHK();
            }
            KTimer tm(ctx, KC_CVPGRAM, st);
            hipLaunchKernelGGL(k_cvp_reduce, dim3((unsigned)(((long long)S * S + 255) / 256), g), dim3(256), 0, st,
                               ptr<double>(sc.part), nchunk, mt, S, ptr<double>(sc.M), Sd);
            LAUNCHCHK();
        } else {
        {
            KTimer tm(ctx, KC_CVPMOM, st);
            hipLaunchKernelGGL(k_cvp_moments, dim3(ceil_div(B, 256), ceil_div(g, CVP_SB)), dim3(256), 0, st,
                               ptr<double>(ctx->Xc), ctx->Bpad, B, J, ptr<int>(ctx->cell_start), ptr<int>(ctx->cell_len),
                               mk, S, g, ptr<double>(sc.mu), ptr<double>(sc.inv), ldt);
            LAUNCHCHK();
        }
        {
            CvpGramArgs a;
            a.X = ptr<double>(ctx->Xc); a.ldx = ctx->Bpad; a.S = S; a.K = B;
            a.mu = ptr<double>(sc.mu); a.inv = ptr<double>(sc.inv); a.ldt = ldt; a.J = J;
            a.cell_of_row = ptr<int>(ctx->cell_of_row); a.masks = mk; a.cov = ctx->cov;
            a.kchunk = kchunk; a.nchunk = nchunk; a.mtiles = mt; a.part = ptr<double>(sc.part);
            KTimer tm(ctx, KC_CVPGRAM, st);
            hipLaunchKernelGGL(k_cvp_gram, dim3(nchunk, ceil_div(mt, 2) * mt, g), dim3(256), 0, st, a);
            LAUNCHCHK();
            hipLaunchKernelGGL(k_cvp_reduce, dim3((unsigned)(((long long)S * S + 255) / 256), g), dim3(256), 0, st,
                               ptr<double>(sc.part), nchunk, mt, S, ptr<double>(sc.M), Sd);
            LAUNCHCHK();
        }
        }
        if (fold == 2)
            if (int e = cfb_fold_Y(ctx, s0, nullptr, 1, g, ptr<double>(sc.Ys), st)) return e;
        for (int s = 0; s < g; ++s) {
            const uint8_t* mks = mk + (size_t)s * S;
            const double* Ms = ptr<double>(sc.M) + (size_t)s * S * Sd;
            for (int p0 = 0; p0 < m; p0 += (int)mb) {
                const int mm = std::min<int>((int)mb, m - p0);
                const int* idx = d_perm_idx ? d_perm_idx + (size_t)p0 * S : nullptr;
                const double* Yp = ptr<double>(ctx->Y);
                if (fold == 2) {
                    Yp = ptr<double>(sc.Ys) + (size_t)s * S * T;       // (Y_s of the whole group: one launch, below)
                    idx = ptr<int>(sc.ident);
                } else if (fold) {
                    if (int e = cfb_fold_Y(ctx, s0 + s, idx, mm, mm, ptr<double>(sc.Ys), st)) return e;
                    Yp = ptr<double>(sc.Ys);
                    idx = ptr<int>(sc.ident);
                }
                HIPCHK(hipMemsetAsync(ctx->Ad.p, 0, (size_t)mm * Tp * Sd * 8, st));
                {
                    KTimer tm(ctx, KC_BUILD, st);
                    hipLaunchKernelGGL(k_cvp_build_A, dim3(mm, J), dim3(256), (size_t)2 * T * 8, st, Yp, T,
                                       S, ptr<int>(ctx->cell_start), ptr<int>(ctx->cell_len), mks, idx, Tp, ctx->cov,
                                       ptr<double>(ctx->Ad), Sd, ystride);
                    LAUNCHCHK();
                }
                // W' = A M^T, all permutations stacked ((mm T') x S); every entry is one block's whole contraction
                {
                    KTimer tm(ctx, KC_CVPW, st);
                    if (int e = run_nt(ctx, ptr<double>(ctx->Ad), 0, Sd, mm * Tp, Ms, 0, Sd, S, nullptr, 0, 0, 0, S, 1,
                                       ptr<double>(ctx->Wd), 0, Sd, nullptr, 0, 0, st, false, false, true))
                        return e;
                }
                // G_p = W'_p A_p^T
                {
                    KTimer tm(ctx, KC_CVPG, st);
                    if (int e = run_nt(ctx, ptr<double>(ctx->Wd), (long long)Tp * Sd, Sd, Tp, ptr<double>(ctx->Ad),
                                       (long long)Tp * Sd, Sd, Tp, nullptr, 0, 0, 0, S, mm, ptr<double>(ctx->Gm),
                                       (long long)Tp * Tp, Tp, nullptr, 0, 0, st, false, false, true))
                        return e;
                }
                SmallArgs a = small_args(ctx, SMALL_DECOMP);
                a.out_V = ptr<double>(ctx->Vs); a.out_d = ptr<double>(ctx->ds);
                if (int e = run_small(ctx, a, mm, st)) return e;
                {
                    KTimer tm(ctx, KC_CVSCORE, st);
                    const size_t o = ((size_t)p0 * n + s0 + s) * T;
                    hipLaunchKernelGGL(k_cvp_final, dim3(mm), dim3(256), 0, st, ptr<double>(ctx->Wd), Sd,
                                       ptr<double>(ctx->Vs), ptr<double>(ctx->ds), Yp, mks, idx,
                                       ptr<int>(ctx->cell_of_row), S, T, J, Tp, L, ptr<double>(ctx->ybar),
                                       ptr<double>(sc.z), ptr<double>(ctx->pred), ptr<double>(sc.r) + o, ptr<double>(sc.r2) + o,
                                       (long long)n * T, ystride);
                    LAUNCHCHK();
                }
                // (the observed fold entry: the split's predictions and its fold-residualised Y go to an open series)
                if (fold == 2)
                    if (int e = cv_pred_export(ctx, ptr<double>(ctx->pred), mks, 1, Yp, 0, s0 + s, st)) return e;
                if (d_lv) {
                    KTimer tm(ctx, KC_CVPLV, st);
                    hipLaunchKernelGGL(k_cvp_lv, dim3(mm), dim3(256), (size_t)2 * J * T * 8, st, ptr<double>(ctx->Vs),
                                       ptr<double>(ctx->ds), Yp, mks, idx, ptr<int>(ctx->cell_of_row),
                                       ptr<int>(ctx->cell_start), ptr<int>(ctx->cell_len), S, T, J, Tp, L, ctx->cov,
                                       ptr<double>(sc.z), ptr<double>(sc.ysc),
                                       lv_pairs + ((size_t)p0 * n + s0 + s) * L, (long long)n * L, ystride);
                    LAUNCHCHK();
                }
            }
        }
    }
    if (fold == 2) {
        // the observed entry: the scores of every split ((1, n, T) = (n, T); d_lv took its values as the pairs)
        HIPCHK(hipMemcpyAsync(d_r, sc.r.p, (size_t)n * T * 8, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(d_r2, sc.r2.p, (size_t)n * T * 8, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        if (ctx->bpred_series.active) ctx->bpred_series.n += n;
        return PLSX_OK;
    }
    // the mean over the splits, in split order (a NaN score makes its permutation's mean NaN)
    {
        KTimer tm(ctx, KC_CVPMEAN, st);
        hipLaunchKernelGGL(k_mean_axis1, dim3(ceil_div(m * T, 256)), dim3(256), 0, st, ptr<double>(sc.r), m, n, T, d_r);
        LAUNCHCHK();
        hipLaunchKernelGGL(k_mean_axis1, dim3(ceil_div(m * T, 256)), dim3(256), 0, st, ptr<double>(sc.r2), m, n, T, d_r2);
        LAUNCHCHK();
        if (d_lv) {
            hipLaunchKernelGGL(k_mean_axis1, dim3(ceil_div(m * L, 256)), dim3(256), 0, st, lv_pairs, m, n, L, d_lv);
            LAUNCHCHK();
        }
    }
    HIPCHK(hipStreamSynchronize(st));                  // the call's own scratch goes when it returns
    return PLSX_OK;
}

// the checks both entries share; `who` names the entry in the messages
int cvperm_entry(plsx_ctx* ctx, const char* who, const uint8_t* d_masks, int n, const int32_t* d_perm_idx, int m,
                 double* d_r, double* d_r2, double* d_lv, double* d_lv_pairs, bool want_lv, void* stream)
{
    const std::string w(who);
    if (ctx->method == PLSX_MULTIBLOCK)
        return fail(ctx, PLSX_ERR_UNSUPPORTED, w + ": cross-validation is not built for multiblock PLS");
    if (ctx->method != PLSX_BEHAVIORAL)
        return fail(ctx, PLSX_ERR_ARG, w + ": cross-validation is defined for behavioral PLS");
    if (!d_masks || !d_perm_idx || !d_r || !d_r2 || (want_lv && !d_lv) || n < 1 || m < 1)
        return fail(ctx, PLSX_ERR_ARG, w + ": bad arguments");
    if (ctx->nc > 0)
        return fail(ctx, PLSX_ERR_UNSUPPORTED, w + ": cross-validation predicts from a fitted "
                                                "decomposition, which non-rotated PLS (contrasts are set) does not have");
    HIPCHK(hipSetDevice(ctx->device));
    return cvperm_impl(ctx, who, d_masks, n, d_perm_idx, m, d_r, d_r2, d_lv, d_lv_pairs, static_cast<hipStream_t>(stream));
}

}  // namespace

namespace plsxi {

int cvperm_fold_entry(plsx_ctx* ctx, const char* who, const uint8_t* d_masks, int n, const int32_t* d_perm_idx, int m,
                      double* d_r, double* d_r2, double* d_lv, double* d_lv_pairs, bool observed, void* stream)
{
    const std::string w(who);
    if (ctx->method == PLSX_MULTIBLOCK)
        return fail(ctx, PLSX_ERR_UNSUPPORTED, w + ": cross-validation is not built for multiblock PLS");
    if (ctx->method != PLSX_BEHAVIORAL)
        return fail(ctx, PLSX_ERR_ARG, w + ": cross-validation is defined for behavioral PLS");
    if (!d_masks || (!observed && !d_perm_idx) || !d_r || !d_r2 || n < 1 || m < 1)
        return fail(ctx, PLSX_ERR_ARG, w + ": bad arguments");
    if (ctx->nc > 0)
        return fail(ctx, PLSX_ERR_UNSUPPORTED, w + ": cross-validation predicts from a fitted "
                                                "decomposition, which non-rotated PLS (contrasts are set) does not have");
    if (!ctx->cf_q) return fail(ctx, PLSX_ERR_STATE, w + ": no confounds are bound (plsx_set_confounds)");
    if (observed)
        if (int e = cv_pred_reserve(ctx, who, n)) return e;
    HIPCHK(hipSetDevice(ctx->device));
    return cvperm_impl(ctx, who, d_masks, n, observed ? nullptr : d_perm_idx, m, d_r, d_r2, d_lv, d_lv_pairs,
                       static_cast<hipStream_t>(stream), observed ? 2 : 1);
}

}  // namespace plsxi

extern "C" {

int plsx_crossval_perm_batch(plsx_ctx* ctx, const uint8_t* d_masks, int n, const int32_t* d_perm_idx, int m,
                             double* d_r, double* d_r2, void* stream)
try {
    NEED_DATA();
    return cvperm_entry(ctx, "plsx_crossval_perm_batch", d_masks, n, d_perm_idx, m, d_r, d_r2, nullptr, nullptr, false,
                        stream);
} PLSX_CATCH(ctx)

int plsx_crossval_perm_lv_batch(plsx_ctx* ctx, const uint8_t* d_masks, int n, const int32_t* d_perm_idx, int m,
                                double* d_r, double* d_r2, double* d_lv, double* d_lv_pairs, void* stream)
try {
    NEED_DATA();
    return cvperm_entry(ctx, "plsx_crossval_perm_lv_batch", d_masks, n, d_perm_idx, m, d_r, d_r2, d_lv, d_lv_pairs, true,
                        stream);
} PLSX_CATCH(ctx)

}  // extern "C"
