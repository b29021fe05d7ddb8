// plsx_weightsci.hip -- percentile intervals of the PLS-C x_weights: plsx_boot_keep (the rotation operands of the
// bootstraps, kept), plsx_boot_weights_ci (the closing pass over a kept stack: dual weights, scale table, k_weights_prod,
// selection)
// Part of libplsx.so (plsx_internal.h has the map of translation units).  gfx950 only.
#include "plsx_internal.h"

using namespace plsxi;

namespace plsxi {

int wkeep_append(plsx_ctx* ctx, int m, hipStream_t st)
{
    if (!ctx->wkeep) return 0;
    // (plsx_boot_batch checked the room of the whole call before it computed anything)
    KTimer tm(ctx, KC_BUILD, st);
    hipLaunchKernelGGL(k_keep_M, dim3(m), dim3(256), 0, st, ptr<double>(ctx->Mfrag), ctx->nks_t, ctx->LT, ctx->Tp,
                       ctx->wkeep_m, ctx->wkeep + (size_t)ctx->wkeep_n * ctx->wkeep_m * ctx->Tp);
    LAUNCHCHK();
    ctx->wkeep_n += m;
    return 0;
}

// bootstraps per batch of the dense A operands (T' x round_up(S, 8) doubles each): 256 MB of them at most
static int wci_abatch(const plsx_ctx* ctx, int n)
{
    const long long per = (long long)ctx->Tp * round_up(ctx->S, 8) * 8;
    return (int)std::max<long long>(1, std::min<long long>(n, (256LL << 20) / per));
}

// W [n][mk][S] = M_b^T A_b of every bootstrap: the A operands are rebuilt from the index rows by the builders of the
// bootstrap routes, dense, a batch at a time
static int wci_build_W(plsx_ctx* ctx, const int32_t* d_idx, const double* d_M, int n, int mk, hipStream_t st)
{
    const int S = ctx->S, Tp = ctx->Tp, Sd = round_up(S, 8);
    const int nb = wci_abatch(ctx, n);
    if (int e = ensure(ctx, ctx->Ad, (size_t)nb * Tp * Sd * 8)) return e;
    GroupLayout lay;
    memset(&lay, 0, sizeof(lay));
    lay.n = 1; lay.Tp = Tp; lay.J = ctx->J; lay.T = ctx->T; lay.MT = ctx->MT; lay.Tpp = ctx->Tpp;
    const size_t wlds = (size_t)mk * Tp * 8;
    HIPCHK(set_lds(k_weights_W, wlds));
    for (int off = 0; off < n; off += nb) {
        const int m = std::min(nb, n - off);
        const int* idx = d_idx + (size_t)off * S;
        KTimer tm(ctx, KC_BUILD, st);
        HIPCHK(hipMemsetAsync(ctx->Ad.p, 0, (size_t)m * Tp * Sd * 8, st));
        int cap = 0;
        if (ctx->method == PLSX_BEHAVIORAL) {
            const size_t lds = build_lds_behav(ctx, &cap);
            hipLaunchKernelGGL(k_build_A_behav, dim3(m, ctx->J), dim3(256), lds, st,
                               ptr<double>(ctx->Y), 0LL, ctx->T, S, ptr<int>(ctx->cell_start),
                               ptr<int>(ctx->cell_len), idx, idx, lay, ctx->cov, 0, ptr<double>(ctx->Ad),
                               (size_t)0, (double*)nullptr, 0, Sd, (double*)nullptr, (size_t)0, (const int*)nullptr,
                               PLSX_MOM_PAIRS, cap);
        } else {
            const size_t lds = build_lds_mc(ctx, &cap);
            hipLaunchKernelGGL(k_build_A_mc, dim3(m), dim3(256), lds, st, S, ctx->J, ctx->n_cond, ctx->mc,
                               ptr<int>(ctx->cell_of_row), idx, lay, ptr<double>(ctx->Ad), (size_t)0, Sd, cap);
        }
        LAUNCHCHK();
        hipLaunchKernelGGL(k_weights_W, dim3(m), dim3(256), wlds, st, ptr<double>(ctx->Ad), Sd, S, Tp, mk,
                           d_M + (size_t)off * mk * Tp, ptr<double>(ctx->wciW) + (size_t)off * mk * S);
        LAUNCHCHK();
    }
    return 0;
}

}  // namespace plsxi

extern "C" {

int plsx_boot_keep(plsx_ctx* ctx, double* d_M, long long capacity, int m)
try {
    if (!ctx) return PLSX_ERR_ARG;
    if (!d_M && capacity == 0 && m == 0) {             // the keeping ends
        wkeep_close(ctx);
        return PLSX_OK;
    }
    NEED_DATA();
    if (ctx->method == PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_boot_keep: data not bound for PLS-C");
    if (ctx->method == PLSX_MULTIBLOCK)
        return fail(ctx, PLSX_ERR_UNSUPPORTED, "plsx_boot_keep: not available for multiblock PLS");
    if (ctx->nc > 0) return fail(ctx, PLSX_ERR_UNSUPPORTED, "plsx_boot_keep: not available with contrasts (non-rotated PLS)");
    if (!ctx->has_orig) return fail(ctx, PLSX_ERR_STATE, "plsx_set_original has not been called");
    if (!d_M || capacity < 1) return fail(ctx, PLSX_ERR_ARG, "plsx_boot_keep: null buffer or capacity < 1");
    if (m < 1 || m > ctx->L) {
        char msg[120];
        snprintf(msg, sizeof msg, "plsx_boot_keep: m = %d outside 1 .. L = %d", m, ctx->L);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    ctx->wkeep = d_M; ctx->wkeep_cap = capacity; ctx->wkeep_n = 0; ctx->wkeep_m = m;
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_boot_weights_ci(plsx_ctx* ctx, const int32_t* d_boot_idx, const double* d_M, int n, int m, int i_lo,
                         double g_lo, int i_hi, double g_hi, double* d_lo, double* d_hi, void* stream)
try {
    NEED_DATA();
    if (ctx->method == PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_boot_weights_ci: data not bound for PLS-C");
    if (ctx->method == PLSX_MULTIBLOCK)
        return fail(ctx, PLSX_ERR_UNSUPPORTED, "plsx_boot_weights_ci: not available for multiblock PLS");
    if (!d_boot_idx || !d_M || !d_lo || !d_hi || n < 1 || i_lo < 0 || i_hi < 0 || i_lo >= n || i_hi >= n)
        return fail(ctx, PLSX_ERR_ARG, "plsx_boot_weights_ci: null pointer, n < 1 or an index outside 0 .. n - 1");
    const int S = ctx->S, B = ctx->B, Tp = ctx->Tp, J = ctx->J;
    char msg[480];
    if (m < 1 || m > ctx->L) {
        snprintf(msg, sizeof msg, "plsx_boot_weights_ci: m = %d outside 1 .. L = %d", m, ctx->L);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    if (n > 16384) {
        snprintf(msg, sizeof msg, "plsx_boot_weights_ci: n = %d bootstraps per series; the percentile kernels take at "
                 "most 16384 (B = %d, m = %d: %.1f GB of series, which no host path forms either)", n, B, m,
                 8.0 * B * m * (double)n / 1073741824.0);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    if ((size_t)m * Tp * 8 > 160 * 1024 - 256) {
        snprintf(msg, sizeof msg, "plsx_boot_weights_ci: m T' = %d x %d doubles of one rotation operand exceed the LDS of "
                 "the dual-weight kernel (20448 doubles)", m, Tp);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    // correlation mode: the features are re-scaled per bootstrap and cell
    const bool scaled = ctx->method == PLSX_BEHAVIORAL && !ctx->cov;
    // What the pass keeps on the device next to the caller's stack: W, the draw counts (scaled), a batch of dense A
    // operands -- and per feature of a chunk its series and (scaled) its J rows of the scale table.  Everything stays
    // inside the scratch budget and in free device memory (what an earlier pass left allocated counts as free); a
    // chunk is whole 128-feature blocks, its series 2 GB at most.
    const long long stack = 8LL * n * m * Tp, wbytes = 8LL * n * m * S, cbytes = scaled ? 4LL * n * S : 0;
    const long long abytes = (long long)wci_abatch(ctx, n) * Tp * round_up(S, 8) * 8;
    const double per_series = 8.0 * (double)n * m, per_feat = per_series + (scaled ? 8.0 * (double)n * J : 0.0);
    const int unit = std::min(B, 128);
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const double have = (double)free_b + (double)ctx->wciW.bytes + (double)ctx->wciCnt.bytes + (double)ctx->wciScale.bytes +
                        (double)ctx->cichunk.bytes + (double)ctx->Ad.bytes;
    const double fixed = (double)(wbytes + cbytes + abytes);
    const double budget = ctx->scratch_gb * 1073741824.0;
    const double need = (double)stack + fixed + unit * per_feat;
    const double room = std::min(budget - (double)stack - fixed, have - fixed);
    if (room < unit * per_feat) {
        snprintf(msg, sizeof msg, "plsx_boot_weights_ci: the stack of n = %d bootstraps (8 n m T' = %lld bytes for m = %d, "
                 "T' = %d), the dual weights (8 n m S = %lld bytes, S = %d), counts and operands (%lld bytes) and the "
                 "smallest chunk of %d features (%.0f bytes of series and scales) need %.0f bytes; the scratch budget is "
                 "%.0f bytes and %.0f bytes of device memory are free", n, stack, m, Tp, wbytes, S, cbytes + abytes, unit,
                 unit * per_feat, need, budget, have);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    long long fc = (long long)(std::min(room / per_feat, 2147483648.0 / per_series));
    fc = std::max<long long>(unit, fc / 128 * 128);
    if (fc >= B) fc = B;
    if (int e = ensure(ctx, ctx->wciW, (size_t)wbytes)) return e;
    if (int e = ensure(ctx, ctx->cichunk, (size_t)((double)fc * per_series))) return e;
    if (scaled) {
        if (int e = ensure(ctx, ctx->wciCnt, (size_t)cbytes)) return e;
        if (int e = ensure(ctx, ctx->wciScale, (size_t)8 * J * (size_t)fc * n)) return e;
        KTimer tm(ctx, KC_BUILD, st);
        HIPCHK(hipMemsetAsync(ctx->wciCnt.p, 0, (size_t)cbytes, st));
        hipLaunchKernelGGL(k_weights_counts, dim3(n), dim3(256), 0, st, d_boot_idx, S, ptr<int>(ctx->wciCnt));
        LAUNCHCHK();
    }
    if (int e = wci_build_W(ctx, d_boot_idx, d_M, n, m, st)) return e;
    WeightsProdArgs a;
    a.Xc = ptr<double>(ctx->Xc); a.ldx = ctx->Bpad;
    a.W = ptr<double>(ctx->wciW);
    a.sc = scaled ? ptr<double>(ctx->wciScale) : nullptr;
    a.cell_start = ptr<int>(ctx->cell_start); a.cell_len = ptr<int>(ctx->cell_len); a.J = J;
    a.S = S; a.mk = m; a.n = n; a.B = B;
    a.out = ptr<double>(ctx->cichunk);
    for (long long f0 = 0; f0 < B; f0 += fc) {
        a.f0 = (int)f0; a.fc = (int)std::min<long long>(fc, B - f0);
        const dim3 grid(ceil_div(a.fc, 128), ceil_div(n, 64), m);
        if (scaled) {
            {
                KTimer tm(ctx, KC_MOM, st);
                hipLaunchKernelGGL(k_weights_scale, dim3(ceil_div(a.fc, 128), ceil_div(n, WS_NB)), dim3(128), 0, st,
                                   a.Xc, a.ldx, B, J, a.cell_start, a.cell_len, ptr<int>(ctx->wciCnt), S, n, a.f0, a.fc,
                                   ptr<double>(ctx->wciScale));
                LAUNCHCHK();
            }
            KTimer tm(ctx, KC_WEIGHTSPROD, st);
            if (J == 1) hipLaunchKernelGGL(k_weights_prod<WP_ONE_CELL>, grid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL(k_weights_prod<WP_CELLS>, grid, dim3(256), 0, st, a);
            LAUNCHCHK();
        } else {
            KTimer tm(ctx, KC_WEIGHTSPROD, st);
            hipLaunchKernelGGL(k_weights_prod<WP_UNSCALED>, grid, dim3(256), 0, st, a);
            LAUNCHCHK();
        }
        if (int e = run_percentile(ctx, a.out, (long long)a.fc * m, n, i_lo, g_lo, i_hi, g_hi,
                                   d_lo + (size_t)f0 * m, d_hi + (size_t)f0 * m, st))
            return e;
    }
    return PLSX_OK;
} PLSX_CATCH(ctx)

}  // extern "C"
