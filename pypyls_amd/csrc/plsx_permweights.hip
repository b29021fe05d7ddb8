// plsx_permweights.hip -- permutation test of the PLS-C x_weights: plsx_perm_weights_build (the subject-space operands
// W_p of the null Z_p = R_p^T V0 = W_p . Xf), plsx_perm_weights_test (W in pieces, then the counting feature pass of the
// SIMPLS coefficients, k_coef_perm_prod / k_coef_perm_max, over Xf)
// Part of libplsx.so (plsx_internal.h has the map of translation units).  gfx950 only.
#include "plsx_internal.h"
#include "plsx_k_permweights.h"

using namespace plsxi;

namespace plsxi {

// the shared refusals of both entries; 0 when the binding takes them
static int pw_check(plsx_ctx* ctx, const char* who, const void* idx, int n, const void* V, int m)
{
    if (ctx->method == PLSX_REGRESSION) return fail(ctx, PLSX_ERR_STATE, std::string(who) + ": data not bound for PLS-C");
    if (ctx->method == PLSX_MULTIBLOCK)
        return fail(ctx, PLSX_ERR_UNSUPPORTED, std::string(who) + ": not available for multiblock PLS");
    if (!idx || !V || n < 1) return fail(ctx, PLSX_ERR_ARG, std::string(who) + ": null pointer or n < 1");
    if (m < 1 || m > ctx->Tp) {
        char msg[160];
        snprintf(msg, sizeof msg, "%s: m = %d outside 1 .. T' = %d", who, m, ctx->Tp);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    return 0;
}

// Xf, the resample-independent feature matrix of the binding in the layout of Xc: Xn (the per-cell scaled X) in
// correlation mode -- what the fixed-X binding keeps; a binding without it (option "no_fixed_x") gets it here, once --
// else the centred X
static int pw_features(plsx_ctx* ctx, hipStream_t st, const double** Xf)
{
    if (ctx->method != PLSX_BEHAVIORAL || ctx->cov) { *Xf = ptr<double>(ctx->Xc); return 0; }
    if (!ctx->has_Xn && !ctx->pw_Xn) {
        const size_t xbytes = (size_t)ctx->Kpad * ctx->Bpad * 8;
        if (int e = ensure(ctx, ctx->Xn, xbytes)) return e;
        KTimer tm(ctx, KC_MOM, st);
        HIPCHK(hipMemsetAsync(ctx->Xn.p, 0, xbytes, st));
        hipLaunchKernelGGL(k_cell_scale, dim3(ceil_div(ctx->B, 256)), dim3(256), 0, st, ptr<double>(ctx->Xc), ctx->Bpad,
                           ctx->B, ctx->J, ptr<int>(ctx->cell_start), ptr<int>(ctx->cell_len), ptr<double>(ctx->Xn));
        LAUNCHCHK();
        ctx->pw_Xn = 1;
    }
    *Xf = ptr<double>(ctx->Xn);
    return 0;
}

// mean-centred PLS: VA = V0^T A (m x S) of the design into ctx->pwVA -- the same for every permutation of a call
static int pw_design(plsx_ctx* ctx, const double* d_V, int m, hipStream_t st)
{
    const int S = ctx->S, Tp = ctx->Tp, Sd = round_up(S, 8);
    if (int e = ensure(ctx, ctx->pwA, (size_t)Tp * Sd * 8)) return e;
    if (int e = ensure(ctx, ctx->pwVA, (size_t)m * S * 8)) return e;
    GroupLayout lay;
    memset(&lay, 0, sizeof(lay));
    lay.n = 1; lay.Tp = Tp; lay.J = ctx->J; lay.T = ctx->T; lay.MT = ctx->MT; lay.Tpp = ctx->Tpp;
    KTimer tm(ctx, KC_BUILD, st);
    HIPCHK(hipMemsetAsync(ctx->pwA.p, 0, (size_t)Tp * Sd * 8, st));
    hipLaunchKernelGGL(k_build_A_mc, dim3(1), dim3(256), 0, st, S, ctx->J, ctx->n_cond, ctx->mc, ptr<int>(ctx->cell_of_row),
                       (const int*)nullptr, lay, ptr<double>(ctx->pwA), (size_t)0, Sd, 0);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_perm_VA, dim3(ceil_div(S, 256), m), dim3(256), 0, st, ptr<double>(ctx->pwA), Sd, S, ctx->J, d_V, m,
                       ptr<double>(ctx->pwVA));
    LAUNCHCHK();
    return 0;
}

// W [n][m][S] of the n index rows at d_idx (mean-centred PLS: after pw_design)
static int pw_build(plsx_ctx* ctx, const int32_t* d_idx, int n, const double* d_V, int m, double* d_W, hipStream_t st)
{
    const int S = ctx->S;
    if (ctx->method == PLSX_BEHAVIORAL) {
        const int T = ctx->T;
        const size_t lds = build_A_proj_lds(T, m);
        const bool vlds = build_A_proj_vlds(T, m);
        auto kern = vlds ? k_perm_W_behav<true> : k_perm_W_behav<false>;
        HIPCHK(set_lds(kern, lds));
        KTimer tm(ctx, KC_BUILD, st);
        hipLaunchKernelGGL(kern, dim3(n, ctx->J), dim3(256), lds, st, ptr<double>(ctx->Y), T, S, ptr<int>(ctx->cell_start),
                           ptr<int>(ctx->cell_len), d_idx, d_V, m, ctx->cov, d_W);
        LAUNCHCHK();
        return 0;
    }
    if (int e = ensure(ctx, ctx->pwInv, (size_t)n * 2 * S * sizeof(int))) return e;
    KTimer tm(ctx, KC_BUILD, st);
    hipLaunchKernelGGL(k_perm_W_mc, dim3(n), dim3(256), 0, st, d_idx, S, ptr<double>(ctx->pwVA), m, ptr<int>(ctx->pwInv), d_W);
    LAUNCHCHK();
    return 0;
}

// the table 1 / s_f of the bound features into ctx->pwRsd (k_col_rsd), once per binding
static int pw_scale(plsx_ctx* ctx, hipStream_t st)
{
    if (ctx->pw_rsd) return 0;
    if (int e = ensure(ctx, ctx->pwRsd, (size_t)ctx->Bpad * 8)) return e;
    KTimer tm(ctx, KC_COEFPROD, st);
    hipLaunchKernelGGL(k_col_rsd, dim3(ceil_div(ctx->Bpad, 256)), dim3(256), 0, st, ptr<double>(ctx->Xc), ctx->Bpad, ctx->S,
                       ctx->B, ptr<double>(ctx->pwRsd));
    LAUNCHCHK();
    ctx->pw_rsd = 1;
    return 0;
}

}  // namespace plsxi

extern "C" {

int plsx_perm_weights_build(plsx_ctx* ctx, const int32_t* d_perm_idx, int n, const double* d_V, int m, double* d_W,
                            void* stream)
try {
    NEED_DATA();
    if (int e = pw_check(ctx, "plsx_perm_weights_build", d_perm_idx, n, d_V, m)) return e;
    if (!d_W) return fail(ctx, PLSX_ERR_ARG, "plsx_perm_weights_build: null pointer or n < 1");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    if (ctx->method == PLSX_MEANCENTERED)
        if (int e = pw_design(ctx, d_V, m, st)) return e;
    // (the grid's x takes any n; a piece of 16384 keeps the index workspace of the mean-centred builder small)
    for (int p0 = 0; p0 < n; p0 += 16384) {
        const int np = std::min(16384, n - p0);
        if (int e = pw_build(ctx, d_perm_idx + (size_t)p0 * ctx->S, np, d_V, m, d_W + (size_t)p0 * m * ctx->S, st)) return e;
    }
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_perm_weights_scale(plsx_ctx* ctx, double* d_rsd, void* stream)
try {
    NEED_DATA();
    if (ctx->method == PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_perm_weights_scale: data not bound for PLS-C");
    if (!d_rsd) return fail(ctx, PLSX_ERR_ARG, "plsx_perm_weights_scale: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    if (int e = pw_scale(ctx, st)) return e;
    HIPCHK(hipMemcpyAsync(d_rsd, ctx->pwRsd.p, (size_t)ctx->B * 8, hipMemcpyDeviceToDevice, st));
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_perm_weights_test(plsx_ctx* ctx, const int32_t* d_perm_idx, int n, const double* d_V, int m, const double* d_obs,
                           int standardise, int32_t* d_count, double* d_max, void* stream)
try {
    NEED_DATA();
    if (int e = pw_check(ctx, "plsx_perm_weights_test", d_perm_idx, n, d_V, m)) return e;
    if (!d_obs || !d_count || !d_max) return fail(ctx, PLSX_ERR_ARG, "plsx_perm_weights_test: null pointer or n < 1");
    const int S = ctx->S, B = ctx->B;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    // What the pass keeps on the device: the stack W of a piece of permutations (8 m S bytes each) and, per 128-feature
    // block of a chunk, the piece's partial maxima (8 m bytes a permutation) -- inside the scratch budget and in free
    // device memory (what an earlier pass left allocated counts as free).  A piece is at most 16384 permutations; one
    // that does not fit with one block of maxima shrinks to whole 64-permutation tiles.
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const double have = (double)free_b + (double)ctx->pwW.bytes + (double)ctx->cppart.bytes;
    const double budget = std::min(ctx->scratch_gb * 1073741824.0, have);
    const double per_perm = 8.0 * m * ((double)S + 1.0);          // a permutation's W and its maxima of one block
    long long piece = std::min(n, 16384);
    if (per_perm * (double)piece > budget) piece = (long long)(budget / per_perm) / 64 * 64;
    if (piece < 1) {
        char msg[400];
        snprintf(msg, sizeof msg, "plsx_perm_weights_test: the operands of 64 permutations (8 m S = %.0f bytes each for "
                 "m = %d, S = %d) with their partial maxima of one 128-feature block (8 m = %d bytes each) need %.0f bytes; "
                 "the scratch budget is %.0f bytes and %.0f bytes of device memory are free", 8.0 * m * S, m, S, 8 * m,
                 64.0 * per_perm, ctx->scratch_gb * 1073741824.0, have);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    const double wbytes = 8.0 * m * (double)S * (double)piece;
    const double room = std::min(budget - wbytes, 2147483648.0);
    const int nfb_all = ceil_div(B, 128);
    const int nfb = (int)std::max<long long>(1, std::min<long long>(nfb_all, (long long)(room / (8.0 * m * (double)piece))));
    if (int e = ensure(ctx, ctx->pwW, (size_t)wbytes)) return e;
    if (int e = ensure(ctx, ctx->cppart, (size_t)nfb * m * (size_t)piece * 8)) return e;
    const double* Xf = nullptr;
    if (int e = pw_features(ctx, st, &Xf)) return e;
    if (standardise)
        if (int e = pw_scale(ctx, st)) return e;
    if (ctx->method == PLSX_MEANCENTERED)
        if (int e = pw_design(ctx, d_V, m, st)) return e;
    CoefPermArgs a;
    a.Xc = Xf; a.ldx = ctx->Bpad;
    a.A = ptr<double>(ctx->pwW);
    a.S = S; a.T = m; a.B = B;
    a.obs = d_obs; a.sd = standardise ? ptr<double>(ctx->pwRsd) : nullptr;
    a.count = d_count; a.pmax = ptr<double>(ctx->cppart);
    for (long long p0 = 0; p0 < n; p0 += piece) {
        a.n = (int)std::min<long long>(piece, n - p0);
        if (int e = pw_build(ctx, d_perm_idx + (size_t)p0 * S, a.n, d_V, m, ptr<double>(ctx->pwW), st)) return e;
        for (int fb0 = 0; fb0 < nfb_all; fb0 += nfb) {
            const int nb = std::min(nfb, nfb_all - fb0);
            a.f0 = fb0 * 128; a.fc = std::min(nb * 128, B - a.f0);
            KTimer tm(ctx, KC_COEFPROD, st);
            hipLaunchKernelGGL(k_coef_perm_prod, dim3(nb, m), dim3(256), 0, st, a);
            LAUNCHCHK();
            hipLaunchKernelGGL(k_coef_perm_max, dim3((unsigned)(((long long)m * a.n + 255) / 256)), dim3(256), 0, st,
                               a.pmax, nb, m, a.n, fb0 == 0 ? 1 : 0, d_max + (size_t)p0 * m);
            LAUNCHCHK();
        }
    }
    return PLSX_OK;
} PLSX_CATCH(ctx)

}  // extern "C"
