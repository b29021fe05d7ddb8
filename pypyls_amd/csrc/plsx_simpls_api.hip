// plsx_simpls_api.hip -- SIMPLS regression (pyls/types/regression.py): dual-space solver batches, permutations, bootstraps
// Part of libplsx.so (plsx_internal.h has the map of translation units).  gfx950 only.
#include "plsx_internal.h"
#include "plsx_simpls.h"
using namespace plsxi;

namespace plsxi {

// Route of the component-step kernels.  On-chip: a wave's LDS slice holds its resample's S-long scatter buffer
// (sd_step_lds, at most 158 KB of a CU's 160).  Global (the `simpls_global` option, or S beyond that bound): the
// S-long data stay in the resample's scratch and the scatter reads the tables sfirst / scnt there; the LDS slice keeps
// the T x T work (sd_step_lds_global), which bounds T alone.
bool simpls_onchip_fits(int S, int T, int k) { return sd_step_lds(S, T, k) * 8 <= 158 * 1024; }
size_t simpls_global_lds_bytes(int T, int k) { return sd_step_lds_global(T, k) * 8; }
static bool simpls_global(const plsx_ctx* ctx)
{
    return ctx->opt[OPT_SIMPLS_GLOBAL] != 0 || !simpls_onchip_fits(ctx->S, ctx->T, ctx->ncomp);
}

// doubles of run_simpls_dual's scratch per resample: the state carved out below plus the two GEMM operands
static size_t sd_scratch_doubles(int S, int T, int k, bool gl)
{
    const size_t per = (size_t)S /* xs, ys as ints share one S-double slot */ + 2 * (size_t)S * T + 4 * (size_t)k * S +
                       2 * (size_t)S + 2 * (size_t)T * T + 2 * (size_t)k * T + 4 + (size_t)T +
                       (gl ? (size_t)S : 0) /* sfirst, scnt */;
    return per + 2 * (size_t)(T + 1) * S;
}

// Resamples per solver batch.  Up to `want` (the on-chip route's fixed 8192, see the batch entries) when they fit half
// the scratch budget -- every shape of the on-chip route at the default 48 GB, so their batches are what they always
// were -- otherwise as many whole groups of `unit` resamples as fit it (S = 24 000, T = 20, k = 15: 28 MB of state per
// resample; 8192 of them would need 230 GB).  `extra`: bytes per resample beyond the solver state (A operand, dense
// dual weights).
static int sd_batch(const plsx_ctx* ctx, int want, int unit, double extra)
{
    const double per = 8.0 * (double)sd_scratch_doubles(ctx->S, ctx->T, ctx->ncomp, simpls_global(ctx)) + extra;
    const double budget = 0.5 * ctx->scratch_gb * 1073741824.0;
    if ((double)want * per <= budget) return want;
    const long long fit = (long long)(budget / per);
    return (int)std::max<long long>(unit, fit / unit * unit);
}

// K = Xc Xc^T (S x S) of the bound data.  On-chip route: one symmetric product (upper blocks, mirrored from partial
// tiles: 2 S^2 doubles of partials).  Beyond it those partials would be twice K (37 GB at S = 48 000): every block of
// the full product stores its own tile instead -- twice the flop of the symmetric form (2 S^2 B: 2.3 Tflop at
// S = 24 000, B = 2000), once per binding, and no partial buffer.
int simpls_form_K(plsx_ctx* ctx, hipStream_t st)
{
    const int S = ctx->S;
    if (int e = ensure(ctx, ctx->Kmat, (size_t)S * S * 8)) return e;
    double* K = ptr<double>(ctx->Kmat);
    if (simpls_onchip_fits(S, ctx->T, ctx->ncomp))
        return run_nt(ctx, ptr<double>(ctx->Xc), 0, ctx->Bpad, S, ptr<double>(ctx->Xc), 0, ctx->Bpad, S,
                      nullptr, 0, 0, 0, ctx->B, 1, K, 0, S, nullptr, 0, 0, st, true);
    return nt_strips(ctx, ptr<double>(ctx->Xc), ctx->Bpad, S, ptr<double>(ctx->Xc), ctx->Bpad, S, ctx->B, K, S, st);
}

// A K of their own for groups of consecutive fits of a batch (the fold-wise confound regression: the fits of one split
// share K_s): K of group g at base + g S^2, `fits` fits per group.  base = nullptr: the bound K for every fit.
struct KGroups {
    const double* base = nullptr;
    int fits = 0;
};

// A [rows][S] against the bound K (S x S, symmetric) into Z [rows][S], on the route of the component step.  With kg:
// `per_fit` rows per fit, the rows of group g against its own K -- still one (batched) launch.  On-chip route only.
static int sd_times_K(plsx_ctx* ctx, const double* A, int rows, double* Z, hipStream_t st, const KGroups& kg = KGroups(),
                      int per_fit = 1)
{
    const int S = ctx->S;
    if (kg.base) {
        const int grows = kg.fits * per_fit;
        // (one chunk: every entry is one block's full contraction, so a fit's bits do not depend on how the splits are
        // grouped or the permutations chunked)
        return run_nt(ctx, A, (long long)grows * S, S, grows, kg.base, (long long)S * S, S, S, nullptr, 0, 0, 0, S,
                      rows / grows, Z, (long long)grows * S, S, nullptr, 0, 0, st, false, false, true);
    }
    const double* K = ptr<double>(ctx->Kmat);
    if (simpls_global(ctx)) return nt_strips(ctx, A, S, rows, K, S, S, S, Z, S, st);
    return run_nt(ctx, A, 0, S, rows, K, 0, S, S, nullptr, 0, 0, 0, S, 1, Z, 0, S, nullptr, 0, 0, st);
}

// What a caller asks of one solver batch (run_simpls_dual): a call site sets the fields it uses.
struct SdRequest {
    const int* xsrc = nullptr;          // [nres][S] X source of every position, or nullptr: identity
    const int* ysrc = nullptr;          // [nres][S] Y source, or nullptr
    int nres = 0;                       // resamples of the batch
    bool scatter = false;               // the dual weights leave the solver (k_sd_final runs); without it pctvar is all that does
    double* pctvar = nullptr;           // [nres][k]
    double* yload = nullptr;            // [nres][T][k]
    double* cvec = nullptr;             // [nres][T][k]
    const double* ystack = nullptr;     // [nres][S][T] a Y of its own per resample, or nullptr: the bound Y
    bool align_signs = false;           // (with scatter) signs aligned in dual space against ctx->Qs
    double* Vd = nullptr;               // (with scatter) the dual weights go out dense, [nres][k][S] (k_sd_final writes every
                                        // entry), not into the A operand
    const uint8_t* pmask = nullptr;     // [nres][S] positions a resample keeps (cross-validation: its training rows)
    SdArgs* args_out = nullptr;         // the carved-out state of the batch, for a kernel that runs after the chain (valid
                                        // until the next call)
    bool weights_only = false;          // (without scatter) k_sd_step keeps the dual weights WD in the batch's state
                                        // (a.weights), nothing leaves the solver but pctvar -- k_sd_final does not run (the
                                        // permutation test of the coefficients reads the state)
    KGroups kgroups;                    // a K of their own per group of fits (nres a multiple of kgroups.fits), or none
};

int run_simpls_dual(plsx_ctx* ctx, const SdRequest& q, hipStream_t st)
{
    const int nres = q.nres;
    const bool scatter = q.scatter;
    const int S = ctx->S, T = ctx->T, k = ctx->ncomp;
    const int groups = ceil_div(nres, ctx->npg);
    if (int e = ensure_scratch(ctx, std::min(groups, ctx->Gcap))) return e;
    SdArgs a;
    memset(&a, 0, sizeof(a));
    a.jacobi_eig = ctx->opt[OPT_SIMPLS_JACOBI] ? 1 : 0;
    a.weights = (scatter || q.weights_only) ? 1 : 0;
    a.S = S; a.T = T; a.k = k; a.nres = nres;
    a.Yc = q.ystack ? q.ystack : ptr<double>(ctx->Y);
    a.y_stride = q.ystack ? (long long)S * T : 0;
    a.okx = ctx->has_okx ? ptr<uint8_t>(ctx->okx) : nullptr;
    a.oky = ctx->has_oky ? ptr<uint8_t>(ctx->oky) : nullptr;
    a.xsrc = q.xsrc; a.ysrc = q.ysrc;
    a.pmask = q.pmask;
    // per-resample state, carved out of one scratch buffer (doubles)
    const bool gl = simpls_global(ctx);
    const size_t n = (size_t)nres;
    const size_t gemm_rows = n * (T + 1);
    if (int e = ensure(ctx, ctx->swork, (n * sd_scratch_doubles(S, T, k, gl) + 64 + (gl ? 2 : 0)) * 8)) return e;
    double* w = ptr<double>(ctx->swork);
    if (gl) {
        a.sfirst = reinterpret_cast<int*>(w);    w += n * S / 2 + 1;
        a.scnt = reinterpret_cast<int*>(w);      w += n * S / 2 + 1;
    }
    a.xs = reinterpret_cast<int*>(w);            w += n * S / 2 + 1;
    a.ys = reinterpret_cast<int*>(w);            w += n * S / 2 + 1;
    a.Y0 = w; w += n * S * T;
    a.Z0 = w; w += n * S * T;
    a.BT = w; w += n * k * S;
    a.KB = w; w += n * k * S;
    a.XW = w; w += n * k * S;
    a.WD = w; w += n * k * S;
    a.va = w; w += n * S;
    a.kcpos = w; w += n * S;
    a.H = w; w += n * T * T;
    a.H0 = w; w += n * T * T;
    a.G = w; w += n * k * T;
    a.gY0 = w; w += n * k * T;
    a.ymean = w; w += n * T;
    a.scal = w; w += n * 4;
    a.Wt = w; w += gemm_rows * S;
    a.Zt = w;
    a.pctvar = q.pctvar; a.yload = q.yload; a.cvec = q.cvec;
    if (scatter && q.Vd) {
        a.Vd = q.Vd;                                   // (k_sd_final writes every entry)
    } else if (scatter) {
        // the solver batch may span several cross-product batches: its own span of A operands
        if (int e = ensure(ctx, ctx->Afrag, (size_t)groups * ctx->group_stride * 8 + 4096)) return e;
        HIPCHK(hipMemsetAsync(ctx->Afrag.p, 0, (size_t)groups * ctx->group_stride * 8, st));
        a.Afrag = ptr<double>(ctx->Afrag); a.group_stride = ctx->group_stride;
        a.lay.n = ctx->npg; a.lay.Tp = ctx->Tp; a.lay.J = 1; a.lay.T = T; a.lay.MT = ctx->MT;
        a.lay.w0 = ctx->w0; a.lay.sq0 = ctx->sq0; a.lay.Tpp = ctx->Tpp;
    }
    // one wavefront per resample; as many waves per block as keep >= 2 blocks of k_sd_step on a CU
    const size_t step_wave = gl ? simpls_global_lds_bytes(T, k) : sd_step_lds(S, T, k) * 8;
    const int wpb = (int)std::max<size_t>(1, std::min<size_t>(4, (72 * 1024) / step_wave));
    const dim3 grid(ceil_div(nres, wpb)), block(wpb * 64);
    // more waves than two per SIMD of the chip: the three-waves-per-SIMD variants (SD_RC).  (The global route keeps the
    // 16-position tiles: its batches are bounded by the scratch, and its kernels exist in that form only.)
    const bool big = nres > 2048 && !gl;
    if (gl) {
        KTimer tm(ctx, KC_SIMPLS, st);
        hipLaunchKernelGGL(k_sd_init<true>, grid, block, 0, st, a);
        LAUNCHCHK();
    } else {
        const size_t lds = (size_t)wpb * S * 8;
        HIPCHK(set_lds(k_sd_init<false>, lds));
        KTimer tm(ctx, KC_SIMPLS, st);
        hipLaunchKernelGGL(k_sd_init<false>, grid, block, lds, st, a);
        LAUNCHCHK();
    }
    // GEMM 0: (T + 1) subject-space vectors per resample against K (symmetric)
    if (int e = sd_times_K(ctx, a.Wt, (int)gemm_rows, a.Zt, st, q.kgroups, T + 1)) return e;
    {
        KTimer tm(ctx, KC_SIMPLS, st);
        void (*post0_kernel)(SdArgs) =
            T <= 32 ? (big ? k_sd_post0<8, 0> : k_sd_post0<16, 0>)
                    : (T <= 64 ? (big ? k_sd_post0<8, 1> : k_sd_post0<16, 1>) : k_sd_post0<16, 2>);
        hipLaunchKernelGGL(post0_kernel, grid, block, 0, st, a);
        LAUNCHCHK();
    }
    const size_t lds_step = (size_t)wpb * step_wave;
    // (Jacobi eigen-solve -- T > S, T > 64 or the option: rare, not time critical -- per class of T like everything else;
    // the 16-rows-per-lane instantiation of 32 < T <= 64 is back, see k_sd_step)
    const bool jac = a.jacobi_eig || T > 64 || T > S;
    void (*step_kernel)(SdArgs) =
        gl ? (jac ? (T <= 32 ? k_sd_step<0, true, 16, true> : (T <= 64 ? k_sd_step<1, true, 16, true>
                                                                       : k_sd_step<2, true, 16, true>))
                  : (T <= 32 ? k_sd_step<0, false, 16, true> : k_sd_step<1, false, 16, true>)) :
        jac ? (T <= 32 ? (big ? k_sd_step<0, true, 8> : k_sd_step<0, true, 16>)
                       : (T <= 64 ? k_sd_step<1, true, 16> : k_sd_step<2, true, 16>))
            : (T <= 32 ? (big ? k_sd_step<0, false, 8> : k_sd_step<0, false, 16>)
                       : (big ? k_sd_step<1, false, 8> : k_sd_step<1, false, 16>));
    HIPCHK(set_lds(step_kernel, lds_step));
    for (int c = 0; c < k; ++c) {
        a.c = c;
        {
            KTimer tm(ctx, KC_SIMPLS, st);
            hipLaunchKernelGGL(step_kernel, grid, block, lds_step, st, a);
            LAUNCHCHK();
        }
        // GEMM c: K beta for every resample of the batch (the last component needs none)
        if (c + 1 < k)
            if (int e = sd_times_K(ctx, a.Wt, nres, a.Zt, st, q.kgroups)) return e;
    }
    if (scatter) {          // (permutations: pctvar is all that leaves the solver -- no y-loadings, no weights)
        a.Qs = q.align_signs ? ptr<double>(ctx->Qs) : nullptr;
        KTimer tm(ctx, KC_SIMPLS, st);
        // (per wave: the signs and, on the on-chip route, one subject-space scatter buffer)
        const size_t lds_f = (size_t)wpb * (gl ? k : k + S) * 8;
        void (*final_kernel)(SdArgs) =
            gl ? (T <= 32 ? k_sd_final<16, 0, true> : (T <= 64 ? k_sd_final<16, 1, true> : k_sd_final<16, 2, true>)) :
            T <= 32 ? (big ? k_sd_final<8, 0> : k_sd_final<16, 0>)
                    : (T <= 64 ? (big ? k_sd_final<8, 1> : k_sd_final<16, 1>) : k_sd_final<16, 2>);
        HIPCHK(set_lds(final_kernel, lds_f));
        hipLaunchKernelGGL(final_kernel, grid, block, lds_f, st, a);
        LAUNCHCHK();
    }
    if (q.args_out) *q.args_out = a;
#ifdef PLSX_SD_PROBE
    {
        unsigned long long h[16][32];
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_sd_probe), sizeof(h)));
        for (int c : {0, 7, 14})
            if (c < k) {
                fprintf(stderr, "[sd probe] c=%d nres=%d cycles:", c, nres);
                for (int m = 1; m <= 12; ++m) fprintf(stderr, " %d:%lld", m, h[c][m] > h[c][m - 1] ? (long long)(h[c][m] - h[c][m - 1]) : -1LL);
                fprintf(stderr, "\n");
            }
    }
#endif
    return 0;
}

// single-pass form of the SIMPLS bootstrap: signs aligned in dual space (k_sd_final), the feature
// pass accumulates the aligned weights and their squares (k_xprod EPI = 2)
bool simpls_single_pass(const plsx_ctx* ctx)
{
    return (size_t)2 * ctx->ncomp * PLSX_ACC_PITCH * 8 <= 72 * 1024 && ctx->Qs.p && !ctx->opt[OPT_TWO_PASS_BOOT];
}


// Free device bytes, with what an earlier pass left allocated in `own` -- the buffer the caller is about to size --
// counting as free.
static int free_bytes(plsx_ctx* ctx, const Buf& own, double* have)
{
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    *have = (double)free_b + (double)own.bytes;
    return 0;
}

// Feature chunks of a closing pass over a kept stack of n resamples (plsx_simpls_coef_ci, plsx_simpls_vip_ci): whole
// 128-feature blocks whose series, `per_feat` bytes a feature, stay next to the stack (`stack` bytes) inside the scratch
// budget and in free device memory, 2 GB at most -- the series are written once and read once, a larger chunk buys
// nothing.  Sets *fc (the caller sizes ctx->cichunk for it, fc . per_feat bytes, after its own checks); refuses when not
// even the smallest chunk fits.  `dim`, `dimv`: the name and value of the stack's middle dimension ("T" or "c") in the
// refusal.
static int ci_chunk(plsx_ctx* ctx, const char* who, long long n, double stack, double per_feat, const char* dim,
                    int dimv, long long* fc)
{
    const int B = ctx->B, unit = std::min(B, 128);
    double have;
    if (int e = free_bytes(ctx, ctx->cichunk, &have)) return e;
    const double room = std::min(ctx->scratch_gb * 1073741824.0 - stack, have);
    if (room < unit * per_feat) {
        char msg[400];
        snprintf(msg, sizeof msg, "%s: the stack of n = %lld bootstraps (8 n %s S = %.3f GB for %s = %d, "
                 "S = %d) and the series of the smallest chunk of %d features (%.3f GB) need %.3f GB; the scratch budget "
                 "is %.3f GB and %.3f GB of device memory are free", who, n, dim, stack / 1073741824.0, dim, dimv,
                 ctx->S, unit, unit * per_feat / 1073741824.0, (stack + unit * per_feat) / 1073741824.0, ctx->scratch_gb,
                 have / 1073741824.0);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    *fc = (long long)(std::min(room, 2147483648.0) / per_feat);
    *fc = std::max<long long>(unit, *fc / 128 * 128);
    if (*fc >= B) *fc = B;
    return 0;
}

// The coefficient series' share of a solver batch (plsx_simpls_coef_begin): k_sd_coef writes A_b of `ms` bootstraps
// dense, in chunks of at most 1 GB, and each chunk goes through quad_accumulate on the series' own accumulator set.
// `a`: the state run_simpls_dual just left (args_out).  The solver batches themselves are what they are without a
// series, so everything else a call computes keeps its bits.
static QuadSet coef_set(plsx_ctx* ctx, const double* Ad = nullptr)
{
    return QuadSet{&ctx->Cc, &ctx->Asumc, Ad ? Ad : ptr<double>(ctx->Adc), ctx->T};
}

// Waves per block and dynamic LDS of a kernel that gives each wave `per_wave` bytes (k_sd_coef, k_sd_vip): up to four
// waves inside 64 KB.
static int sd_waves(size_t per_wave, size_t* lds)
{
    const int wpb = (int)std::max<size_t>(1, std::min<size_t>(4, (64 * 1024) / std::max<size_t>(per_wave, 1)));
    *lds = (size_t)wpb * per_wave;
    return wpb;
}

// k_sd_coef on the state `a` run_simpls_dual just left for a batch of `ms` resamples: A_r of resamples r0 .. r0 + mc - 1
// with cc components, dense into Ad [mc][T][S]; Q in ctx->Qc.  The kernel variant goes by the batch, not by mc.
static int sd_coef_launch(plsx_ctx* ctx, SdArgs a, int cc, int ms, int r0, int mc, double* Ad, hipStream_t st)
{
    const bool gl = simpls_global(ctx);
    // (a batch's first chunk is its largest and ensure() never shrinks: Qc is sized once per batch)
    if (int e = ensure(ctx, ctx->Qc, (size_t)mc * cc * ctx->T * 8)) return e;
    size_t lds;
    const int wpb = sd_waves(((size_t)cc + (gl ? 0 : (size_t)ctx->S)) * 8, &lds);
    a.cfq = ptr<double>(ctx->Qc); a.cf_c = cc;
    a.cfA = Ad; a.cf_r0 = r0; a.cf_n = mc;
    KTimer tm(ctx, KC_COEF, st);
    // (more waves than two per SIMD of the chip: the short position tiles, as in the solver)
    void (*coef_kernel)(SdArgs) = gl ? k_sd_coef<16, true> : (ms > 2048 ? k_sd_coef<8, false> : k_sd_coef<16, false>);
    HIPCHK(set_lds(coef_kernel, lds));
    hipLaunchKernelGGL(coef_kernel, dim3(ceil_div(mc, wpb)), dim3(wpb * 64), lds, st, a);
    LAUNCHCHK();
    return 0;
}

static int coef_accumulate(plsx_ctx* ctx, SdArgs a, int ms, hipStream_t st)
{
    const int S = ctx->S, T = ctx->T, cc = ctx->coef_c;
    const int chunk = (int)std::max<long long>(1, std::min<long long>(ms, (1LL << 30) / ((long long)T * S * 8)));
    // (a series that keeps its A_b -- plsx_simpls_coef_keep -- has every chunk written where it stays, in the caller's
    // buffer, and accumulated from there: the same values through the same kernels, so the sums keep their bits)
    if (ctx->keepA && ctx->keep_n + ms > ctx->keep_cap)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_boot_batch: the kept coefficient stack is full");
    if (!ctx->keepA)
        if (int e = ensure(ctx, ctx->Adc, (size_t)chunk * T * S * 8)) return e;
    for (int r0 = 0; r0 < ms; r0 += chunk) {
        const int mc = std::min(chunk, ms - r0);
        double* Ad = ctx->keepA ? ctx->keepA + (size_t)(ctx->keep_n + r0) * T * S : ptr<double>(ctx->Adc);
        if (int e = sd_coef_launch(ctx, a, cc, ms, r0, mc, Ad, st)) return e;
        const QuadSet qs = coef_set(ctx, Ad);
        if (int e = quad_accumulate(ctx, mc, st, &qs)) return e;
    }
    ctx->coef_n += ms;
    if (ctx->keepA) ctx->keep_n += ms;
    return 0;
}


// k_sd_vip on the state `a` run_simpls_dual just left (args_out) for a batch of `ms` resamples: the cc scaled dual-weight
// rows of each, dense into G [ms][cc][S].  Nothing else reads or writes what it touches.
static int sd_vip_launch(plsx_ctx* ctx, SdArgs a, int cc, int ms, double* G, hipStream_t st)
{
    const bool gl = simpls_global(ctx);
    size_t lds;
    const int wpb = sd_waves(gl ? 0 : (size_t)ctx->S * 8, &lds);
    a.vpG = G; a.vp_c = cc;
    KTimer tm(ctx, KC_COEF, st);
    void (*vip_kernel)(SdArgs) = gl ? k_sd_vip<true> : k_sd_vip<false>;
    HIPCHK(set_lds(vip_kernel, lds));
    hipLaunchKernelGGL(vip_kernel, dim3(ceil_div(ms, wpb)), dim3(wpb * 64), lds, st, a);
    LAUNCHCHK();
    return 0;
}

// The VIP stack's share of a solver batch (plsx_simpls_vip_keep): the rows of the batch's `ms` bootstraps go where they
// stay, in the caller's buffer, so everything else a call computes keeps its bits.
static int vip_append(plsx_ctx* ctx, SdArgs a, int ms, hipStream_t st)
{
    const int S = ctx->S, cc = ctx->vip_c;
    if (ctx->vip_n + ms > ctx->vip_cap)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_boot_batch: the kept VIP stack is full");
    if (int e = sd_vip_launch(ctx, a, cc, ms, ctx->vipG + (size_t)ctx->vip_n * cc * S, st)) return e;
    ctx->vip_n += ms;
    return 0;
}


// s_f of every bound feature into ctx->colsd (k_col_sd): the standard deviation over the usable rows of X
static int col_sd(plsx_ctx* ctx, hipStream_t st)
{
    if (int e = ensure(ctx, ctx->colsd, (size_t)ctx->Bpad * 8)) return e;
    const double nx = ctx->has_okx ? (double)ctx->n_okx : (double)ctx->S;
    KTimer tm(ctx, KC_COEFPROD, st);
    hipLaunchKernelGGL(k_col_sd, dim3(ceil_div(ctx->Bpad, 256)), dim3(256), 0, st, ptr<double>(ctx->Xc), ctx->Bpad, ctx->S,
                       ctx->B, nx, ptr<double>(ctx->colsd));
    LAUNCHCHK();
    return 0;
}

// The permutation statistics of a stack A [n][T][S] against `obs` (plsx_simpls_coef_perm_test and the open series of
// plsx_simpls_coef_perm_begin): count (B, T) += exceedances, dmax (n, T) = maxima over the features.  The stack goes in
// pieces of at most 16384 permutations, the features of a piece in chunks of whole 128-feature blocks whose partial
// maxima, 8 T n bytes per block, fit `room` bytes and 2 GB.  Counts are integers and a maximum has no order: the
// result depends on neither.
static int coef_perm_run(plsx_ctx* ctx, const double* A, long long n, const double* obs, const double* sd, int* count,
                         double* dmax, double room, const char* who, hipStream_t st)
{
    const int S = ctx->S, T = ctx->T, B = ctx->B;
    room = std::min(room, 2147483648.0);
    long long piece = std::min<long long>(n, 16384);
    if (room < 8.0 * T * (double)piece) piece = (long long)(room / (8.0 * T)) / 64 * 64;
    if (piece < 1) {
        char msg[320];
        snprintf(msg, sizeof msg, "%s: the partial maxima of one 128-feature block and 64 permutations (8 T n = %.0f "
                 "bytes for T = %d) do not fit next to the stack: the scratch budget is %.6f GB", who, 8.0 * T * 64, T,
                 ctx->scratch_gb);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    const int nfb_all = ceil_div(B, 128);
    const int nfb = (int)std::max<long long>(1, std::min<long long>(nfb_all, (long long)(room / (8.0 * T * (double)piece))));
    if (int e = ensure(ctx, ctx->cppart, (size_t)nfb * T * (size_t)piece * 8)) return e;
    CoefPermArgs a;
    a.Xc = ptr<double>(ctx->Xc); a.ldx = ctx->Bpad;
    a.S = S; a.T = T; a.B = B;
    a.obs = obs; a.sd = sd; a.count = count; a.pmax = ptr<double>(ctx->cppart);
    for (long long p0 = 0; p0 < n; p0 += piece) {
        a.n = (int)std::min<long long>(piece, n - p0);
        a.A = A + (size_t)p0 * T * S;
        for (int fb0 = 0; fb0 < nfb_all; fb0 += nfb) {
            const int nb = std::min(nfb, nfb_all - fb0);
            a.f0 = fb0 * 128; a.fc = std::min(nb * 128, B - a.f0);
            KTimer tm(ctx, KC_COEFPROD, st);
            hipLaunchKernelGGL(k_coef_perm_prod, dim3(nb, T), dim3(256), 0, st, a);
            LAUNCHCHK();
            hipLaunchKernelGGL(k_coef_perm_max, dim3((unsigned)(((long long)T * a.n + 255) / 256)), dim3(256), 0, st,
                               a.pmax, nb, T, a.n, fb0 == 0 ? 1 : 0, dmax + (size_t)p0 * T);
            LAUNCHCHK();
        }
    }
    return 0;
}

// The open permutation series' share of a solver batch (plsx_simpls_coef_perm_begin): k_sd_coef writes A_p of the
// batch's `ms` permutations dense into scratch, the test above runs on that piece and appends its maxima.  `a`: the
// state run_simpls_dual just left (args_out; weights on).
static int coef_perm_append(plsx_ctx* ctx, SdArgs a, int ms, hipStream_t st)
{
    const int S = ctx->S, T = ctx->T;
    if (int e = ensure(ctx, ctx->cpA, (size_t)ms * T * S * 8)) return e;
    if (int e = sd_coef_launch(ctx, a, ctx->cperm_c, ms, 0, ms, ptr<double>(ctx->cpA), st)) return e;
    double have;
    if (int e = free_bytes(ctx, ctx->cppart, &have)) return e;
    const double room = std::min(0.25 * ctx->scratch_gb * 1073741824.0, have);
    if (int e = coef_perm_run(ctx, ptr<double>(ctx->cpA), ms, ctx->cperm_obs, ctx->cperm_std ? ptr<double>(ctx->colsd) : nullptr,
                              ctx->cperm_count, ctx->cperm_max + (size_t)ctx->cperm_n * T, room,
                              "plsx_simpls_perm_batch", st))
        return e;
    ctx->cperm_n += ms;
    return 0;
}

// The permutation statistics of a stack G [n][c][S] against the observed VIP scores `obs` (plsx_simpls_vip_perm_test and
// the open series of plsx_simpls_vip_perm_begin): count (B,) += exceedances, dmax (n,) = maxima over the features.
// coef_perm_run's rule with one row per permutation: the stack goes in pieces of at most 16384 permutations, the
// features of a piece in chunks of whole 128-feature blocks whose partial maxima, 8 n bytes per block, fit `room` bytes
// and 2 GB.  The permutation tiles of a piece go in runs of tpb tiles, one block per (feature block, run), tpb the
// largest for which a chunk still launches VIP_PERM_BLOCKS blocks -- sixteen rounds of the chip's two blocks per CU, so
// that the last, partial round costs a few percent -- and every run leaves its counts in a row of vpcnt.  Counts are
// integers and a maximum has no order: the result depends on none of this.
static const int VIP_PERM_BLOCKS = 8192;
static int vip_perm_run(plsx_ctx* ctx, const double* G, long long n, int c, const double* obs, int* count, double* dmax,
                        double room, const char* who, hipStream_t st)
{
    const int S = ctx->S, B = ctx->B;
    room = std::min(room, 2147483648.0);
    long long piece = std::min<long long>(n, 16384);
    if (room < 8.0 * (double)piece) piece = (long long)(room / 8.0) / 64 * 64;
    if (piece < 1) {
        char msg[320];
        snprintf(msg, sizeof msg, "%s: the partial maxima of one 128-feature block and 64 permutations (512 bytes) do "
                 "not fit next to the stack of n = %lld permutations (8 n c S = %.6f GB for c = %d, S = %d): the scratch "
                 "budget is %.6f GB", who, n, 8.0 * (double)n * c * S / 1073741824.0, c, S, ctx->scratch_gb);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    const int nfb_all = ceil_div(B, 128);
    const int nfb = (int)std::max<long long>(1, std::min<long long>(nfb_all, (long long)(room / (8.0 * (double)piece))));
    if (int e = ensure(ctx, ctx->cppart, (size_t)nfb * (size_t)piece * 8)) return e;
    const int tiles = (int)((piece + 63) / 64);
    const int tpb = std::max(1, tiles / std::max(1, ceil_div(VIP_PERM_BLOCKS, std::min(nfb, nfb_all))));
    if (int e = ensure(ctx, ctx->vpcnt, (size_t)ceil_div(tiles, tpb) * ctx->Bpad * sizeof(int))) return e;
    VipPermArgs a;
    a.Xc = ptr<double>(ctx->Xc); a.ldx = ctx->Bpad;
    a.S = S; a.c = c; a.B = B;
    a.obs = obs; a.pmax = ptr<double>(ctx->cppart);
    a.tpb = tpb; a.pcount = ptr<int>(ctx->vpcnt);
    for (long long p0 = 0; p0 < n; p0 += piece) {
        a.n = (int)std::min<long long>(piece, n - p0);
        a.G = G + (size_t)p0 * c * S;
        const int runs = ceil_div(ceil_div(a.n, 64), tpb);
        for (int fb0 = 0; fb0 < nfb_all; fb0 += nfb) {
            const int nb = std::min(nfb, nfb_all - fb0);
            a.f0 = fb0 * 128; a.fc = std::min(nb * 128, B - a.f0);
            KTimer tm(ctx, KC_COEFPROD, st);
            hipLaunchKernelGGL(k_vip_perm_prod, dim3(nb, runs), dim3(256), 0, st, a);
            LAUNCHCHK();
            hipLaunchKernelGGL(k_vip_perm_count, dim3(ceil_div(a.fc, 256)), dim3(256), 0, st, a.pcount, a.ldx, runs, a.f0,
                               a.f0 + a.fc, count);
            LAUNCHCHK();
            hipLaunchKernelGGL(k_coef_perm_max, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st,
                               a.pmax, nb, 1, a.n, fb0 == 0 ? 1 : 0, dmax + (size_t)p0);
            LAUNCHCHK();
        }
    }
    return 0;
}

// The open VIP series' share of a solver batch (plsx_simpls_vip_perm_begin): k_sd_vip writes the scaled dual weights of
// the batch's `ms` permutations dense into scratch, the test above runs on that piece and appends its maxima.  `a`: the
// state run_simpls_dual just left (args_out; weights on).
static int vip_perm_append(plsx_ctx* ctx, SdArgs a, int ms, hipStream_t st)
{
    const int S = ctx->S, cc = ctx->vperm_c;
    if (int e = ensure(ctx, ctx->vpG, (size_t)ms * cc * S * 8)) return e;
    if (int e = sd_vip_launch(ctx, a, cc, ms, ptr<double>(ctx->vpG), st)) return e;
    double have;
    if (int e = free_bytes(ctx, ctx->cppart, &have)) return e;
    const double room = std::min(0.25 * ctx->scratch_gb * 1073741824.0, have);
    if (int e = vip_perm_run(ctx, ptr<double>(ctx->vpG), ms, cc, ctx->vperm_obs, ctx->vperm_count,
                             ctx->vperm_max + (size_t)ctx->vperm_n, room, "plsx_simpls_perm_batch", st))
        return e;
    ctx->vperm_n += ms;
    return 0;
}


}  // namespace plsxi

// The two series of counts that ride along the cross-validation entries (CountSeries): confusion counts, blocks
// [k][G][G] int32 (plsx_simpls_cv_class_begin), and AUC counts, blocks [k][G][2] int64 (plsx_simpls_cv_auc_begin).  The
// bodies of their _begin / _end entries:
static int count_begin(plsx_ctx* ctx, bool auc, void* d_buf, long long capacity)
{
    NEED_DATA();
    CountSeries& s = auc ? ctx->auc_series : ctx->cls_series;
    const std::string who = s.entry;
    if (ctx->method != PLSX_REGRESSION) return fail(ctx, PLSX_ERR_STATE, who + ": data not bound for regression");
    if (!ctx->has_cls) return fail(ctx, PLSX_ERR_STATE, who + ": plsx_simpls_set_classes has not been called");
    count_close(s);
    if (!d_buf || capacity < 1) return fail(ctx, PLSX_ERR_ARG, who + ": null buffer or capacity < 1");
    s.base = static_cast<char*>(d_buf); s.cap = capacity; s.n = 0;
    s.blk_bytes = (size_t)ctx->ncomp * ctx->T * (auc ? 2 * sizeof(long long) : ctx->T * sizeof(int));
    s.active = 1;
    return PLSX_OK;
}

static int count_end(plsx_ctx* ctx, bool auc)
{
    if (!ctx) return PLSX_ERR_ARG;
    count_close(auc ? ctx->auc_series : ctx->cls_series);
    return PLSX_OK;
}

// Room for m more blocks in each series that is open, or PLSX_ERR_ARG before anything is computed or zeroed; the blocks
// are zeroed here, in stream order before the kernels that count into them.
static int count_reserve(plsx_ctx* ctx, const char* who, int m, hipStream_t st)
{
    CountSeries* const both[2] = {&ctx->cls_series, &ctx->auc_series};
    for (const CountSeries* s : both)
        if (s->active && s->n + m > s->cap) {
            char msg[240];
            snprintf(msg, sizeof msg, "%s: the open series of %s holds %lld of %lld blocks, %d more do not fit (%s)", who,
                     s->what, s->n, s->cap, m, s->entry);
            return fail(ctx, PLSX_ERR_ARG, msg);
        }
    for (const CountSeries* s : both)
        if (s->active) HIPCHK(hipMemsetAsync(s->base + (size_t)s->n * s->blk_bytes, 0, (size_t)m * s->blk_bytes, st));
    return 0;
}

// The counting kernel (k_sd_cv_class, or auc: k_sd_cv_auc behind it) on the ms fits k_sd_cv_score has just scored: fit r
// counts into block (f0 + r) / n - f0 / n behind `out`, the block of the batch's first fit.
template <bool PERM>
static int count_launch(plsx_ctx* ctx, bool auc, void* out, SdArgs a, int ms, long long f0, int n, hipStream_t st)
{
    a.cls = ptr<int>(ctx->cls);
    a.cfreq = ptr<double>(ctx->clsfreq);
    if (auc) a.auc = static_cast<long long*>(out); else a.conf = static_cast<int*>(out);
    a.cls_f0 = f0; a.cls_n = n;
    KTimer tm(ctx, auc ? KC_CVAUC : KC_CVCLASS, st);
    void (*kernel)(SdArgs) =
        auc ? (a.T <= 4 ? k_sd_cv_auc<4, PERM> : (a.T <= 16 ? k_sd_cv_auc<16, PERM> : k_sd_cv_auc<32, PERM>))
            : (a.T <= 4 ? k_sd_cv_class<4, PERM> : (a.T <= 16 ? k_sd_cv_class<16, PERM> : k_sd_cv_class<32, PERM>));
    hipLaunchKernelGGL(kernel, dim3(ceil_div(ms, 4)), dim3(256), 0, st, a);
    LAUNCHCHK();
    return 0;
}

// The series of out-of-fold predictions (PredSeries).  Room for m more slots, or PLSX_ERR_ARG before anything is computed
// or written; `nested`: the entry selects the component count per fit, which a series opened with c = 0 waits for.
static int pred_reserve(plsx_ctx* ctx, const char* who, int m, bool nested)
{
    const PredSeries& s = ctx->pred_series;
    if (!s.active) return 0;
    char msg[260];
    if (s.c == 0 && !nested) {
        snprintf(msg, sizeof msg, "%s: the open series of predictions takes the component count of the nested selection "
                 "(c = 0); this entry selects none (plsx_simpls_cv_pred_begin)", who);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    if (s.n + m > s.cap) {
        snprintf(msg, sizeof msg, "%s: the open series of predictions holds %lld of %lld fits, %d more do not fit "
                 "(plsx_simpls_cv_pred_begin)", who, s.n, s.cap, m);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    return 0;
}

// Which fits of a batch the open series keeps: slot `slot0` of this call onwards takes fits 0, unit, 2 unit, ... of the
// batch, `ncomp` their component counts on the device (the nested selection's) or nullptr: the series' own c.
struct PredAppend { long long slot0; int unit; const int* ncomp; };

// k_sd_cv_pred on the fits k_sd_cv_score has just scored (and the kernels of the counts have classified), in the
// scoring kernels' timing class
static int pred_launch(plsx_ctx* ctx, SdArgs a, int ms, const PredAppend& pa, hipStream_t st)
{
    const PredSeries& s = ctx->pred_series;
    const size_t slot = (size_t)(s.n + pa.slot0), TS = (size_t)a.T * a.S;
    SdPredArgs q;
    q.pred = s.pred + slot * TS;
    q.ytrue = s.ytrue ? s.ytrue + slot * TS : nullptr;
    q.ncomp_out = s.ncomp ? s.ncomp + slot : nullptr;
    q.ncomp_in = s.c == 0 ? pa.ncomp : nullptr;
    q.c = s.c;
    q.unit = pa.unit; q.slots = ms / pa.unit;
    const bool da = ctx->has_cls != 0;
    if (da) { a.cls = ptr<int>(ctx->cls); a.cfreq = ptr<double>(ctx->clsfreq); }
    KTimer tm(ctx, KC_CVSCORE, st);
    void (*kernel)(SdArgs, SdPredArgs) =
        !da ? k_sd_cv_pred<0> : (a.T <= 4 ? k_sd_cv_pred<4> : (a.T <= 16 ? k_sd_cv_pred<16> : k_sd_cv_pred<32>));
    hipLaunchKernelGGL(kernel, dim3(ceil_div(q.slots, 4)), dim3(256), 0, st, a, q);
    LAUNCHCHK();
    return 0;
}

// Scratch of a cross-validation batch of nb fits: pctvar [nb][k] with the y-loadings [nb][T][k] behind it, the right
// singular vectors, the dense dual weights Vd and Z = Vd . K
static int cv_scratch(plsx_ctx* ctx, int nb)
{
    const size_t S = ctx->S, T = ctx->T, k = ctx->ncomp;
    if (int e = ensure(ctx, ctx->spct, nb * (T + 1) * k * 8)) return e;
    if (int e = ensure(ctx, ctx->sc, nb * T * k * 8)) return e;
    if (int e = ensure(ctx, ctx->Vdq, nb * k * S * 8)) return e;
    return ensure(ctx, ctx->Zcv, nb * k * S * 8);
}

// Where k_sd_cv_score leaves the scores of a batch's fits: [ms][k][T], [ms][k][T], [ms][k + 1][T] and, PERM only, [ms]
struct CvScores { double* r; double* r2; double* sse; double* nte; };

// One solver batch of cross-validated fits, end to end (plsx_simpls_crossval_batch, PERM: plsx_simpls_crossval_perm_batch):
// the ms fits on their training positions (`pmask` [ms][S]; X keeps its rows, Y takes rows `ysrc` or its own), ONE
// product with K, the scores, `after_score` in the scores' timed bracket (the reduction of the permuted entry), and the
// counts of the series that are open, whose blocks are addressed as count_launch says.  nb: the fits cv_scratch was
// sized for.  ystack / kg: a Y ([ms][S][T]) and a K of the fits' own (the fold-wise confound regression), or the bound ones.
// pred: what an open series of predictions keeps of the batch (observed fits only), or nullptr: nothing.
// fitcnt: the nested selection on counts -- every fit counts into a block of its own in scratch (zeroed by the caller),
// and `after_score` runs BEHIND the counting kernels, in a scores' bracket of its own.
struct FitCounts { int* conf; long long* auc; };
template <bool PERM, class F>
static int cv_fit_score(plsx_ctx* ctx, int nb, int ms, const int* ysrc, const uint8_t* pmask, const CvScores& out,
                        long long blk0, long long f0, int n, hipStream_t st, F after_score,
                        const double* ystack = nullptr, const KGroups& kg = KGroups(), const PredAppend* pred = nullptr,
                        const FitCounts* fitcnt = nullptr)
{
    const int k = ctx->ncomp;
    SdArgs a;
    // identity X sources, the test positions excluded, weights wanted; the signs stay as the solver produced them
    // (t_j q_j^T does not depend on them)
    SdRequest q;
    q.ysrc = ysrc; q.nres = ms; q.scatter = true;
    q.pctvar = ptr<double>(ctx->spct); q.yload = q.pctvar + (size_t)nb * k; q.cvec = ptr<double>(ctx->sc);
    q.Vd = ptr<double>(ctx->Vdq); q.pmask = pmask; q.args_out = &a;
    q.ystack = ystack; q.kgroups = kg;
    if (int e = run_simpls_dual(ctx, q, st)) return e;
    // ONE product with K: the scores of all k nested models at every row, training and test
    a.cvZ = ptr<double>(ctx->Zcv);
    if (int e = sd_times_K(ctx, q.Vd, ms * k, a.cvZ, st, kg, k)) return e;
    a.cvr = out.r; a.cvr2 = out.r2; a.cvsse = out.sse; a.cvnte = out.nte;
    {
        KTimer tm(ctx, KC_CVSCORE, st);
        // (more waves than two per SIMD of the chip: the three-waves-per-SIMD variant, as in the solver)
        void (*score_kernel)(SdArgs) = (ms > 2048 && !simpls_global(ctx)) ? k_sd_cv_score<8, PERM> : k_sd_cv_score<16, PERM>;
        hipLaunchKernelGGL(score_kernel, dim3(ceil_div(ms, 4)), dim3(256), 0, st, a);
        LAUNCHCHK();
        if (!fitcnt)
            if (int e = after_score()) return e;
    }
    if (fitcnt) {
        if (int e = count_launch<PERM>(ctx, false, fitcnt->conf, a, ms, 0, 1, st)) return e;
        if (fitcnt->auc)
            if (int e = count_launch<PERM>(ctx, true, fitcnt->auc, a, ms, 0, 1, st)) return e;
        KTimer tm(ctx, KC_CVSCORE, st);
        if (int e = after_score()) return e;
    }
    for (const CountSeries* s : {&ctx->cls_series, &ctx->auc_series})
        if (s->active)
            if (int e = count_launch<PERM>(ctx, s == &ctx->auc_series, s->base + (size_t)(s->n + blk0) * s->blk_bytes, a, ms,
                                           f0, n, st))
                return e;
    if constexpr (!PERM)
        if (pred && ctx->pred_series.active)
            if (int e = pred_launch(ctx, a, ms, *pred, st)) return e;
    return 0;
}

extern "C" {

int plsx_simpls_decompose(plsx_ctx* ctx, double* d_xwT, double* d_pctvar, double* d_cvec, double* d_yload,
                          void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION) return fail(ctx, PLSX_ERR_STATE, "data not bound for regression");
    if (!d_xwT || !d_pctvar || !d_cvec || !d_yload) return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_decompose: null output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    SdRequest q;
    q.nres = 1; q.scatter = true;
    q.pctvar = d_pctvar; q.yload = d_yload; q.cvec = d_cvec;
    if (int e = run_simpls_dual(ctx, q, st)) return e;
    if (int e = run_xprod(ctx, nullptr, nullptr, 1, st, true)) return e;
    hipLaunchKernelGGL(k_gather_cols, dim3(ceil_div(ctx->Tp * ctx->B, 256), 1), dim3(256), 0, st,
                       ptr<double>(ctx->R), ctx->strideR, ctx->Bpad, 0, ctx->Tp, ctx->B, d_xwT);
    LAUNCHCHK();
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_set_original(plsx_ctx* ctx, const double* d_w0cT, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION) return fail(ctx, PLSX_ERR_STATE, "data not bound for regression");
    if (!d_w0cT) return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_set_original: null input");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemsetAsync(ctx->U0T.p, 0, (size_t)ctx->L * ctx->Bpad * 8, st));
    HIPCHK(hipMemcpy2DAsync(ctx->U0T.p, (size_t)ctx->Bpad * 8, d_w0cT, (size_t)ctx->B * 8, (size_t)ctx->B * 8,
                            ctx->ncomp, hipMemcpyDeviceToDevice, st));
    // Qs = Xc . W0c^T (S x k): what the sign alignment of a bootstrap needs in dual space
    if (int e = ensure(ctx, ctx->Qs, (size_t)ctx->S * ctx->ncomp * 8)) return e;
    if (int e = run_nt(ctx, ptr<double>(ctx->Xc), 0, ctx->Bpad, ctx->S, ptr<double>(ctx->U0T), 0, ctx->Bpad, ctx->ncomp,
                       nullptr, 0, 0, 0, ctx->B, 1, ptr<double>(ctx->Qs), 0, ctx->ncomp, nullptr, 0, 0, st))
        return e;
    ctx->has_orig = true; ctx->quad_active = 0;
    coef_close(ctx);
    vip_close(ctx);
    cperm_close(ctx);
    vperm_close(ctx);
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_perm_batch(plsx_ctx* ctx, const int32_t* d_perm_idx, int n, double* d_out, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION) return fail(ctx, PLSX_ERR_STATE, "data not bound for regression");
    if (!d_perm_idx || !d_out || n < 1) return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_perm_batch: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    // (an open permutation series that cannot take the call: refused before anything is computed)
    const bool series = ctx->cperm_active != 0, vseries = ctx->vperm_active != 0;
    if (series && ctx->cperm_n + n > ctx->cperm_cap) {
        char msg[200];
        snprintf(msg, sizeof msg, "plsx_simpls_perm_batch: the open coefficient series holds %lld of %lld permutations, "
                 "%d more do not fit (plsx_simpls_coef_perm_begin)", ctx->cperm_n, ctx->cperm_cap, n);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    if (vseries && ctx->vperm_n + n > ctx->vperm_cap) {
        char msg[200];
        snprintf(msg, sizeof msg, "plsx_simpls_perm_batch: the open VIP series holds %lld of %lld permutations, "
                 "%d more do not fit (plsx_simpls_vip_perm_begin)", ctx->vperm_n, ctx->vperm_cap, n);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    // solver batches are as large as the call: a launch of the component step lasts as long as one
    // wave's latency chain whatever the batch (one wave per resample, up to 8 per SIMD)
    // (8192, or fewer where the solver state of 8192 resamples would exceed half the scratch budget: sd_batch; an open
    // coefficient series adds a permutation's A_p, T S doubles, and its y-loadings to that state, an open VIP series its
    // scaled dual weights, c S doubles)
    const int nb = sd_batch(ctx, 8192, 1, (series ? 8.0 * ctx->T * ((double)ctx->S + ctx->cperm_c) : 0.0) +
                                              (vseries ? 8.0 * ctx->vperm_c * (double)ctx->S : 0.0));
    if (int e = ensure(ctx, ctx->spct, (size_t)nb * ctx->T * ctx->ncomp * 8)) return e;
    if (int e = ensure(ctx, ctx->sc, (size_t)nb * ctx->T * ctx->ncomp * 8)) return e;
    for (int off = 0; off < n; off += nb) {
        const int m = std::min(nb, n - off);
        SdArgs sda;
        // Y is permuted, X is not (BasePLS.make_permutation, base.py:599)
        SdRequest q;
        q.ysrc = d_perm_idx + (size_t)off * ctx->S; q.nres = m;
        q.pctvar = d_out + (size_t)off * ctx->ncomp; q.yload = ptr<double>(ctx->spct); q.cvec = ptr<double>(ctx->sc);
        q.args_out = (series || vseries) ? &sda : nullptr; q.weights_only = series || vseries;
        if (int e = run_simpls_dual(ctx, q, st)) return e;
        if (series)
            if (int e = coef_perm_append(ctx, sda, m, st)) return e;
        if (vseries)
            if (int e = vip_perm_append(ctx, sda, m, st)) return e;
    }
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_crossval_batch(plsx_ctx* ctx, const uint8_t* d_masks, int m, double* d_r, double* d_r2, double* d_sse,
                               void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_crossval_batch: data not bound for regression");
    if (!d_masks || !d_r || !d_r2 || !d_sse || m < 1)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_crossval_batch: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    const int S = ctx->S, T = ctx->T, k = ctx->ncomp;
    // (an open series of counts that cannot take the call: refused before anything is computed)
    if (int e = pred_reserve(ctx, "plsx_simpls_crossval_batch", m, false)) return e;
    if (int e = count_reserve(ctx, "plsx_simpls_crossval_batch", m, st)) return e;
    // solver batches as for the permutations; a split also holds its dense dual weights Vd and Z = Vd . K
    const int nb = std::min(m, sd_batch(ctx, 8192, 1, 2.0 * k * S * 8.0));
    if (int e = cv_scratch(ctx, nb)) return e;
    for (int off = 0; off < m; off += nb) {
        const int ms = std::min(nb, m - off);
        // the fits on the training rows of the splits themselves; one block of counts per split, in submission order
        const CvScores out = {d_r + (size_t)off * k * T, d_r2 + (size_t)off * k * T, d_sse + (size_t)off * (k + 1) * T,
                              nullptr};
        const PredAppend pa = {off, 1, nullptr};
        if (int e = cv_fit_score<false>(ctx, nb, ms, nullptr, d_masks + (size_t)off * S, out, off, 0, 1, st,
                                        [] { return 0; }, nullptr, KGroups(), &pa))
            return e;
    }
    if (ctx->cls_series.active) ctx->cls_series.n += m;
    if (ctx->auc_series.active) ctx->auc_series.n += m;
    if (ctx->pred_series.active) ctx->pred_series.n += m;
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_crossval_perm_batch(plsx_ctx* ctx, const uint8_t* d_masks, int n, const int32_t* d_perm_idx, int m,
                                    double* d_r, double* d_r2, double* d_mse, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_crossval_perm_batch: data not bound for regression");
    if (!d_masks || !d_perm_idx || !d_r || !d_r2 || !d_mse || n < 1 || m < 1)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_crossval_perm_batch: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    const int S = ctx->S, T = ctx->T, k = ctx->ncomp;
    // the pair list: fit f = permutation f / n under split f % n, m n of them (64-bit), cut into solver batches sized
    // as plsx_simpls_crossval_batch sizes its own; a fit also holds its expanded sources and mask (5 S bytes) and
    // its scores until the reduction over the splits
    if (int e = count_reserve(ctx, "plsx_simpls_crossval_perm_batch", m, st)) return e;
    const long long fits = (long long)m * n;
    const size_t kT = (size_t)k * T, per_fit = 2 * kT + (size_t)(k + 1) * T + 1;       // doubles of scores per fit
    const double extra = 2.0 * k * S * 8.0 + 5.0 * S + 8.0 * per_fit;
    int nb = (int)std::min<long long>(fits, sd_batch(ctx, 8192, 1, extra));
    // a tail of less than an eighth of a batch is a whole latency chain for a handful of fits (8200 fits: 8 of them
    // cost a sixth of the 8192 before): spread it over the batches before it where the budget allows -- the bits do not
    // depend on where a batch ends (k_sd_cvp_reduce)
    if (fits > nb && fits % nb != 0 && fits % nb < nb / 8) {
        const long long full = fits / nb, bs = (fits + full - 1) / full;
        if (sd_batch(ctx, (int)bs, 1, extra) == (int)bs) nb = (int)bs;
    }
    if (int e = cv_scratch(ctx, nb)) return e;
    if (int e = ensure(ctx, ctx->cvpsrc, (size_t)nb * S * 5)) return e;
    if (int e = ensure(ctx, ctx->cvpfit, (size_t)nb * per_fit * 8)) return e;
    int* ysrc = ptr<int>(ctx->cvpsrc);
    uint8_t* pmask = reinterpret_cast<uint8_t*>(ysrc + (size_t)nb * S);
    double* fr = ptr<double>(ctx->cvpfit);
    double* fsse = fr + 2 * (size_t)nb * kT;
    const CvScores fs = {fr, fr + (size_t)nb * kT, fsse, fsse + (size_t)nb * (k + 1) * T};
    // the running sums over the splits live in the outputs (k_sd_cvp_reduce)
    HIPCHK(hipMemsetAsync(d_r, 0, (size_t)m * kT * 8, st));
    HIPCHK(hipMemsetAsync(d_r2, 0, (size_t)m * kT * 8, st));
    HIPCHK(hipMemsetAsync(d_mse, 0, (size_t)m * (k + 1) * 8, st));
    for (long long f0 = 0; f0 < fits; f0 += nb) {
        const int ms = (int)std::min<long long>(nb, fits - f0);
        {
            KTimer tm(ctx, KC_CVSCORE, st);
            hipLaunchKernelGGL(k_sd_cvp_expand, dim3(ceil_div(S, 256), ms), dim3(256), 0, st, d_perm_idx, d_masks, S, n, f0,
                               ysrc, pmask);
            LAUNCHCHK();
        }
        // the fits on the training positions of (X, Y[perm]): X keeps its rows, Y takes the permutation's (as
        // plsx_simpls_perm_batch), the test positions are excluded (as plsx_simpls_crossval_batch); one block of counts
        // per permutation: its splits add up in it, in any order
        auto reduce = [&] {
            const int touched = (int)((f0 + ms - 1) / n - f0 / n) + 1;
            hipLaunchKernelGGL(k_sd_cvp_reduce, dim3(ceil_div((int)(2 * kT) + k + 1, 256), touched), dim3(256), 0, st,
                               fs.r, fs.r2, fs.sse, fs.nte, k, T, n, f0, ms, d_r, d_r2, d_mse);
            LAUNCHCHK();
            return 0;
        };
        if (int e = cv_fit_score<true>(ctx, nb, ms, ysrc, pmask, fs, f0 / n, f0, n, st, reduce)) return e;
    }
    if (ctx->cls_series.active) ctx->cls_series.n += m;
    if (ctx->auc_series.active) ctx->auc_series.n += m;
    return PLSX_OK;
} PLSX_CATCH(ctx)

// Nested cross-validation, both entries (perm = false: the observed data, Y keeps its rows, m = 1).  The fit list (k_sd_cvn_expand)
// is cut into solver batches of WHOLE groups of 1 + ni fits, so the selection of a group (k_sd_cvn_select) finds all its
// members' scores in the batch's scratch; observed: the selected scores are the outputs, permuted: they are reduced over
// the outer splits in split order (k_sd_cvn_reduce), which does not care where a batch ends.  With the series of
// plsx_simpls_cvn_class_begin open (PLS-DA) every fit is also classified into a block of its own in scratch, the selection
// runs on those counts (k_sd_cvn_class_select) and the selected blocks go out as the scores do (k_sd_cvn_class_reduce).
static int cvn_entry(plsx_ctx* ctx, const char* who, bool perm, const uint8_t* d_codes, int n, int ni,
                     const int32_t* d_perm_idx, int m, double* d_r, double* d_r2, double* d_mse, int32_t* d_nc, double* d_inner, void* stream)
{
    NEED_DATA();
    const std::string w = who;
    if (ctx->method != PLSX_REGRESSION) return fail(ctx, PLSX_ERR_STATE, w + ": data not bound for regression");
    if (ctx->cls_series.active || ctx->auc_series.active)
        return fail(ctx, PLSX_ERR_STATE, w + ": a series of counts per split is open (plsx_simpls_cv_class_begin / "
                                             "plsx_simpls_cv_auc_begin); the nested selection keeps its counts in the series "
                                             "of plsx_simpls_cvn_class_begin");
    NestedCounts& nc = ctx->ncls_series;
    const bool cls = nc.active != 0;
    if ((perm && !d_perm_idx) || !d_codes || !d_r || !d_r2 || !d_mse || !d_nc || (!perm && !d_inner) || n < 1 || ni < 1 || m < 1)
        return fail(ctx, PLSX_ERR_ARG, w + ": bad arguments");
    if (ctx->cf_q)
        return fail(ctx, PLSX_ERR_UNSUPPORTED, w + ": confounds are bound; the nested selection is not available with "
                                                   "the fold-wise confound regression");
    // (an open series of predictions takes the outer fits of the observed entry, m = 1: n slots; the permuted one none)
    if (!perm)
        if (int e = pred_reserve(ctx, who, n, true)) return e;
    if (cls && nc.n + (perm ? m : n) > nc.cap) {
        char msg[260];
        snprintf(msg, sizeof msg, "%s: the open series of nested counts holds %lld of %lld blocks, %d more do not fit "
                 "(plsx_simpls_cvn_class_begin)", who, nc.n, nc.cap, perm ? m : n);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    const int S = ctx->S, T = ctx->T, k = ctx->ncomp, unit = 1 + ni;
    // (PLS-DA: a fit also holds its blocks of counts, [k][G][G] int32 and [k][G][2] int64, a group its selected ones)
    const size_t GG = (size_t)T * T, G2 = 2 * (size_t)T;
    const bool cauc = cls && nc.auc;
    const size_t cnt_fit = cls ? (size_t)k * (GG * 4 + (cauc ? G2 * 8 : 0)) : 0, cnt_group = cls ? GG * 4 + (cauc ? G2 * 8 : 0) : 0;
    // a fit holds what a fit of plsx_simpls_crossval_perm_batch holds; a group also its selected scores
    const size_t kT = (size_t)k * T, per_fit = 2 * kT + (size_t)(k + 1) * T + 1, per_group = 2 * (size_t)T + 2;
    double extra = 2.0 * k * S * 8.0 + 5.0 * S + 8.0 * per_fit + 8.0 * per_group / unit;
    if (cls) extra += (double)cnt_fit + (double)cnt_group / unit;
    const double fit_bytes = 8.0 * (double)sd_scratch_doubles(S, T, k, simpls_global(ctx)) + extra;
    if ((double)unit * fit_bytes > 0.5 * ctx->scratch_gb * 1073741824.0) {
        char msg[320];
        snprintf(msg, sizeof msg, "%s: one group of 1 + %d fits of %.3g MB each (S = %d, T = %d, k = %d) does not fit half "
                 "the scratch budget of %.3g GB", who, ni, fit_bytes / 1048576.0, S, T, k, ctx->scratch_gb);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    const long long groups = (long long)m * n;
    long long gb = std::min<long long>(groups, std::max(1, sd_batch(ctx, 8192, unit, extra) / unit));   // groups per batch
    // (the tail-spreading rule of plsx_simpls_crossval_perm_batch, in whole groups)
    if (groups > gb && groups % gb != 0 && groups % gb < gb / 8) {
        const long long full = groups / gb, bs = (groups + full - 1) / full;
        if (bs * unit <= 2147483647LL && sd_batch(ctx, (int)(bs * unit), unit, extra) == (int)(bs * unit)) gb = bs;
    }
    const int nb = (int)(gb * unit);
    if (int e = cv_scratch(ctx, nb)) return e;
    if (int e = ensure(ctx, ctx->cvpsrc, (size_t)nb * S * 5)) return e;
    if (int e = ensure(ctx, ctx->cvpfit, ((size_t)nb * per_fit + (size_t)gb * per_group) * 8)) return e;
    int* ysrc = ptr<int>(ctx->cvpsrc);
    uint8_t* pmask = reinterpret_cast<uint8_t*>(ysrc + (size_t)nb * S);
    double* fr = ptr<double>(ctx->cvpfit);
    double* fsse = fr + 2 * (size_t)nb * kT;
    const CvScores fs = {fr, fr + (size_t)nb * kT, fsse, perm ? fsse + (size_t)nb * (k + 1) * T : nullptr};
    double* gr = fsse + (size_t)nb * (k + 1) * T + nb;             // the selected scores of a batch's groups: [gb][T],
    double* gr2 = gr + (size_t)gb * T;                             // [gb][T], [gb] and, as ints, [gb]
    double* gmse = gr2 + (size_t)gb * T;
    int* gnc = reinterpret_cast<int*>(gmse + gb);
    const uint8_t* okx = ctx->has_okx ? ptr<uint8_t>(ctx->okx) : nullptr;
    const uint8_t* oky = ctx->has_oky ? ptr<uint8_t>(ctx->oky) : nullptr;
    // the counts of a batch: the 64-bit blocks first -- [nb][k][G][2] of the fits, [gb][G][2] of the groups -- then the
    // 32-bit ones, [nb][k][G][G] and [gb][G][G]
    long long* fauc = nullptr; long long* gauc = nullptr;
    int* fconf = nullptr; int* gconf = nullptr;
    if (cls) {
        if (int e = ensure(ctx, ctx->cvncnt, (size_t)nb * cnt_fit + (size_t)gb * cnt_group)) return e;
        long long* base = ptr<long long>(ctx->cvncnt);
        if (cauc) { fauc = base; gauc = fauc + (size_t)nb * k * G2; base = gauc + (size_t)gb * G2; }
        fconf = reinterpret_cast<int*>(base);
        gconf = fconf + (size_t)nb * k * GG;
    }
    int* oconf = cls ? nc.conf + (size_t)nc.n * GG : nullptr;                     // this call's blocks of the series
    long long* oauc = cauc ? nc.auc + (size_t)nc.n * G2 : nullptr;
    int* oinner = (cls && !perm && nc.inner) ? nc.inner + (size_t)nc.n * k * GG : nullptr;
    if (cls && perm) {
        // ... and so do the sums of the selected counts (k_sd_cvn_class_reduce)
        HIPCHK(hipMemsetAsync(oconf, 0, (size_t)m * GG * 4, st));
        if (cauc) HIPCHK(hipMemsetAsync(oauc, 0, (size_t)m * G2 * 8, st));
    }
    if (perm) {
        // the running sums over the outer splits live in the outputs (k_sd_cvn_reduce)
        HIPCHK(hipMemsetAsync(d_r, 0, (size_t)m * T * 8, st));
        HIPCHK(hipMemsetAsync(d_r2, 0, (size_t)m * T * 8, st));
        HIPCHK(hipMemsetAsync(d_mse, 0, (size_t)m * 8, st));
        HIPCHK(hipMemsetAsync(d_nc, 0, (size_t)m * k * 4, st));
    }
    for (long long g0 = 0; g0 < groups; g0 += gb) {
        const int mg = (int)std::min<long long>(gb, groups - g0), ms = mg * unit;
        const long long f0 = g0 * unit;
        // observed: the codes are the fits' masks as they lie, [n][1 + ni][S], and Y keeps its rows
        const uint8_t* pm = perm ? pmask : d_codes + (size_t)f0 * S;
        if (perm) {
            KTimer tm(ctx, KC_CVSCORE, st);
            hipLaunchKernelGGL(k_sd_cvn_expand, dim3(ceil_div(S, 256), ms), dim3(256), 0, st, d_perm_idx, d_codes, S, n, ni,
                               f0, ysrc, pmask);
            LAUNCHCHK();
        }
        if (cls) {
            // (the fits' blocks are counted into with integer atomics: zeroed in stream order before them)
            HIPCHK(hipMemsetAsync(fconf, 0, (size_t)ms * k * GG * 4, st));
            if (cauc) HIPCHK(hipMemsetAsync(fauc, 0, (size_t)ms * k * G2 * 8, st));
        }
        auto select = [&] {
            if (cls)
                hipLaunchKernelGGL(k_sd_cvn_class_select, dim3(ceil_div(mg, 4)), dim3(256),
                                   (size_t)4 * (2 * (k + 1) * 8 + (GG + G2) * 4), st, fs.r, fs.r2, fs.sse, fs.nte, pm, okx, oky,
                                   S, k, T, ni, mg, nc.rule, fconf, fauc, perm ? gr : d_r + (size_t)g0 * T,
                                   perm ? gr2 : d_r2 + (size_t)g0 * T, perm ? gmse : d_mse + g0, perm ? gnc : d_nc + g0,
                                   perm ? nullptr : d_inner + (size_t)g0 * (k + 1), perm ? gconf : oconf + (size_t)g0 * GG,
                                   perm ? gauc : (cauc ? oauc + (size_t)g0 * G2 : nullptr),
                                   oinner ? oinner + (size_t)g0 * k * GG : nullptr);
            else
                hipLaunchKernelGGL(k_sd_cvn_select, dim3(ceil_div(mg, 4)), dim3(256), (size_t)4 * (k + 1) * 8, st, fs.r, fs.r2,
                                   fs.sse, fs.nte, pm, okx, oky, S, k, T, ni, mg, perm ? gr : d_r + (size_t)g0 * T,
                                   perm ? gr2 : d_r2 + (size_t)g0 * T, perm ? gmse : d_mse + g0, perm ? gnc : d_nc + g0,
                                   perm ? nullptr : d_inner + (size_t)g0 * (k + 1));
            LAUNCHCHK();
            if (!perm) return 0;
            const int touched = (int)((g0 + mg - 1) / n - g0 / n) + 1;
            hipLaunchKernelGGL(k_sd_cvn_reduce, dim3(ceil_div(2 * T + 1 + k, 256), touched), dim3(256), 0, st, gr, gr2, gmse,
                               gnc, k, T, n, g0, mg, d_r, d_r2, d_mse, d_nc);
            LAUNCHCHK();
            if (cls) {
                hipLaunchKernelGGL(k_sd_cvn_class_reduce, dim3(ceil_div((int)(GG + G2), 256), touched), dim3(256), 0, st,
                                   gconf, gauc, T, n, g0, mg, oconf, oauc);
                LAUNCHCHK();
            }
            return 0;
        };
        const PredAppend pa = {g0, unit, perm ? nullptr : d_nc + g0};
        const FitCounts fc = {fconf, fauc};
        if (int e = perm ? cv_fit_score<true>(ctx, nb, ms, ysrc, pm, fs, 0, 0, 1, st, select, nullptr, KGroups(), nullptr,
                                              cls ? &fc : nullptr)
                         : cv_fit_score<false>(ctx, nb, ms, nullptr, pm, fs, 0, 0, 1, st, select, nullptr, KGroups(), &pa,
                                               cls ? &fc : nullptr))
            return e;
    }
    if (!perm && ctx->pred_series.active) ctx->pred_series.n += n;
    if (cls) nc.n += perm ? m : n;
    return PLSX_OK;
}

int plsx_simpls_crossval_nested_batch(plsx_ctx* ctx, const uint8_t* d_codes, int n, int ni, double* d_r, double* d_r2,
                                      double* d_mse, int32_t* d_ncomp, double* d_inner_mse, void* stream)
try {
    return cvn_entry(ctx, "plsx_simpls_crossval_nested_batch", false, d_codes, n, ni, nullptr, 1, d_r, d_r2, d_mse, d_ncomp,
                     d_inner_mse, stream);
} PLSX_CATCH(ctx)

int plsx_simpls_crossval_nested_perm_batch(plsx_ctx* ctx, const uint8_t* d_codes, int n, int ni, const int32_t* d_perm_idx,
                                           int m, double* d_r, double* d_r2, double* d_mse, int32_t* d_ncomp_count,
                                           void* stream)
try {
    return cvn_entry(ctx, "plsx_simpls_crossval_nested_perm_batch", true, d_codes, n, ni, d_perm_idx, m, d_r, d_r2, d_mse,
                     d_ncomp_count, nullptr, stream);
} PLSX_CATCH(ctx)

// What both fold entries of the confound regression check first and how they group the splits: bytes of one K_s and of
// one fit (solver state, dense dual weights and Z = Vd . K_s, its own Y, `extra`), and as many splits per group as fit
// half the scratch budget with one fit each.
static int cf_fold_plan(plsx_ctx* ctx, const char* who, int n, double extra, double* k_bytes, double* fit_bytes, int* ng)
{
    char msg[320];
    if (ctx->method != PLSX_REGRESSION) {
        snprintf(msg, sizeof msg, "%s: data not bound for regression", who);
        return fail(ctx, PLSX_ERR_STATE, msg);
    }
    if (!ctx->cf_q) {
        snprintf(msg, sizeof msg, "%s: no confounds are bound (plsx_simpls_set_confounds)", who);
        return fail(ctx, PLSX_ERR_STATE, msg);
    }
    if (ctx->cls_series.active || ctx->auc_series.active) {
        snprintf(msg, sizeof msg, "%s: a series of counts is open; the fold-wise confound regression has none", who);
        return fail(ctx, PLSX_ERR_STATE, msg);
    }
    const double S = ctx->S, T = ctx->T, k = ctx->ncomp;
    if (simpls_global(ctx)) {
        snprintf(msg, sizeof msg, "%s: the fold-wise confound regression forms K_s (S x S) per split and runs on the "
                 "on-chip route of the solver only; S = %d (or the simpls_global option) takes the global route, where "
                 "K_s is %.2f GB a split", who, ctx->S, 8.0 * S * S / 1073741824.0);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    *k_bytes = 8.0 * S * S;
    *fit_bytes = 8.0 * (double)sd_scratch_doubles(ctx->S, ctx->T, ctx->ncomp, false) + 2.0 * k * S * 8.0 + 8.0 * S * T + extra;
    const double budget = 0.5 * ctx->scratch_gb * 1073741824.0;
    if (*k_bytes + *fit_bytes > budget) {
        snprintf(msg, sizeof msg, "%s: one K_s (%.3f GB) and one fit (%.3f GB) do not fit half the scratch budget of "
                 "%.6f GB", who, *k_bytes / 1073741824.0, *fit_bytes / 1073741824.0, ctx->scratch_gb);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    *ng = (int)std::min<double>(std::min(n, 8192), std::floor(budget / (*k_bytes + *fit_bytes)));
    return 0;
}

int plsx_simpls_crossval_confound_batch(plsx_ctx* ctx, const uint8_t* d_masks, int n, double* d_r, double* d_r2,
                                        double* d_sse, void* stream)
try {
    NEED_DATA();
    if (!d_masks || !d_r || !d_r2 || !d_sse || n < 1)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_crossval_confound_batch: bad arguments");
    double kb = 0.0, fb = 0.0;
    int ng = 0;
    if (int e = cf_fold_plan(ctx, "plsx_simpls_crossval_confound_batch", n, 0.0, &kb, &fb, &ng)) return e;
    if (int e = pred_reserve(ctx, "plsx_simpls_crossval_confound_batch", n, false)) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    const int S = ctx->S, T = ctx->T, k = ctx->ncomp;
    ng = std::min(ng, 8192);
    if (int e = cv_scratch(ctx, ng)) return e;
    if (int e = ensure(ctx, ctx->cfY, (size_t)ng * S * T * 8)) return e;
    for (int s0 = 0; s0 < n; s0 += ng) {
        // a group of splits: K_s and Y_s of each, then one fit per split on its own (K_s, Y_s)
        const int ns = std::min(ng, n - s0);
        const uint8_t* masks = d_masks + (size_t)s0 * S;
        if (int e = cf_fold_prepare(ctx, masks, s0, ns, st)) return e;
        if (int e = cf_fold_Y(ctx, ns, nullptr, 1, ptr<double>(ctx->cfY), st)) return e;
        const CvScores out = {d_r + (size_t)s0 * k * T, d_r2 + (size_t)s0 * k * T, d_sse + (size_t)s0 * (k + 1) * T, nullptr};
        KGroups kg;
        kg.base = ptr<double>(ctx->cfK); kg.fits = 1;
        const PredAppend pa = {s0, 1, nullptr};
        if (int e = cv_fit_score<false>(ctx, ng, ns, nullptr, masks, out, 0, 0, 1, st, [] { return 0; },
                                        ptr<double>(ctx->cfY), kg, &pa))
            return e;
    }
    if (ctx->pred_series.active) ctx->pred_series.n += n;
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_crossval_confound_perm_batch(plsx_ctx* ctx, const uint8_t* d_masks, int n, const int32_t* d_perm_idx, int m,
                                             double* d_r, double* d_r2, double* d_mse, void* stream)
try {
    NEED_DATA();
    if (!d_masks || !d_perm_idx || !d_r || !d_r2 || !d_mse || n < 1 || m < 1)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_crossval_confound_perm_batch: bad arguments");
    const int S = ctx->S, T = ctx->T, k = ctx->ncomp;
    const size_t kT = (size_t)k * T, per_fit = 2 * kT + (size_t)(k + 1) * T;           // doubles of scores per fit
    double kb = 0.0, fb = 0.0;
    int ng = 0;
    if (int e = cf_fold_plan(ctx, "plsx_simpls_crossval_confound_perm_batch", n, 8.0 * per_fit + S, &kb, &fb, &ng)) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    // the splits in groups of ng, the permutations in chunks of mb: a solver batch is [splits of the group][mb], the
    // fits of one split share its K_s.  (About 8192 fits a batch where the budget allows, as everywhere.)
    const double budget = 0.5 * ctx->scratch_gb * 1073741824.0;
    const int mb = (int)std::max(1.0, std::min<double>(std::min(m, std::max(1, 8192 / ng)),
                                                       std::floor((budget - ng * kb) / (ng * fb))));
    const int nb = ng * mb;
    if (int e = cv_scratch(ctx, nb)) return e;
    if (int e = ensure(ctx, ctx->cfY, (size_t)nb * S * T * 8)) return e;
    if (int e = ensure(ctx, ctx->cffit, (size_t)nb * per_fit * 8 + (size_t)nb * S)) return e;
    double* fr = ptr<double>(ctx->cffit);
    const CvScores fs = {fr, fr + (size_t)nb * kT, fr + 2 * (size_t)nb * kT, nullptr};
    uint8_t* pmask = reinterpret_cast<uint8_t*>(fr + (size_t)nb * per_fit);
    // the running sums over the splits live in the outputs (k_cf_cvp_acc)
    HIPCHK(hipMemsetAsync(d_r, 0, (size_t)m * kT * 8, st));
    HIPCHK(hipMemsetAsync(d_r2, 0, (size_t)m * kT * 8, st));
    HIPCHK(hipMemsetAsync(d_mse, 0, (size_t)m * (k + 1) * 8, st));
    for (int s0 = 0; s0 < n; s0 += ng) {
        const int ns = std::min(ng, n - s0);
        if (int e = cf_fold_prepare(ctx, d_masks + (size_t)s0 * S, s0, ns, st)) return e;
        for (int p0 = 0; p0 < m; p0 += mb) {
            const int mp = std::min(mb, m - p0);
            // fit f = split f / mp of the group under permutation p0 + f % mp: its training mask, its own Y (the
            // permutation is inside it: identity sources, the identity variant of the scores)
            if (int e = cf_expand_masks(ctx, d_masks + (size_t)s0 * S, mp, ns * mp, pmask, st)) return e;
            if (int e = cf_fold_Y(ctx, ns, d_perm_idx + (size_t)p0 * S, mp, ptr<double>(ctx->cfY), st)) return e;
            KGroups kg;
            kg.base = ptr<double>(ctx->cfK); kg.fits = mp;
            auto reduce = [&] {
                return cf_cvp_acc(ctx, fs.r, fs.r2, fs.sse, ns, mp, n, s0 + ns == n, d_r + (size_t)p0 * kT,
                                  d_r2 + (size_t)p0 * kT, d_mse + (size_t)p0 * (k + 1), st);
            };
            if (int e = cv_fit_score<false>(ctx, nb, ns * mp, nullptr, pmask, fs, 0, 0, 1, st, reduce,
                                            ptr<double>(ctx->cfY), kg))
                return e;
        }
    }
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_split_half_batch(plsx_ctx* ctx, const int32_t* d_perm_idx, int np, const uint8_t* d_masks, int ns,
                                 double* d_ucorr, double* d_vcorr, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_split_half_batch: data not bound for regression");
    if (!d_masks || !d_ucorr || !d_vcorr || np < 1 || ns < 1)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_split_half_batch: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    const int S = ctx->S, T = ctx->T, k = ctx->ncomp;
    // Solver batches as for the permutations.  An arrangement also holds its y-loadings and yq (8 k (T + S) bytes) and,
    // per split, the two stacks of half vectors: G and G . K, 2 . 8 . 2 k S bytes.  Where all the splits of even one
    // arrangement do not fit half the scratch budget next to its solver state they go in groups; only a single split
    // that does not fit is refused.  (Rows of one product stay below 2^30.)
    const double per_arr = 8.0 * (double)sd_scratch_doubles(S, T, k, simpls_global(ctx)) + 8.0 * k * ((double)T + S);
    const double per_split = 32.0 * k * (double)S;
    const double budget = 0.5 * ctx->scratch_gb * 1073741824.0;
    if (per_arr + per_split > budget) {
        char msg[320];
        snprintf(msg, sizeof msg, "plsx_simpls_split_half_batch: the solver state of one arrangement (%.0f bytes) and the "
                 "half vectors of one split with their products (32 k S = %.0f bytes for S = %d, k = %d) do not fit half "
                 "the scratch budget of %.6f GB", per_arr, per_split, S, k, ctx->scratch_gb);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    const long long max_rows = 1LL << 30;
    const int nsg = (int)std::min<long long>(std::min<long long>(ns, (long long)((budget - per_arr) / per_split)),
                                             std::max<long long>(1, max_rows / (2 * k)));
    int nb = 1;
    if (nsg == ns) {
        nb = std::min(np, sd_batch(ctx, 8192, 1, 8.0 * k * ((double)T + S) + ns * per_split));
        nb = (int)std::max<long long>(1, std::min<long long>(nb, max_rows / (2LL * k * ns)));
    }
    if (int e = ensure(ctx, ctx->spct, (size_t)nb * (T + 1) * k * 8)) return e;     // pctvar [nb][k], y-loadings [nb][T][k]
    if (int e = ensure(ctx, ctx->sc, (size_t)nb * T * k * 8)) return e;
    if (int e = ensure(ctx, ctx->shq, (size_t)nb * k * ((size_t)T + S) * 8)) return e;
    if (int e = ensure(ctx, ctx->shG, (size_t)nb * nsg * k * 2 * S * 8)) return e;
    if (int e = ensure(ctx, ctx->shKG, (size_t)nb * nsg * k * 2 * S * 8)) return e;
    if (!ctx->has_shrsum) {
        if (int e = ensure(ctx, ctx->shrsum, (size_t)S * 8)) return e;
        KTimer tm(ctx, KC_CVSCORE, st);
        hipLaunchKernelGGL(k_row_sum, dim3(ceil_div(S, 4)), dim3(256), 0, st, ptr<double>(ctx->Xc), ctx->Bpad, S, ctx->B,
                           ptr<double>(ctx->shrsum));
        LAUNCHCHK();
        ctx->has_shrsum = 1;
    }
    ShArgs h;
    memset(&h, 0, sizeof(h));
    h.S = S; h.T = T; h.k = k; h.B = ctx->B; h.ns = ns;
    h.masks = d_masks; h.rsum = ptr<double>(ctx->shrsum);
    h.q = ptr<double>(ctx->shq); h.yq = h.q + (size_t)nb * k * T;
    h.G = ptr<double>(ctx->shG); h.KG = ptr<double>(ctx->shKG);
    h.ucorr = d_ucorr; h.vcorr = d_vcorr;
    const double* K = ptr<double>(ctx->Kmat);
    for (int off = 0; off < np; off += nb) {
        const int ms = std::min(nb, np - off);
        SdArgs a;
        // the fit on all usable rows of (X, Y[perm]): X keeps its rows, Y takes the permutation's (as
        // plsx_simpls_perm_batch; nullptr: the observed arrangement); the scores stay in the batch's state
        SdRequest q;
        q.ysrc = d_perm_idx ? d_perm_idx + (size_t)off * S : nullptr; q.nres = ms;
        q.pctvar = ptr<double>(ctx->spct); q.yload = q.pctvar + (size_t)nb * k; q.cvec = ptr<double>(ctx->sc);
        q.args_out = &a;
        if (int e = run_simpls_dual(ctx, q, st)) return e;
        h.nres = ms; h.a0 = off;
        h.xs = a.xs; h.Y0 = a.Y0; h.XW = a.XW;
        {
            KTimer tm(ctx, KC_CVSCORE, st);
            hipLaunchKernelGGL(k_sd_sh_prep, dim3(ceil_div(ms, 4)), dim3(256), 0, st, h);
            LAUNCHCHK();
        }
        for (int s0 = 0; s0 < ns; s0 += nsg) {
            h.s0 = s0; h.nsg = std::min(nsg, ns - s0);
            const long long waves = (long long)ms * h.nsg;
            const dim3 grid((unsigned)((waves + 3) / 4));
            {
                KTimer tm(ctx, KC_CVSCORE, st);
                hipLaunchKernelGGL(k_sd_sh_expand, grid, dim3(256), 0, st, h);
                LAUNCHCHK();
            }
            // both half vectors of every (arrangement, split, component) against K (symmetric): 4 S^2 k flop per split;
            // never a split contraction: the bits of a row do not depend on how many rows ride with it
            if (int e = nt_strips(ctx, h.G, S, (int)(waves * k * 2), K, S, S, S, ptr<double>(ctx->shKG), S, st, true))
                return e;
            KTimer tm(ctx, KC_CVSCORE, st);
            hipLaunchKernelGGL(k_sd_sh_score, grid, dim3(256), 0, st, h);
            LAUNCHCHK();
        }
    }
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_coef_begin(plsx_ctx* ctx, int c, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_coef_begin: data not bound for regression");
    if (!ctx->has_orig) return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_coef_begin: plsx_simpls_set_original has not been called");
    coef_close(ctx);
    if (c < 1 || c > ctx->ncomp) {
        char msg[120];
        snprintf(msg, sizeof msg, "plsx_simpls_coef_begin: c = %d outside 1 .. n_components = %d", c, ctx->ncomp);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    const int S = ctx->S, T = ctx->T;
    // C_t (T x S x S) and the partial tiles of its batched S x S products (2 x 64 x 64 doubles per tile and behaviour)
    // must fit in free device memory (what an earlier series left allocated counts as free) and in the scratch budget
    const double cbytes = 8.0 * T * (double)S * S;
    const double pbytes = 16.0 * T * (double)round_up(S, 64) * round_up(S, 64);
    double have;
    if (int e = free_bytes(ctx, ctx->Cc, &have)) return e;
    have += (double)ctx->part.bytes;
    const double budget = ctx->scratch_gb * 1073741824.0;
    if (cbytes + pbytes > have || cbytes + pbytes > budget || !nt_sym_fits(S)) {
        char msg[320];
        snprintf(msg, sizeof msg, "plsx_simpls_coef_begin: the coefficient series needs T S^2 doubles (%.2f GB for T = %d, "
                 "S = %d) plus %.2f GB of partial tiles; %.2f GB of device memory are free next to K and the scratch "
                 "budget is %.2f GB (S <= 23168)", cbytes / 1073741824.0, T, S, pbytes / 1073741824.0,
                 have / 1073741824.0, ctx->scratch_gb);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    if (int e = ensure(ctx, ctx->Cc, (size_t)T * S * S * 8)) return e;
    if (int e = ensure(ctx, ctx->Asumc, (size_t)T * S * 8)) return e;
    HIPCHK(hipMemsetAsync(ctx->Cc.p, 0, (size_t)T * S * S * 8, st));
    HIPCHK(hipMemsetAsync(ctx->Asumc.p, 0, (size_t)T * S * 8, st));
    ctx->coef_c = c;
    ctx->coef_active = 1;
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_coef_finish(plsx_ctx* ctx, double* d_bsum, double* d_bsq, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_coef_finish: data not bound for regression");
    if (!ctx->coef_active) return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_coef_finish: no coefficient series is open");
    if (!d_bsum || !d_bsq) return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_coef_finish: null output");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    const long long n = ctx->coef_n;
    coef_close(ctx);
    if (n == 0) return PLSX_OK;
    // ONE pass over the features: bsum += Xc^T (sum_b A_b), bsq[f][t] += x_f^T C_t x_f
    const QuadSet qs = coef_set(ctx);
    return quad_finish(ctx, d_bsum, d_bsq, st, &qs);
} PLSX_CATCH(ctx)

int plsx_simpls_coef_keep(plsx_ctx* ctx, double* d_A, long long capacity)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_coef_keep: data not bound for regression");
    if (!ctx->coef_active) return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_coef_keep: no coefficient series is open");
    if (!d_A || capacity < 1) return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_coef_keep: null buffer or capacity < 1");
    ctx->keepA = d_A; ctx->keep_cap = capacity; ctx->keep_n = 0;
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_coef_ci(plsx_ctx* ctx, const double* d_A, long long n, int i_lo, double g_lo, int i_hi, double g_hi,
                        double* d_lo, double* d_hi, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_coef_ci: data not bound for regression");
    if (!d_A || !d_lo || !d_hi || n < 1 || i_lo < 0 || i_hi < 0 || i_lo >= n || i_hi >= n)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_coef_ci: null pointer, n < 1 or an index outside 0 .. n - 1");
    const int S = ctx->S, T = ctx->T, B = ctx->B;
    char msg[400];
    if (n > 16384) {
        snprintf(msg, sizeof msg, "plsx_simpls_coef_ci: n = %lld bootstraps per series; the percentile kernels take at "
                 "most 16384 (B = %d, T = %d: %.1f GB of series, which no host path forms either)", n, B, T,
                 8.0 * B * T * (double)n / 1073741824.0);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    long long fc;
    if (int e = ci_chunk(ctx, "plsx_simpls_coef_ci", n, 8.0 * (double)n * T * S, 8.0 * T * (double)n, "T", T, &fc))
        return e;
    if (fc * T > 2147483647LL)                         // (series per selection launch: one block each, grid x)
        return fail(ctx, PLSX_ERR_UNSUPPORTED, "plsx_simpls_coef_ci: more than 2^31 series in one chunk");
    if (int e = ensure(ctx, ctx->cichunk, (size_t)fc * T * (size_t)n * 8)) return e;
    CoefProdArgs a;
    a.Xc = ptr<double>(ctx->Xc); a.ldx = ctx->Bpad;
    a.A = d_A; a.S = S; a.T = T; a.n = (int)n; a.B = B;
    a.out = ptr<double>(ctx->cichunk);
    for (long long f0 = 0; f0 < B; f0 += fc) {
        a.f0 = (int)f0; a.fc = (int)std::min<long long>(fc, B - f0);
        {
            KTimer tm(ctx, KC_COEFPROD, st);
            hipLaunchKernelGGL(k_coef_prod, dim3(ceil_div(a.fc, 128), ceil_div(a.n, 64), T), dim3(256), 0, st, a);
            LAUNCHCHK();
        }
        if (int e = run_percentile(ctx, a.out, (long long)a.fc * T, a.n, i_lo, g_lo, i_hi, g_hi,
                                   d_lo + (size_t)f0 * T, d_hi + (size_t)f0 * T, st))
            return e;
    }
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_coef_perm_test(plsx_ctx* ctx, const double* d_A, long long n, const double* d_obs, int standardise,
                               int32_t* d_count, double* d_max, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_coef_perm_test: data not bound for regression");
    if (!d_A || !d_obs || !d_count || !d_max || n < 1)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_coef_perm_test: null pointer or n < 1");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    if (standardise)
        if (int e = col_sd(ctx, st)) return e;
    // the partial maxima stay next to the caller's stack inside the scratch budget and in free device memory (what an
    // earlier pass left allocated counts as free)
    double have;
    if (int e = free_bytes(ctx, ctx->cppart, &have)) return e;
    const double stack = 8.0 * (double)n * ctx->T * ctx->S;
    const double room = std::min(ctx->scratch_gb * 1073741824.0 - stack, have);
    return coef_perm_run(ctx, d_A, n, d_obs, standardise ? ptr<double>(ctx->colsd) : nullptr, d_count, d_max, room,
                         "plsx_simpls_coef_perm_test", st);
} PLSX_CATCH(ctx)

int plsx_simpls_coef_perm_begin(plsx_ctx* ctx, int c, const double* d_obs, int standardise, int32_t* d_count,
                                double* d_max, long long capacity)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_coef_perm_begin: data not bound for regression");
    if (!ctx->has_orig)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_coef_perm_begin: plsx_simpls_set_original has not been called");
    cperm_close(ctx);
    if (c < 1 || c > ctx->ncomp) {
        char msg[120];
        snprintf(msg, sizeof msg, "plsx_simpls_coef_perm_begin: c = %d outside 1 .. n_components = %d", c, ctx->ncomp);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    if (!d_obs || !d_count || !d_max || capacity < 1)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_coef_perm_begin: null pointer or capacity < 1");
    HIPCHK(hipSetDevice(ctx->device));
    if (standardise) {                                 // once per series; the entry takes no stream: fenced both ways
        HIPCHK(hipDeviceSynchronize());
        if (int e = col_sd(ctx, nullptr)) return e;
        HIPCHK(hipStreamSynchronize(nullptr));
    }
    ctx->cperm_c = c; ctx->cperm_obs = d_obs; ctx->cperm_std = standardise ? 1 : 0;
    ctx->cperm_count = d_count; ctx->cperm_max = d_max; ctx->cperm_cap = capacity; ctx->cperm_n = 0;
    ctx->cperm_active = 1;
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_coef_perm_end(plsx_ctx* ctx)
try {
    if (!ctx) return PLSX_ERR_ARG;
    cperm_close(ctx);
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_vip_perm_test(plsx_ctx* ctx, const double* d_G, long long n, int c, const double* d_obs,
                              int32_t* d_count, double* d_max, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_vip_perm_test: data not bound for regression");
    if (!d_G || !d_obs || !d_count || !d_max || n < 1)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_vip_perm_test: null pointer or n < 1");
    if (c < 1 || c > ctx->ncomp) {
        char msg[120];
        snprintf(msg, sizeof msg, "plsx_simpls_vip_perm_test: c = %d outside 1 .. n_components = %d", c, ctx->ncomp);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    // the partial maxima stay next to the caller's stack inside the scratch budget and in free device memory (what an
    // earlier pass left allocated counts as free)
    double have;
    if (int e = free_bytes(ctx, ctx->cppart, &have)) return e;
    const double stack = 8.0 * (double)n * c * ctx->S;
    const double room = std::min(ctx->scratch_gb * 1073741824.0 - stack, have);
    return vip_perm_run(ctx, d_G, n, c, d_obs, d_count, d_max, room, "plsx_simpls_vip_perm_test", st);
} PLSX_CATCH(ctx)

int plsx_simpls_vip_perm_begin(plsx_ctx* ctx, int c, const double* d_obs, int32_t* d_count, double* d_max,
                               long long capacity)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_vip_perm_begin: data not bound for regression");
    if (!ctx->has_orig)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_vip_perm_begin: plsx_simpls_set_original has not been called");
    vperm_close(ctx);
    if (c < 1 || c > ctx->ncomp) {
        char msg[120];
        snprintf(msg, sizeof msg, "plsx_simpls_vip_perm_begin: c = %d outside 1 .. n_components = %d", c, ctx->ncomp);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    if (!d_obs || !d_count || !d_max || capacity < 1)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_vip_perm_begin: null pointer or capacity < 1");
    ctx->vperm_c = c; ctx->vperm_obs = d_obs;
    ctx->vperm_count = d_count; ctx->vperm_max = d_max; ctx->vperm_cap = capacity; ctx->vperm_n = 0;
    ctx->vperm_active = 1;
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_vip_perm_end(plsx_ctx* ctx)
try {
    if (!ctx) return PLSX_ERR_ARG;
    vperm_close(ctx);
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_vip_keep(plsx_ctx* ctx, int c, double* d_G, long long capacity)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_vip_keep: data not bound for regression");
    if (!ctx->has_orig) return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_vip_keep: plsx_simpls_set_original has not been called");
    vip_close(ctx);
    if (c < 1 || c > ctx->ncomp) {
        char msg[120];
        snprintf(msg, sizeof msg, "plsx_simpls_vip_keep: c = %d outside 1 .. n_components = %d", c, ctx->ncomp);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    if (!d_G || capacity < 1) return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_vip_keep: null buffer or capacity < 1");
    ctx->vipG = d_G; ctx->vip_cap = capacity; ctx->vip_n = 0; ctx->vip_c = c;
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_vip_ci(plsx_ctx* ctx, const double* d_G, long long n, int c, int i_lo, double g_lo, int i_hi, double g_hi,
                       double* d_sd, double* d_lo, double* d_hi, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_vip_ci: data not bound for regression");
    if (!d_G || !d_sd || !d_lo || !d_hi || n < 1 || c < 1 || i_lo < 0 || i_hi < 0 || i_lo >= n || i_hi >= n)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_vip_ci: null pointer, n < 1, c < 1 or an index outside 0 .. n - 1");
    const int S = ctx->S, B = ctx->B;
    char msg[400];
    if (n > 16384) {
        snprintf(msg, sizeof msg, "plsx_simpls_vip_ci: n = %lld bootstraps per series; the percentile kernels take at "
                 "most 16384 (B = %d: %.1f GB of series, which no host path forms either)", n, B,
                 8.0 * B * (double)n / 1073741824.0);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    long long fc;
    if (int e = ci_chunk(ctx, "plsx_simpls_vip_ci", n, 8.0 * (double)n * c * S, 8.0 * (double)n, "c", c, &fc))
        return e;
    if (int e = ensure(ctx, ctx->cichunk, (size_t)fc * (size_t)n * 8)) return e;
    VipProdArgs a;
    a.Xc = ptr<double>(ctx->Xc); a.ldx = ctx->Bpad;
    a.G = d_G; a.S = S; a.c = c; a.n = (int)n; a.B = B;
    a.out = ptr<double>(ctx->cichunk);
    for (long long f0 = 0; f0 < B; f0 += fc) {
        a.f0 = (int)f0; a.fc = (int)std::min<long long>(fc, B - f0);
        {
            KTimer tm(ctx, KC_COEFPROD, st);
            hipLaunchKernelGGL(k_vip_prod, dim3(ceil_div(a.fc, 128), ceil_div(a.n, 64)), dim3(256), 0, st, a);
            LAUNCHCHK();
            // (the moments read the series the product just wrote: they count with it)
            hipLaunchKernelGGL(k_vip_moments, dim3(a.fc), dim3(256), 0, st, a.out, a.n, d_sd + (size_t)f0);
            LAUNCHCHK();
        }
        if (int e = run_percentile(ctx, a.out, (long long)a.fc, a.n, i_lo, g_lo, i_hi, g_hi, d_lo + (size_t)f0,
                                   d_hi + (size_t)f0, st))
            return e;
    }
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_set_classes(plsx_ctx* ctx, const int32_t* d_class, int G, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_set_classes: data not bound for regression");
    count_close(ctx->cls_series);
    count_close(ctx->auc_series);
    ncls_close(ctx->ncls_series);
    ctx->has_cls = 0;
    if (!d_class) return PLSX_OK;                      // (a null pointer clears the binding)
    char msg[200];
    if (G != ctx->T) {
        snprintf(msg, sizeof msg, "plsx_simpls_set_classes: G = %d classes, but the bound Y has T = %d indicator columns",
                 G, ctx->T);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    if (G > 32) {
        snprintf(msg, sizeof msg, "plsx_simpls_set_classes: G = %d classes; k_sd_cv_class keeps one y-loading per class "
                 "in registers and G x G counters per wave in LDS, at most 32 classes", G);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<int32_t> h(ctx->S);
    HIPCHK(hipMemcpyAsync(h.data(), d_class, (size_t)ctx->S * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < ctx->S; ++i)
        if (h[i] < 0 || h[i] >= G) {
            snprintf(msg, sizeof msg, "plsx_simpls_set_classes: row %d has class code %d outside 0 .. %d", i, h[i], G - 1);
            return fail(ctx, PLSX_ERR_ARG, msg);
        }
    // the bound Y is the indicator matrix minus its column means over all S rows: the class frequencies n_g / S
    std::vector<double> freq(G, 0.0);
    for (int i = 0; i < ctx->S; ++i) freq[h[i]] += 1.0;
    for (double& f : freq) f /= ctx->S;
    if (int e = ensure(ctx, ctx->cls, (size_t)ctx->S * 4)) return e;
    if (int e = ensure(ctx, ctx->clsfreq, (size_t)G * 8)) return e;
    HIPCHK(hipMemcpyAsync(ctx->cls.p, d_class, (size_t)ctx->S * 4, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->clsfreq.p, freq.data(), (size_t)G * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    ctx->has_cls = 1;
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_cv_class_begin(plsx_ctx* ctx, int32_t* d_conf, long long capacity)
try {
    return count_begin(ctx, false, d_conf, capacity);
} PLSX_CATCH(ctx)

int plsx_simpls_cv_class_end(plsx_ctx* ctx)
try {
    return count_end(ctx, false);
} PLSX_CATCH(ctx)

int plsx_simpls_cv_auc_begin(plsx_ctx* ctx, int64_t* d_auc, long long capacity)
try {
    return count_begin(ctx, true, d_auc, capacity);
} PLSX_CATCH(ctx)

int plsx_simpls_cv_auc_end(plsx_ctx* ctx)
try {
    return count_end(ctx, true);
} PLSX_CATCH(ctx)

int plsx_simpls_cvn_class_begin(plsx_ctx* ctx, int rule, int32_t* d_conf, int64_t* d_auc, int32_t* d_inner_conf,
                                long long capacity)
try {
    NEED_DATA();
    const std::string who = "plsx_simpls_cvn_class_begin";
    if (ctx->method != PLSX_REGRESSION) return fail(ctx, PLSX_ERR_STATE, who + ": data not bound for regression");
    if (!ctx->has_cls) return fail(ctx, PLSX_ERR_STATE, who + ": plsx_simpls_set_classes has not been called");
    ncls_close(ctx->ncls_series);
    if (!d_conf || capacity < 1) return fail(ctx, PLSX_ERR_ARG, who + ": null buffer or capacity < 1");
    if (rule != PLSX_CVN_SELECT_MSE && rule != PLSX_CVN_SELECT_ACCURACY && rule != PLSX_CVN_SELECT_BALANCED)
        return fail(ctx, PLSX_ERR_ARG, who + ": unknown selection rule");
    NestedCounts& s = ctx->ncls_series;
    s.rule = rule; s.conf = d_conf; s.auc = reinterpret_cast<long long*>(d_auc); s.inner = d_inner_conf;
    s.cap = capacity; s.n = 0;
    s.active = 1;
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_cvn_class_end(plsx_ctx* ctx)
try {
    if (!ctx) return PLSX_ERR_ARG;
    ncls_close(ctx->ncls_series);
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_cv_pred_begin(plsx_ctx* ctx, int c, int32_t* d_ncomp, double* d_pred, double* d_true, long long capacity)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION)
        return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_cv_pred_begin: data not bound for regression");
    pred_close(ctx->pred_series);
    if (!d_pred || capacity < 1) return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_cv_pred_begin: null stack or capacity < 1");
    char msg[320];
    if (c < 0 || c > ctx->ncomp) {
        snprintf(msg, sizeof msg, "plsx_simpls_cv_pred_begin: c = %d outside 1 .. k = %d (0: the count the nested selection "
                 "chooses per fit)", c, ctx->ncomp);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    // the stack is the caller's, and so large that the batches beside it must still find their scratch
    const double bytes = 8.0 * ctx->S * ctx->T * (double)capacity * (d_true ? 2.0 : 1.0);
    const double budget = ctx->scratch_gb * 1073741824.0;
    if (bytes > budget) {
        snprintf(msg, sizeof msg, "plsx_simpls_cv_pred_begin: a stack of %lld fits x T = %d x S = %d doubles%s is %.3f GB, "
                 "beyond the scratch budget of %.3f GB (plsx_set_scratch)", capacity, ctx->T, ctx->S,
                 d_true ? " with the observed values beside it" : "", bytes / 1073741824.0, ctx->scratch_gb);
        return fail(ctx, PLSX_ERR_UNSUPPORTED, msg);
    }
    PredSeries& s = ctx->pred_series;
    s.c = c; s.ncomp = d_ncomp; s.pred = d_pred; s.ytrue = d_true; s.cap = capacity; s.n = 0;
    s.active = 1;
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_cv_pred_end(plsx_ctx* ctx)
try {
    if (!ctx) return PLSX_ERR_ARG;
    pred_close(ctx->pred_series);
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_set_row_masks(plsx_ctx* ctx, const uint8_t* d_okx, const uint8_t* d_oky, void* stream)
try {
    NEED_DATA();
    if (ctx->method != PLSX_REGRESSION) return fail(ctx, PLSX_ERR_STATE, "data not bound for regression");
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    ctx->has_okx = ctx->has_oky = false;
    if (d_okx) {
        if (int e = ensure(ctx, ctx->okx, ctx->S)) return e;
        HIPCHK(hipMemcpyAsync(ctx->okx.p, d_okx, ctx->S, hipMemcpyDeviceToDevice, st));
        ctx->has_okx = true;
        // the number of usable rows of X: the denominator of the feature scale (k_col_sd)
        std::vector<uint8_t> h(ctx->S);
        HIPCHK(hipMemcpyAsync(h.data(), d_okx, ctx->S, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ctx->n_okx = 0;
        for (uint8_t v : h) ctx->n_okx += v ? 1 : 0;
    }
    if (d_oky) {
        if (int e = ensure(ctx, ctx->oky, ctx->S)) return e;
        HIPCHK(hipMemcpyAsync(ctx->oky.p, d_oky, ctx->S, hipMemcpyDeviceToDevice, st));
        ctx->has_oky = true;
    }
    HIPCHK(hipStreamSynchronize(st));
    return PLSX_OK;
} PLSX_CATCH(ctx)

int plsx_simpls_boot_batch(plsx_ctx* ctx, const int32_t* d_boot_idx, const double* d_ystack, int n,
                           double* d_usum, double* d_usq, double* d_yload, void* stream)
try {
    NEED_ORIG();
    if (ctx->method != PLSX_REGRESSION) return fail(ctx, PLSX_ERR_STATE, "data not bound for regression");
    if (!d_boot_idx || !d_usum || !d_usq || !d_yload || n < 1)
        return fail(ctx, PLSX_ERR_ARG, "plsx_simpls_boot_batch: bad arguments");
    // (a kept coefficient stack that cannot take the call's bootstraps: refused before anything is computed)
    if (ctx->coef_active && ctx->keepA && ctx->keep_n + n > ctx->keep_cap) {
        char msg[200];
        snprintf(msg, sizeof msg, "plsx_simpls_boot_batch: the kept coefficient stack holds %lld of %lld bootstraps, "
                 "%d more do not fit (plsx_simpls_coef_keep)", ctx->keep_n, ctx->keep_cap, n);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    if (ctx->vipG && ctx->vip_n + n > ctx->vip_cap) {
        char msg[200];
        snprintf(msg, sizeof msg, "plsx_simpls_boot_batch: the kept VIP stack holds %lld of %lld bootstraps, "
                 "%d more do not fit (plsx_simpls_vip_keep)", ctx->vip_n, ctx->vip_cap, n);
        return fail(ctx, PLSX_ERR_ARG, msg);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIPCHK(hipSetDevice(ctx->device));
    const int k = ctx->ncomp, T = ctx->T;
    const int nb = launch_groups(ctx, n, ctx->npg) * ctx->npg;          // cross-product batch (R scratch)
    // the dual solver runs on batches of up to 8192 bootstraps (whole groups; one wave per bootstrap, up to 8 per
    // SIMD: a launch of the component step lasts one wave's latency chain whatever the batch, so 5000 bootstraps
    // in one batch cost little more than 4096 -- and less than 4096 + 904), each followed by the cross-product
    // batches that turn its dual weights into feature-space weights
    int nbs = std::max(nb, (8192 / ctx->npg) * ctx->npg);
    if (ctx->quad_active) {        // V of a solver batch, dense and transposed, within 1 GB each
        if (!simpls_single_pass(ctx)) return fail(ctx, PLSX_ERR_STATE, "plsx_simpls_boot_batch: open series on a route that left it");
        nbs = (int)std::max<long long>(ctx->npg, std::min<long long>(nbs, (1LL << 30) / ((long long)k * ctx->S * 8)));
    }
    // ... and within half the scratch budget with the solver state and the batch's A operand (or dense V): unchanged
    // wherever that already held
    nbs = sd_batch(ctx, nbs, ctx->npg,
                   ctx->quad_active ? 8.0 * k * ctx->S : 8.0 * (double)ctx->group_stride / std::max(ctx->npg, 1));
    if (int e = ensure(ctx, ctx->spct, (size_t)std::min(n, nbs) * k * 8)) return e;
    if (int e = ensure(ctx, ctx->sc, (size_t)std::min(n, nbs) * T * k * 8)) return e;
    for (int off = 0; off < n; off += nbs) {
        const int ms = std::min(nbs, n - off);
        const int* idx = d_boot_idx + (size_t)off * ctx->S;
        double* yl = d_yload + (size_t)off * T * k;
        const double* yst = d_ystack ? d_ystack + (size_t)off * ctx->S * T : nullptr;
        const bool single = simpls_single_pass(ctx);
        SdArgs sda;                      // the batch's solver state, for an open coefficient series or a kept VIP stack
        const bool want_state = ctx->coef_active || ctx->vipG;
        SdRequest q;
        q.xsrc = q.ysrc = idx; q.nres = ms; q.scatter = true;
        q.pctvar = ptr<double>(ctx->spct); q.yload = yl; q.cvec = ptr<double>(ctx->sc);
        q.ystack = yst; q.args_out = want_state ? &sda : nullptr;
        if (ctx->quad_active) {
            // quadratic-form route: the aligned dual weights stay in dual space (plsx_boot_finish passes the features)
            if (int e = ensure(ctx, ctx->Vdq, (size_t)ms * k * ctx->S * 8)) return e;
            q.align_signs = true; q.Vd = ptr<double>(ctx->Vdq);
            if (int e = run_simpls_dual(ctx, q, st)) return e;
            if (ctx->timing) ctx->timed_units += ms;
            if (int e = quad_accumulate(ctx, ms, st)) return e;
            if (ctx->coef_active)
                if (int e = coef_accumulate(ctx, sda, ms, st)) return e;
            if (ctx->vipG)
                if (int e = vip_append(ctx, sda, ms, st)) return e;
            continue;
        }
        q.align_signs = single;
        if (int e = run_simpls_dual(ctx, q, st)) return e;
        // (the solver state of the batch outlives the feature passes below: they work in buffers of their own)
        if (ctx->coef_active)
            if (int e = coef_accumulate(ctx, sda, ms, st)) return e;
        if (ctx->vipG)
            if (int e = vip_append(ctx, sda, ms, st)) return e;
        if (single) {
            // ONE feature pass, no R: x_weights = X0_r^T (flip . Wd) accumulated per group in the epilogue
            const int MT = 24, NW = 4, npg_w = (MT * 16) / k;
            if (npg_w != ctx->npg) return fail(ctx, PLSX_ERR_STATE, "simpls single pass: group layout mismatch");
            if (ctx->npg_w != npg_w || ctx->out_row_w.bytes < (size_t)MT * 16 * sizeof(int)) {
                std::vector<int> lmap(MT * 16, -1);
                for (int rr = 0; rr < npg_w; ++rr)
                    for (int l = 0; l < k; ++l) lmap[rr * k + l] = l;
                if (int e = ensure(ctx, ctx->out_row_w, lmap.size() * sizeof(int))) return e;
                HIPCHK(hipMemcpy(ctx->out_row_w.p, lmap.data(), lmap.size() * sizeof(int), hipMemcpyHostToDevice));
                ctx->npg_w = npg_w;
            }
            const int gtot = ceil_div(ms, npg_w);
            // groups per pass: partial (sum, sum of squares) tiles [groups][B][k] x 2 within a quarter of the scratch
            const double per_group = 2.0 * ctx->B * (double)k * 8.0;
            const int gmax = (int)std::max(1.0, std::min(512.0, ctx->scratch_gb * 1073741824.0 / 4.0 / per_group));
            for (int g0 = 0; g0 < gtot; g0 += gmax) {
                const int groups = std::min(gmax, gtot - g0);
                if (int e = ensure(ctx, ctx->psum, (size_t)groups * ctx->B * k * 8)) return e;
                if (int e = ensure(ctx, ctx->psq, (size_t)groups * ctx->B * k * 8)) return e;
                if (ctx->timing) ctx->timed_units += std::min(ms - g0 * npg_w, groups * npg_w);
                if (int e = launch_xprod_acc(ctx, ptr<double>(ctx->Afrag) + (size_t)g0 * ctx->group_stride, ctx->group_stride,
                                             groups, k, st))
                    return e;
                KTimer tm(ctx, KC_UROT, st);
                const long long count = (long long)ctx->B * k;
                hipLaunchKernelGGL(k_add_splits, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st,
                                   ptr<double>(ctx->psum), ptr<double>(ctx->psq), groups, count, d_usum, d_usq);
                LAUNCHCHK();
            }
            continue;
        }
        for (int o2 = 0; o2 < ms; o2 += nb) {
            const int m = std::min(nb, ms - o2);
            ctx->afrag_group0 = o2 / ctx->npg;
            int e = run_xprod(ctx, idx, idx, m, st, true);                    // R_r = W_r^T (k x B)
            ctx->afrag_group0 = 0;
            if (e) return e;
            // sign alignment against the (centred) original weights
            if (int e2 = run_gram_ex(ctx, m, 2, ptr<double>(ctx->U0T), k, ptr<double>(ctx->Pm), st)) return e2;
            hipLaunchKernelGGL(k_simpls_signs, dim3(m), dim3(256), 0, st, ptr<double>(ctx->Pm), k, T, ctx->nks_t,
                               ctx->LT, ptr<double>(ctx->Mfrag), yl + (size_t)o2 * T * k);
            LAUNCHCHK();
            if (int e2 = run_urot(ctx, m, d_usum, d_usq, nullptr, st)) return e2;
        }
    }
    return PLSX_OK;
} PLSX_CATCH(ctx)

}  // extern "C"

