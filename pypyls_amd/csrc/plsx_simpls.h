// plsx_simpls.h -- SIMPLS (de Jong 1993) per resample in the S-dimensional dual
// space.  Restates pyls/types/regression.py:56-186 (simpls), :279-373
// (_single_boot / _single_perm).
//
// Every B-long vector SIMPLS manipulates lies in span(X0^T): with
// K = X0 X0^T (S x S),
//     r_c = X0^T a_c,  t_c = K a_c,  p_c = X0^T t_c,  v_c = X0^T beta_c,
//     Cov_c = X0^T Yd_c  with  Yd_{c+1} = Yd_c - beta_c (beta_c^T K Yd_c),
//     Cov_c^T Cov_c = Yd_c^T K Yd_c = H_c,   H_{c+1} = H_c - g g^T, g = (K beta_c)^T Yd_c.
// A resample (row sources xsrc / ysrc) only changes which entries of K are
// gathered and the centring: K_r = Jc K[xs, xs] Jc, Y0_r = Jc Y[ys].
// The permutation statistic (pctvar of Y, regression.py:369) needs nothing
// B-sized; a bootstrap needs x_weights = X0_r^T Wd (B x k), obtained by
// scattering the dual weights into the A operand of k_xprod.
//
// Batched formulation.  Every product with K_r is gather(K . scatter(v)): with
// P_r the S x S selection matrix of the resample (row p picks xs_p),
//     K_r v = Jc P_r K P_r^T Jc v,
// i.e. the SAME K for every resample once the centred vector is scattered to
// subject space (w[i] = sum over positions p with xs_p = i).  The products of a
// whole batch of resamples are therefore ONE GEMM against K per step
// (k_nt_gemm, MFMA) instead of one pass over K per resample and product
// (round 1: a GEMV per product, 63 % of the solver streaming K through the fabric):
//     Z_0 = K_r Yd_0     T columns per resample, plus K . cnt for the mean of the
//                        un-centred scores: (T + 1) x nres columns       GEMM 0
//     K_r beta_c         one column per resample and component          GEMM c
// The other product of the classical recursion, t_c = K_r a_c with
// a_c = Yd c / s, is free: t_c = (K_r Yd) c / s = Z c / s, and Z = K_r Yd is
// carried along.  Deflation is kept in factored form --
//     Yd = Y0 - sum_j beta_j g_j^T,  Z = Z0 - sum_j (K beta_j) g_j^T,  H -= g g^T
// -- so Y0 / Z0 are written once.  (The reference re-applies the deflation
// against the earlier basis vectors, regression.py:148-150; in exact
// arithmetic those coefficients vanish and they are not re-applied here.)
// Kernels, ONE WAVEFRONT per resample (round 3; round 2 ran one 256-thread block per
// resample, whose ~100 block barriers per component -- Jacobi steps, block-wide sums, the
// 2 c sequential dot products of the Gram-Schmidt pass -- left the kernels 10 x off their
// memory traffic):
//   k_sd_init -> [GEMM 0] -> k_sd_post0 -> { k_sd_step(c) -> [GEMM c] } x k -> k_sd_final
//   cross-validation appends:  k_sd_final (dual weights dense, Vd) -> [Z = Vd . K] -> k_sd_cv_score
//   split-half appends:  k_sd_sh_prep -> { k_sd_sh_expand -> [KG = G . K] -> k_sd_sh_score } per group of splits
//   an open coefficient series appends to a bootstrap batch:  k_sd_coef (A_b = sum_{j <= c} wd_j q_j^T, dense)
//   a kept VIP stack appends to a bootstrap batch:  k_sd_vip (the scaled dual weights of the first c components, dense)
// k_sd_step(c) finishes component c - 1 (what follows its K beta product: basis pair,
// deflation coefficients, H -= g g^T) and opens component c (leading eigenpair of H, scores,
// dual weights, new basis vector scattered for GEMM c); the last component needs no
// product.  Everything a resample owns is touched by its wave only: reductions are
// wavefront shuffles, the S-long vectors stay with the lane that owns position p
// (p = lane + 64 i), the small matrices (H, G, ...) live in the wave's slice of LDS.
// S x T matrices are stored T-major ([t][p]) so that lanes over p read 512 contiguous bytes.
#pragma once
#include "plsx_kernels.h"

__device__ __forceinline__ double wave_sum(double v)
{
    v += dpp_f64<SD_DPP_XOR1>(v);
    v += dpp_f64<SD_DPP_XOR2>(v);
    v += dpp_f64<SD_DPP_HALF_MIRROR>(v);
    v += dpp_f64<SD_DPP_ROW_MIRROR>(v);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// LDS written by some lanes of the wave, read by others: the wave's DS operations execute in
// order, the compiler must not move them across
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct SdArgs {
    int S, T, k, c;             // c: current component
    int nres;
    const double* Yc;           // S x T globally centred Y (or a stack, y_stride != 0)
    long long y_stride;
    const uint8_t* okx;         // [S] usable X rows or nullptr
    const uint8_t* oky;         // [S] usable Y rows or nullptr
    const int* xsrc;            // [nres][S] or nullptr (identity)
    const int* ysrc;            // [nres][S] or nullptr
    // per-resample state (library scratch)
    int* xs;                    // [nres][S] X source of position p, -1 = position excluded
    int* ys;                    // [nres][S]
    double* Y0;                 // [nres][T][S]  resample-centred Y, T-major
    double* Z0;                 // [nres][T][S]  K_r Y0, T-major
    double* BT;                 // [nres][k][S]  beta_j (centred, normalised)
    double* KB;                 // [nres][k][S]  K_r beta_j
    double* XW;                 // [nres][k][S]  X[xs] w_j (un-centred)
    double* WD;                 // [nres][k][S]  dual weights (centred)
    double* va;                 // [nres][S]  centred beta of the open component
    double* kcpos;              // [nres][S]  (K cnt)[xs_p]
    double* H;                  // [nres][T][T]
    double* H0;                 // [nres][T][T]
    double* G;                  // [nres][k][T]  deflation coefficients g_j
    double* gY0;                // [nres][k][T]  (K beta_j)^T Y0
    double* scal;               // [nres][4]: n included, sum Y0^2
    double* ymean;              // [nres][T]: column means of Y[ys] over the included positions (Y0 = Y[ys] - ymean there)
    double* Wt;                 // GEMM operand rows (vectors in subject space), S doubles each
    double* Zt;                 // GEMM result rows
    double* pctvar;             // [nres][k]   sum(y_loadings^2) / sum(Y0^2)
    double* yload;              // [nres][T][k]  Y[ys]^T (X[xs] W), signs not yet aligned
    double* cvec;               // [nres][T][k]  right singular vectors c_c (sign rule when B <= T)
    double* Afrag;              // dual weights scattered into k_xprod's A operand (or nullptr)
    double* Vd;                 // or: scattered dense, [nres][k][S] (every entry written; quadratic-form route, cross-validation), or nullptr
    const double* Qs;           // [S][k] Xc . W0c^T (centred original weights): bootstrap sign alignment in dual space, or nullptr
    size_t group_stride;
    GroupLayout lay;
    int jacobi_eig;             // 1: full one-sided Jacobi for the leading eigenpair (round 3) instead of wave_top_eig
    int weights;                // 1: the dual weights / scores are wanted (bootstraps, decomposition); 0: permutations --
                                // only pctvar leaves the solver, the Yd c pass and what hangs on it are skipped
    // global route (GL = true instantiations): no S-long LDS buffer; the scatter to subject space reads these tables
    int* sfirst;                // [nres][S] first included position p with xs_p = i (INT_MAX: subject not drawn)
    int* scnt;                  // [nres][S] number of included positions with xs_p = i
    // cross-validation (plsx_simpls_crossval_batch): a split is a resample with identity sources whose test positions
    // are excluded
    const uint8_t* pmask;       // [nres][S] 1 = position included (training row), or nullptr: every position
                                // (0 = test row; the nested cross-validation also writes 2 = on neither side)
    double* cvZ;                // [nres][k][S] Vd . K: un-centred scores of every row (k_sd_cv_score centres them in place)
    double* cvr;                // [nres][k][T] Pearson r of the nested predictions on the test rows
    double* cvr2;               // [nres][k][T] R^2
    double* cvsse;              // [nres][k + 1][T] squared error summed over the test rows (row 0: intercept only)
    double* cvnte;              // [nres] usable test rows of the fit (k_sd_cv_score<RC, true> only: they depend on the permutation)
    // coefficient series (plsx_simpls_coef_begin): k_sd_coef runs on resamples cf_r0 .. cf_r0 + cf_n - 1 of the batch
    double* cfA;                // [cf_n][T][S] A_b = sum_{j < cf_c} wd_j q_j^T scattered to subject space (every entry written), or nullptr
    double* cfq;                // [cf_n][cf_c][T] q_j = Y0^T t_j (simpls y_loadings of the resample)
    int cf_c, cf_r0, cf_n;
    // VIP stack (plsx_simpls_vip_keep): k_sd_vip runs on every resample of the batch
    double* vpG;                // [nres][vp_c][S] row a = sqrt(ssq_a / (|w_a|^2 sum_j ssq_j)) . wd_a scattered to subject space (every entry written), or nullptr
    int vp_c;
    // confusion counts (plsx_simpls_cv_class_begin): k_sd_cv_class runs after k_sd_cv_score on every fit of the batch
    const int* cls;             // [S] class code 0 .. T - 1 of every row of the bound data
    const double* cfreq;        // [T] class frequencies n_g / S: the column means the bound, globally centred indicators lost
    int* conf;                  // blocks [k][T][T] int32, [c][true][predicted]; fit r adds to block (cls_f0 + r) / cls_n - cls_f0 / cls_n
    long long cls_f0;           // the batch's first fit in the call's pair list (identity route: 0)
    int cls_n;                  // fits per block: the splits of a permutation (identity route: 1)
    // AUC counts (plsx_simpls_cv_auc_begin): k_sd_cv_auc runs after k_sd_cv_score (and k_sd_cv_class) on every fit of the
    // batch; cls / cfreq / cls_f0 / cls_n as above
    long long* auc;             // blocks [k][T][2] int64, [c][class][u2, pairs]; the block of fit r as for conf
};

// doubles of LDS one wave of k_sd_step needs (on-chip route: the last S of them are the scatter buffer)
__host__ __device__ inline size_t sd_step_lds(int S, int T, int k)
{
    return (size_t)T * (T | 1) + 3 * (size_t)T + 2 * (size_t)k + (size_t)S + 8;
}
// ... on the global route: the scatter buffer is gone, T doubles remain (the workspace of wave_top_eig)
__host__ __device__ inline size_t sd_step_lds_global(int T, int k) { return sd_step_lds(T, T, k); }

// Scatter a position-space vector to subject space through the wave's LDS buffer
// (w[i] = sum over included positions p with xs_p = i) and write it to dst[0..S).
// A subject drawn more than once receives bit-identical addends, so the order in which
// the LDS atomics land does not matter.
template <class F>
__device__ __forceinline__ void sd_scatter(double* buf, const int* xs, int S, int lane, double* dst, F value)
{
    for (int i = lane; i < S; i += 64) buf[i] = 0.0;
    wave_sync();
    for (int p = lane; p < S; p += 64) {
        const int x = xs[p];
        if (x >= 0) atomicAdd(&buf[x], value(p));
    }
    wave_sync();
    for (int i = lane; i < S; i += 64) dst[i] = buf[i];
    wave_sync();
}

// The same scatter on the global route (no LDS): subject i takes the value of its first position, added as often as
// the subject was drawn -- the addends of the atomics above, added in the only order identical addends have, so both
// routes write bit-identical vectors.  `first` / `cnt` were built by k_sd_init<true>; value(p) reads positions owned by
// other lanes, so what this wave wrote before must be visible (the caller fences).
template <class F>
__device__ __forceinline__ void sd_scatter_g(const int* first, const int* cnt, int S, int lane, double* dst, F value)
{
    for (int i = lane; i < S; i += 64) {
        const int n = cnt[i];
        double s = 0.0;
        if (n > 0) {
            const double v = value(first[i]);
            for (int m = 0; m < n; ++m) s += v;
        }
        dst[i] = s;
    }
}

// what lanes of this wave stored to global memory is visible to its other lanes
__device__ __forceinline__ void wave_global_sync()
{
    wave_sync();
    __threadfence();
    wave_sync();
}

// Resample setup: sources, masks, Y0 = Jc Y[ys], sum of squares, and the T + 1
// subject-space vectors scatter(Y0[:, t]), cnt for GEMM 0.
// dynamic LDS: S doubles per wave (GL: none -- the scatter tables sfirst / scnt are built here instead, with
// integer atomics: exact in any order).
template <bool GL>
static __global__ __launch_bounds__(256)
void k_sd_init(SdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double sm_sd[];
    const int S = a.S, T = a.T, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: scalar pointers
    const int r = blockIdx.x * (blockDim.x >> 6) + wave;
    if (r >= a.nres) return;
    double* buf = GL ? nullptr : sm_sd + (size_t)wave * S;
    int* xs = a.xs + (size_t)r * S;
    int* ys = a.ys + (size_t)r * S;
    const double* Ysrc = a.Yc + (size_t)r * a.y_stride;
    double* Y0 = a.Y0 + (size_t)r * S * T;
    double cnt = 0.0;
    for (int p = lane; p < S; p += 64) {
        const int x = a.xsrc ? a.xsrc[(size_t)r * S + p] : p;
        const int y = a.ysrc ? a.ysrc[(size_t)r * S + p] : p;
        const int ok = (!a.okx || a.okx[x]) && (!a.oky || a.oky[y]) && (!a.pmask || a.pmask[(size_t)r * S + p] == 1);
        xs[p] = ok ? x : -1;
        ys[p] = y;
        cnt += ok;
    }
    const double ninc = wave_sum(cnt);
    if constexpr (GL) {
        int* first = a.sfirst + (size_t)r * S;
        int* nct = a.scnt + (size_t)r * S;
        for (int i = lane; i < S; i += 64) { first[i] = 0x7fffffff; nct[i] = 0; }
        wave_global_sync();
        for (int p = lane; p < S; p += 64) {
            const int x = xs[p];
            if (x >= 0) { atomicAdd(&nct[x], 1); atomicMin(&first[x], p); }
        }
    }
    double ssy = 0.0;
    for (int t = 0; t < T; ++t) {
        double part = 0.0;
        for (int p = lane; p < S; p += 64) if (xs[p] >= 0) part += Ysrc[(size_t)ys[p] * T + t];
        const double mean = wave_sum(part) / ninc;
        if (lane == 0) a.ymean[(size_t)r * T + t] = mean;
        for (int p = lane; p < S; p += 64) {
            const double y = xs[p] >= 0 ? Ysrc[(size_t)ys[p] * T + t] - mean : 0.0;
            Y0[(size_t)t * S + p] = y;
            ssy += y * y;
        }
    }
    const double ssY = wave_sum(ssy);
    if (lane == 0) { a.scal[(size_t)r * 4] = ninc; a.scal[(size_t)r * 4 + 1] = ssY; }
    // subject-space operands of GEMM 0: vectors 0..T-1 = columns of Y0, vector T = counts
    double* Wt = a.Wt + (size_t)r * (T + 1) * S;
    if constexpr (GL) {
        wave_global_sync();                    // Y0 and the tables, as the other lanes wrote them
        const int* first = a.sfirst + (size_t)r * S;
        const int* nct = a.scnt + (size_t)r * S;
        for (int t = 0; t <= T; ++t)
            sd_scatter_g(first, nct, S, lane, Wt + (size_t)t * S,
                         [&](int p) { return t < T ? Y0[(size_t)t * S + p] : 1.0; });
    } else {
        for (int t = 0; t <= T; ++t)
            sd_scatter(buf, xs, S, lane, Wt + (size_t)t * S,
                       [&](int p) { return t < T ? Y0[(size_t)t * S + p] : 1.0; });
    }
}

// The kernels below are latency chains of ONE wave (a launch lasts as long as its slowest
// wave, and a batch rarely fills every SIMD more than once), so what matters is how many
// independent loads a wave has in flight.  Positions are walked in tiles of 64 x SD_RC: a
// lane owns SD_RC positions of a tile, the loops over them are fully unrolled with clamped
// addresses (no control flow around the loads), and reductions are taken four at a time.
// tools-only phase timing of k_sd_step (compile with -DPLSX_SD_PROBE; never in the product build)
#ifdef PLSX_SD_PROBE
__device__ unsigned long long g_sd_probe[16][32];
#define SD_MARK(n) do { if (r == 0 && lane == 0) g_sd_probe[a.c & 15][n] = __builtin_readcyclecounter(); } while (0)
#else
#define SD_MARK(n) do {} while (0)
#endif

// SD_RC is the template parameter RC of the three kernels below: 16 for batches the chip holds at once (one or two
// waves per SIMD: a wave's own loads in flight are all the latency hiding there is), 8 for larger ones (round 5: three
// waves per SIMD -- what the [S] scatter buffer in LDS allows -- finish 5000 resamples in 2 rounds instead of 3 and
// overlap one wave's eigen-solve with another's passes over S: k_sd_step 0.90 -> 0.83, k_sd_post0 1.41 -> 0.97,
// k_sd_final 2.03 -> 1.11 ms per 5000).  The register budget follows: waves_per_eu(1, 2) / (3, 4).
#define SD_RC RC
#define SD_WPE (RC >= 16 ? 1 : 3), (RC >= 16 ? 2 : 4)
#define SD_TILE (64 * SD_RC)
#define SD_OWN(i) _Pragma("unroll") for (int i = 0; i < SD_RC; ++i)
// positions of the tile at p0 owned by this lane, clamped into [0, S): 32-bit offsets against
// wave-uniform row pointers (scalar base + vector offset addressing, no 64-bit pointer per load)
#define SD_TILE_PC(pc, p0) int pc[SD_RC]; SD_OWN(i_) pc[i_] = min((p0) + lane + 64 * i_, S - 1)
#define SD_IN(p0, i) ((p0) + lane + 64 * (i) < S)

// 8-byte load through a buffer resource: vector byte offset (one 32-bit register per owned
// position, shared by every row) + scalar byte offset (the row).  Keeps the address arithmetic
// of the hot loops on the scalar unit; with plain pointers the compiler strength-reduces every
// (position, array) pair into its own 64-bit induction pointer, runs out of registers and
// ends up waiting for each load before it issues the next.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sd_rsrc(const double* base)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, 0x7fffffff, PLSX_RSRC_FLAGS);
}
__device__ __forceinline__ double sd_ld(__amdgpu_buffer_rsrc_t rs, int voff, int soff)
{
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, 0));
}

__device__ __forceinline__ void wave_sum4(double& a, double& b, double& c, double& d)
{
#define SD_STEP4(CTRL) a += dpp_f64<CTRL>(a); b += dpp_f64<CTRL>(b); c += dpp_f64<CTRL>(c); d += dpp_f64<CTRL>(d);
    SD_STEP4(SD_DPP_XOR1) SD_STEP4(SD_DPP_XOR2) SD_STEP4(SD_DPP_HALF_MIRROR) SD_STEP4(SD_DPP_ROW_MIRROR)
#undef SD_STEP4
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        a += __shfl_xor(a, o); b += __shfl_xor(b, o); c += __shfl_xor(c, o); d += __shfl_xor(d, o);
    }
}

// H = H0 = Y0^T Z0 (T x T; Y0, Z0 T-major [t][p]) of one resample by its wave.
template <int TT>
__device__ __forceinline__ void sd_gram_h(const double* Y0, const double* Z0, int S, int T, int lane, double* H, double* H0)
{
    d4 acc[TT][TT];
#pragma unroll
    for (int i = 0; i < TT; ++i)
#pragma unroll
        for (int j = 0; j < TT; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
    auto rows = [&](const double* M) {
        return [=](int t, int p, double (&v)[4]) {
            const double* src = M + (size_t)min(t, T - 1) * S;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double x = src[min(p + j, S - 1)];
                v[j] = (t < T && p + j < S) ? x : 0.0;
            }
        };
    };
    wave_mfma_nt<TT, TT>(acc, S, lane, rows(Y0), rows(Z0));
#pragma unroll
    for (int mt = 0; mt < TT; ++mt)
#pragma unroll
        for (int nt = 0; nt < TT; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t1 = mt * 16 + (lane >> 4) + 4 * i, t2 = nt * 16 + (lane & 15);
                if (t1 < T && t2 < T) { H[t1 * T + t2] = acc[mt][nt][i]; H0[t1 * T + t2] = acc[mt][nt][i]; }
            }
}

// After GEMM 0: Z0 = Jc gather(K scatter(Y0)), kcpos, H = H0 = Y0^T Z0.
template <int RC, int TC>       // TC as in k_sd_step: the 64 x 64 accumulators of T <= 64 are not allocated for T <= 32
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SD_WPE)))
void k_sd_post0(SdArgs a)
{
    const int S = a.S, T = a.T, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: scalar pointers
    const int r = blockIdx.x * (blockDim.x >> 6) + wave;
    if (r >= a.nres) return;
    const int* xs = a.xs + (size_t)r * S;
    const double* Zt = a.Zt + (size_t)r * (T + 1) * S;
    const double* Y0 = a.Y0 + (size_t)r * S * T;
    double* Z0 = a.Z0 + (size_t)r * S * T;
    const double ninc = a.scal[(size_t)r * 4];
    // column means of the gathered products, four columns at a time
    for (int t0 = 0; t0 <= T; t0 += 4) {
        const double* z0 = Zt + (size_t)min(t0, T) * S;
        const double* z1 = Zt + (size_t)min(t0 + 1, T) * S;
        const double* z2 = Zt + (size_t)min(t0 + 2, T) * S;
        const double* z3 = Zt + (size_t)min(t0 + 3, T) * S;
        double m[4] = {0.0, 0.0, 0.0, 0.0};
        for (int p0 = 0; p0 < S; p0 += SD_TILE) {
            SD_TILE_PC(pc, p0);
            SD_OWN(i) {
                const int x = xs[pc[i]];
                const bool ok = SD_IN(p0, i) && x >= 0;
                const int xc = x >= 0 ? x : 0;
                const double a0 = z0[xc], a1 = z1[xc], a2 = z2[xc], a3 = z3[xc];
                m[0] += ok ? a0 : 0.0; m[1] += ok ? a1 : 0.0; m[2] += ok ? a2 : 0.0; m[3] += ok ? a3 : 0.0;
            }
        }
        wave_sum4(m[0], m[1], m[2], m[3]);
        for (int p0 = 0; p0 < S; p0 += SD_TILE) {
            SD_TILE_PC(pc, p0);
            SD_OWN(i) {
                const int x = xs[pc[i]];
                const int xc = x >= 0 ? x : 0;
                const double zz[4] = {z0[xc], z1[xc], z2[xc], z3[xc]};
                if (SD_IN(p0, i)) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int t = t0 + u;
                        if (t < T) Z0[(size_t)t * S + pc[i]] = x >= 0 ? zz[u] - m[u] / ninc : 0.0;
                        if (t == T) a.kcpos[(size_t)r * S + pc[i]] = x >= 0 ? zz[u] : 0.0;     // un-centred K cnt
                    }
                }
            }
        }
    }
    // H[t1][t2] = sum_p Y0[p][t1] Z0[p][t2] on the matrix pipe (Z0 as this wave just wrote it: same lanes' stores are
    // visible to the wave after the fence)
    double* H = a.H + (size_t)r * T * T;
    double* H0 = a.H0 + (size_t)r * T * T;
    wave_sync();
    __threadfence_block();
    if (TC == 0 && T <= 16) sd_gram_h<1>(Y0, Z0, S, T, lane, H, H0);
    else if (TC == 0 && T <= 32) sd_gram_h<2>(Y0, Z0, S, T, lane, H, H0);
    else if (TC == 1 && T <= 48) sd_gram_h<3>(Y0, Z0, S, T, lane, H, H0);
    else if (TC == 1 && T <= 64) sd_gram_h<4>(Y0, Z0, S, T, lane, H, H0);
    else {
        for (int t1 = 0; t1 < T; ++t1)
            for (int t2 = 0; t2 < T; t2 += 4) {
                const double* y1 = Y0 + (size_t)t1 * S;
                const double* z0 = Z0 + (size_t)min(t2, T - 1) * S;
                const double* z1 = Z0 + (size_t)min(t2 + 1, T - 1) * S;
                const double* z2 = Z0 + (size_t)min(t2 + 2, T - 1) * S;
                const double* z3 = Z0 + (size_t)min(t2 + 3, T - 1) * S;
                double s4[4] = {0.0, 0.0, 0.0, 0.0};
                for (int p0 = 0; p0 < S; p0 += SD_TILE) {
                    SD_TILE_PC(pc, p0);
                    SD_OWN(i) {
                        const double yv = y1[pc[i]], y = SD_IN(p0, i) ? yv : 0.0;
                        s4[0] += y * z0[pc[i]]; s4[1] += y * z1[pc[i]]; s4[2] += y * z2[pc[i]]; s4[3] += y * z3[pc[i]];
                    }
                }
                wave_sum4(s4[0], s4[1], s4[2], s4[3]);
                if (lane == 0)
                    for (int u = 0; u < 4 && t2 + u < T; ++u) { H[t1 * T + t2 + u] = s4[u]; H0[t1 * T + t2 + u] = s4[u]; }
            }
    }
}

// One-sided Jacobi on the columns of A (m x n, column pitch ld, in the wave's LDS) by ONE
// wavefront: 4 lanes per column pair, 16 disjoint pairs of a round-robin step at a time.  At
// convergence column j holds lambda_j v_j for a symmetric PSD input.  Same pairing, threshold
// and null-pair rule as jacobi_cols (the block-level solver of the PLS-C path).  A step is a
// pure latency chain (152 of them for T = 20: the longest phase of k_sd_step), so: both
// columns of a pair are fetched into registers up front (IT rows per lane), the group sums are
// two DPP butterflies, and the rotation comes from two reciprocal square roots instead of
// three divisions and three square roots:
//     d = beta - alpha, g = 2 gamma, h = hypot(d, g):  cos 2t = |d| / h,
//     c = sqrt((1 + |d| / h) / 2),  s = sign(d g) |g| / (2 h c)
// -- the same inner rotation (|t| <= pi/4) as t = sign(z) / (|z| + sqrt(1 + z^2)), z = d / g.
template <int IT>
__device__ __forceinline__ void wave_jacobi_cols(double* A, int m, int n, int ld, int lane, double tol)
{
    constexpr int LANES = 4;
    const int sub = lane % LANES, grp = lane / LANES, ngrp = 64 / LANES;
    const int np = (n + 1) >> 1, ne = np * 2, mod = ne - 1;
    double mx = 0.0;
    for (int c = lane; c < n; c += 64) {
        double s = 0.0;
        for (int i = 0; i < m; ++i) { const double x = A[(size_t)c * ld + i]; s += x * x; }
        mx = fmax(mx, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    const double null2 = 1e-26 * mx, tol2 = tol * tol;
    int ri[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) ri[i] = min(sub + LANES * i, m - 1);
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int step = 0; step < mod; ++step) {
            for (int pr0 = 0; pr0 < np; pr0 += ngrp) {
                const int pr = pr0 + grp;
                int p = 0, q = n;                                   // q >= n: this group sits the pass out
                if (pr < np) {
                    if (pr == 0) { p = step; q = ne - 1; }
                    else {
                        p = step + pr; if (p >= mod) p -= mod;
                        q = step + mod - pr; if (q >= mod) q -= mod;
                    }
                    if (p > q) { const int t = p; p = q; q = t; }
                }
                const bool act = q < n;
                double* ap = A + (size_t)(act ? p : 0) * ld;
                double* aq = A + (size_t)(act ? q : 0) * ld;
                double x[IT], y[IT];
#pragma unroll
                for (int i = 0; i < IT; ++i) { x[i] = ap[ri[i]]; y[i] = aq[ri[i]]; }
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
                for (int i = 0; i < IT; ++i) {
                    const bool in = act && sub + LANES * i < m;
                    const double xx = in ? x[i] : 0.0, yy = in ? y[i] : 0.0;
                    alpha += xx * xx; beta += yy * yy; gamma += xx * yy;
                }
#if defined(PLSX_JV) && PLSX_JV == 1                   // (probe variants: tools/jacobi16_probe.sh)
                alpha += __shfl_xor(alpha, 1); beta += __shfl_xor(beta, 1); gamma += __shfl_xor(gamma, 1);
                alpha += __shfl_xor(alpha, 2); beta += __shfl_xor(beta, 2); gamma += __shfl_xor(gamma, 2);
#else
                alpha += dpp_f64<SD_DPP_XOR1>(alpha); beta += dpp_f64<SD_DPP_XOR1>(beta); gamma += dpp_f64<SD_DPP_XOR1>(gamma);
                alpha += dpp_f64<SD_DPP_XOR2>(alpha); beta += dpp_f64<SD_DPP_XOR2>(beta); gamma += dpp_f64<SD_DPP_XOR2>(gamma);
#endif
                const bool rot = act && gamma != 0.0 && gamma * gamma > tol2 * (alpha * beta) &&
                                 !(alpha < null2 && beta < null2);
                if (rot) {
                    const double d = beta - alpha, g = 2.0 * gamma;
                    const double rh = sd_rsqrt(__builtin_fma(d, d, g * g));          // 1 / hypot(d, g)
                    const double c2 = __builtin_fma(0.5 * fabs(d), rh, 0.5);          // cos^2 t, in [1/2, 1]
                    const double rc = sd_rsqrt(c2);
                    const double c = c2 * rc;
                    const double sn = copysign(0.5 * fabs(g) * rh * rc, d >= 0.0 ? g : -g);
#pragma unroll
                    for (int i = 0; i < IT; ++i)
                        if (sub + LANES * i < m) {
                            ap[ri[i]] = c * x[i] - sn * y[i];
                            aq[ri[i]] = sn * x[i] + c * y[i];
                        }
                    rotated = true;
                }
#if defined(PLSX_JV) && PLSX_JV == 3
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
                wave_sync();
            }
        }
        if (!__any(rotated)) break;
    }
}

// Leading eigenpair of a symmetric PSD matrix by ONE wavefront without Jacobi sweeps (round 4): SIMPLS needs
// only the top eigenpair of the T x T matrix H per component (pyls/types/regression.py:106-112 takes the leading
// singular triplet of the cross-covariance), and the full one-sided Jacobi solve was the longest phase of
// k_sd_step (152 dependent pair-steps per sweep at T = 20, ~8 sweeps: 0.16 ms of a 0.38 ms launch).
//   1. Householder reduction to tridiagonal form, in place (A: n x n, A[c * ld + r], both triangles stored):
//      for k = 0 .. n-3 the unit reflector v_k (rows k+1 ..) annihilates column k below the subdiagonal,
//      A22 <- A22 - 2 v w^T - 2 w v^T with p = A22 v, w = p - (v.p) v; lanes own rows, v_k stays in column k.
//   2. Largest eigenvalue of the tridiagonal (d, e) by MULTIsection: every lane evaluates the Sturm count
//      (number of eigenvalues below its abscissa) at one of 64 points of the bracket, a ballot finds the
//      sub-interval: 65 x narrower per round, 9 rounds from the Gershgorin bracket to eps (robust for
//      clustered eigenvalues -- permuted data has closely spaced singular values).
//   3. Its eigenvector by inverse iteration on the tridiagonal (LU with partial pivoting as LAPACK's dlagtf /
//      dlagts, three iterations from a flat start vector; one lane, n-step recurrences).
//   4. Back-transformation y <- H_0 H_1 ... H_{n-3} y.
// n <= 64.  Measured with the s_memtime probes at c5 (T = 20): see DESIGN.md.  ws: n doubles of the wave's LDS.
// Returns lambda_max; vec[0..n)
// = unit eigenvector (sign arbitrary, as with Jacobi: SIMPLS is invariant to it, the front-end's sign rule
// and the bootstrap's sign alignment act on the weights).
// Value of lane `i` (wave-uniform, runtime) of a per-lane double: two v_readlane_b32 -- a few cycles, where a
// broadcast through the wave's LDS costs a ~64-cycle round trip on every link of a serial recurrence.
__device__ __forceinline__ double lane_get(double v, int i)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), i);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), i);
    return __hiloint2double(hi, lo);
}

__device__ double wave_top_eig(double* A, int n, int ld, int lane, double* ws, double* vec)
{
    // n <= 64: the vectors of the tridiagonal stage live one element per lane (d, e, the LU factors, the iterate);
    // serial recurrences read them with lane_get.
    double* pw = ws;             // [n] p / w of the reflector step (LDS)
    if (n == 1) {
        if (lane == 0) vec[0] = 1.0;
        wave_sync();
        return A[0];
    }
    double dl = 0.0, el = 0.0;   // d[lane], e[lane] (e[i] couples rows i and i + 1)
    for (int k = 0; k + 2 < n; ++k) {
        double s2 = 0.0;
        for (int i = k + 2 + lane; i < n; i += 64) { const double x = A[(size_t)k * ld + i]; s2 += x * x; }
        s2 = wave_sum(s2);
        const double x0 = A[(size_t)k * ld + k + 1];
        const double dk = A[(size_t)k * ld + k];
        if (lane == k) dl = dk;
        if (!(s2 > 0.0)) {                                 // already tridiagonal in this column: H_k = I
            if (lane == k) el = x0;
            wave_sync();
            if (lane == 0) A[(size_t)k * ld + k + 1] = 0.0;
            wave_sync();
            continue;
        }
        const double alpha = -copysign(sqrt(__builtin_fma(x0, x0, s2)), x0);
        if (lane == k) el = alpha;
        const double v0 = x0 - alpha;
        const double inv = 1.0 / sqrt(__builtin_fma(v0, v0, s2));
        wave_sync();
        for (int i = k + 1 + lane; i < n; i += 64)
            A[(size_t)k * ld + i] = (i == k + 1 ? v0 : A[(size_t)k * ld + i]) * inv;
        wave_sync();
        const double* v = A + (size_t)k * ld;             // v[i], i = k + 1 .. n - 1
        // p = A22 v, rows lane-strided; operands of eight columns are fetched before they are used (independent
        // LDS reads in flight instead of one round trip per column)
        const int i = k + 1 + lane;                        // (n <= 64: one row per lane)
        const int ic = min(i, n - 1);
        double pi = 0.0;
        for (int j0 = k + 1; j0 < n; j0 += 8) {
            double av[8], vv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int j = min(j0 + u, n - 1); av[u] = A[(size_t)j * ld + ic]; vv[u] = v[j]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) pi = __builtin_fma(av[u], (j0 + u < n) ? vv[u] : 0.0, pi);
        }
        const double vi = i < n ? v[ic] : 0.0;
        const double K = wave_sum(i < n ? vi * pi : 0.0);
        const double wi = __builtin_fma(-K, vi, pi);      // w = p - K v
        if (i < n) pw[i] = wi;
        wave_sync();
        for (int j0 = k + 1; j0 < n; j0 += 8) {
            double av[8], vv[8], ww[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = min(j0 + u, n - 1);
                av[u] = A[(size_t)j * ld + ic]; vv[u] = v[j]; ww[u] = pw[j];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const double t = __builtin_fma(vi, ww[u], wi * vv[u]);
                av[u] = __builtin_fma(-2.0, t, av[u]);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (i < n && j0 + u < n) A[(size_t)(j0 + u) * ld + i] = av[u];
        }
        wave_sync();
    }
    {
        const double a = A[(size_t)(n - 2) * ld + n - 2], b = A[(size_t)(n - 2) * ld + n - 1], c = A[(size_t)(n - 1) * ld + n - 1];
        if (lane == n - 2) { dl = a; el = b; }
        if (lane == n - 1) { dl = c; el = 0.0; }
    }
    // ---- lambda_max by multisection on the Sturm count
    double hi = -1e300, lo = -1e300, emax = 0.0;
    {
        const double eup = __shfl_up(el, 1);               // (unconditionally: every source lane must be active)
        const double em = lane > 0 ? fabs(eup) : 0.0, ep = lane + 1 < n ? fabs(el) : 0.0;
        double g = lane < n ? dl + em + ep : -1e300, dd = lane < n ? dl : -1e300, ee = lane < n ? ep : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            g = fmax(g, __shfl_xor(g, o)); dd = fmax(dd, __shfl_xor(dd, o)); ee = fmax(ee, __shfl_xor(ee, o));
        }
        hi = g; lo = dd; emax = ee;                          // lambda_max >= every diagonal entry
    }
    const double pivmin = 2.2250738585072014e-308 * fmax(1.0, emax * emax);
    const double span0 = fmax(fabs(hi), fabs(lo));
    lo -= 4.0 * 2.220446049250313e-16 * span0 + pivmin;
    hi += 4.0 * 2.220446049250313e-16 * span0 + pivmin;
    const double e2l = el * el;
    for (int round = 0; round < 14; ++round) {
        const double x = lo + (hi - lo) * ((double)(lane + 1) * (1.0 / 65.0));
        // Sturm count without divisions: the sign changes of the leading principal minors p_i of (T - x I),
        // p_i = (d_i - x) p_{i-1} - e_{i-1}^2 p_{i-2}, equal the number of eigenvalues below x (a zero minor takes
        // the sign opposite to its predecessor, as the pivot rule q = -pivmin of the quotient form does); the
        // pair (p_{i-1}, p_i) is rescaled by a power of two when it leaves [2^-200, 2^200].  d_i, e_{i-1}^2 come
        // from lane i / i - 1 by readlane: two dependent FMAs per row is what a round costs.
        double pm = 1.0, pc = lane_get(dl, 0) - x;
        bool nprev = pc < 0.0 || pc == 0.0;                // sign assigned to the latest minor (p_0 = 1 is positive)
        int cnt = nprev;
        for (int i = 1; i < n; ++i) {
            const double di = lane_get(dl, i), e2 = lane_get(e2l, i - 1);
            const double pn = __builtin_fma(di - x, pc, -e2 * pm);
            const bool nnew = pn < 0.0 || (pn == 0.0 && !nprev);
            cnt += nnew != nprev;
            nprev = nnew;
            pm = pc; pc = pn;
            const double mag = fmax(fabs(pm), fabs(pc));
            if (mag > 0x1p200) { pm *= 0x1p-200; pc *= 0x1p-200; }
            else if (mag < 0x1p-200 && mag > 0.0) { pm *= 0x1p200; pc *= 0x1p200; }
        }
        const unsigned long long above = __ballot(cnt >= n);          // abscissas above every eigenvalue
        const int jf = above ? __builtin_ctzll(above) : 64;
        const double span = hi - lo;
        const double nlo = jf > 0 ? lo + span * ((double)jf * (1.0 / 65.0)) : lo;
        const double nhi = jf < 64 ? lo + span * ((double)(jf + 1) * (1.0 / 65.0)) : hi;
        lo = nlo; hi = nhi;
        if (hi - lo <= 2.0 * 2.220446049250313e-16 * fmax(fabs(lo), fabs(hi)) + 2.0 * pivmin) break;
    }
    const double lam = 0.5 * (lo + hi);
    // ---- eigenvector of the tridiagonal: LU with partial pivoting of (T - lam I) (as LAPACK's dlagtf / dlagts),
    // ---- three inverse iterations.  Element i of every vector lives in lane i; each step of the recurrences is
    // ---- computed by every lane from readlane values (wave-uniform) and kept by the lane that owns it.
    double la = dl - lam;                                  // diagonal of U
    double lb = lane + 1 < n ? el : 0.0;                   // first superdiagonal of U
    double lc = 0.0, l2 = 0.0;                             // multipliers, second superdiagonal (fill-in of row swaps)
    bool sw = false;
    {
        const double eup = __shfl_up(el, 1);
        double tn = fabs(la) + (lane > 0 ? fabs(eup) : 0.0) + (lane + 1 < n ? fabs(el) : 0.0);
        if (lane >= n) tn = 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tn = fmax(tn, __shfl_xor(tn, o));
        const double tiny = fmax(2.220446049250313e-16 * tn, pivmin);
        for (int i = 0; i + 1 < n; ++i) {
            const double sub = lane_get(el, i);                // entry (i + 1, i) before elimination
            const double ai = lane_get(la, i), bi = lane_get(lb, i);
            const double a1 = lane_get(la, i + 1), b1 = lane_get(lb, i + 1);
            if (fabs(ai) >= fabs(sub)) {
                double piv = ai;
                if (fabs(piv) < tiny) piv = copysign(tiny, piv == 0.0 ? 1.0 : piv);
                const double m = sub / piv;
                if (lane == i) { la = piv; lc = m; }
                if (lane == i + 1) la = a1 - m * bi;
            } else {                                           // swap rows i and i + 1
                const double m = ai / sub;
                if (lane == i) { lc = m; sw = true; la = sub; lb = a1; l2 = b1; }
                if (lane == i + 1) { la = bi - m * a1; lb = -m * b1; }
            }
        }
        const double an = lane_get(la, n - 1);
        if (lane == n - 1 && fabs(an) < tiny) la = copysign(tiny, an == 0.0 ? 1.0 : an);
    }
    double y = lane < n ? ((lane & 1) ? 0.9 : 1.1) : 0.0;
    const unsigned long long swm = __ballot(sw);
    for (int it = 0; it < 3; ++it) {
        for (int i = 0; i + 1 < n; ++i) {                   // forward: the same row operations on the right-hand side
            const double yi = lane_get(y, i), y1 = lane_get(y, i + 1), m = lane_get(lc, i);
            if ((swm >> i) & 1) {
                if (lane == i) y = y1;
                if (lane == i + 1) y = yi - m * y1;
            } else if (lane == i + 1) y = y1 - m * yi;
        }
        for (int i = n - 1; i >= 0; --i) {                  // back substitution with (la, lb, l2)
            double t = lane_get(y, i);
            if (i + 1 < n) t -= lane_get(lb, i) * lane_get(y, i + 1);
            if (i + 2 < n) t -= lane_get(l2, i) * lane_get(y, i + 2);
            t /= lane_get(la, i);
            if (lane == i) y = t;
        }
        double nr = lane < n ? fabs(y) : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nr = fmax(nr, __shfl_xor(nr, o));
        y *= 1.0 / nr;
    }
    y *= 1.0 / sqrt(wave_sum(lane < n ? y * y : 0.0));
    // ---- back-transformation: y <- H_k y for k = n - 3 .. 0 (lane i holds y_i and reads v_k[i] from column k)
    for (int k = n - 3; k >= 0; --k) {
        const double vk = (lane > k && lane < n) ? A[(size_t)k * ld + lane] : 0.0;
        const double dp = wave_sum(vk * y);
        y = __builtin_fma(-2.0 * dp, vk, y);
    }
    if (lane < n) vec[lane] = y;
    wave_sync();
    return lam;
}

// Component step c (see the header): closes component c - 1 when c > 0, opens component c
// unless c == k.  dynamic LDS: sd_step_lds(S, T, k) doubles per wave (GL: sd_step_lds_global(T, k) -- the scatter of
// the new basis vector goes through sd_scatter_g).
// TC: class of T the instantiation serves (0: T <= 32, 1: T <= 64, 2: any) -- the register allocation of a kernel is
// the maximum over its paths, and the Jacobi fall-back for large T (36 rows of two columns per lane) would otherwise
// set it for every T.  JAC: the leading eigenpair by the full one-sided Jacobi solve (T > 64, T > S, or the
// `simpls_jacobi` option) instead of wave_top_eig.
template <int TC, bool JAC, int RC, bool GL = false>
#if defined(PLSX_JV) && PLSX_JV == 8                    // (probe: the attribute of the build in which <16> was first seen wrong)
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RC >= 16 ? 1 : 3, RC >= 16 ? 2 : 4)))
#else
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((JAC || RC >= 16) ? 1 : 3, JAC ? 1 : (RC >= 16 ? 2 : 4))))
#endif
void k_sd_step(SdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double sm_sd[];
    const int S = a.S, T = a.T, k = a.k, c = a.c, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: scalar pointers
    const int r = blockIdx.x * (blockDim.x >> 6) + wave;
    if (r >= a.nres) return;
    const int ldh = T | 1;
    double* Hw = sm_sd + (size_t)wave * (GL ? sd_step_lds_global(T, k) : sd_step_lds(S, T, k));   // [T][ldh] Jacobi work copy of H
    double* cv = Hw + (size_t)T * ldh;         // [T]
    double* gv = cv + T;                       // [T]
    double* gn = gv + T;                       // [T] new row of G
    double* gc = gn + T;                       // [k]
    double* mj = gc + k;                       // [k]
    double* buf = mj + k;                      // [S] scatter buffer (GL: [T], the eigen-solver's workspace only)
    const int* xs = a.xs + (size_t)r * S;
    const double* Y0 = a.Y0 + (size_t)r * S * T;
    const double* Z0 = a.Z0 + (size_t)r * S * T;
    double* BT = a.BT + (size_t)r * k * S;
    double* KB = a.KB + (size_t)r * k * S;
    double* va = a.va + (size_t)r * S;
    const double* kcpos = a.kcpos + (size_t)r * S;
    // H, G, gY0 stay in global memory: every entry is only ever touched by the lane that owns
    // its index (idx = lane + 64 i for H, t = lane + 64 i for the rows of G / gY0), in this
    // launch and in the earlier ones, so no value crosses lanes through global memory
    double* H = a.H + (size_t)r * T * T;
    const double* H0 = a.H0 + (size_t)r * T * T;
    double* G = a.G + (size_t)r * k * T;
    double* gY0 = a.gY0 + (size_t)r * k * T;
    const double ninc = a.scal[(size_t)r * 4], ssY = a.scal[(size_t)r * 4 + 1];
    const int* ys = a.ys + (size_t)r * S;
    const double* Ysrc = a.Yc + (size_t)r * a.y_stride;
    const double* ym = a.ymean + (size_t)r * T;

    SD_MARK(0);
    if (c > 0) {
        // ---- close component cc = c - 1 (after GEMM cc): K beta gathered and centred, the new
        // ---- basis pair, deflation coefficients g = (K beta)^T Yd, H -= g g^T
        const int cc = c - 1;
        const double* Zt = a.Zt + (size_t)r * S;
        double* btc = BT + (size_t)cc * S;
        double* kbc = KB + (size_t)cc * S;
        // Zt gathered through xs (a dependent load): the indices of a tile first, then the values
        double zs = 0.0;
        for (int p0 = 0; p0 < S; p0 += SD_TILE) {
            SD_TILE_PC(pc, p0);
            int xv[SD_RC];
            SD_OWN(i) xv[i] = xs[pc[i]];
            double zv[SD_RC];
            SD_OWN(i) zv[i] = Zt[max(xv[i], 0)];
            SD_OWN(i) zs += (SD_IN(p0, i) && xv[i] >= 0) ? zv[i] : 0.0;
        }
        const double zmean = wave_sum(zs) / ninc;
        double part = 0.0;
        for (int p0 = 0; p0 < S; p0 += SD_TILE) {
            SD_TILE_PC(pc, p0);
            int xv[SD_RC];
            double vv[SD_RC], zv[SD_RC];
            SD_OWN(i) { xv[i] = xs[pc[i]]; vv[i] = va[pc[i]]; }
            SD_OWN(i) zv[i] = Zt[max(xv[i], 0)];
            SD_OWN(i) part += (SD_IN(p0, i) && xv[i] >= 0) ? vv[i] * (zv[i] - zmean) : 0.0;
        }
        const double nrm = sqrt(wave_sum(part));
        for (int p0 = 0; p0 < S; p0 += SD_TILE) {
            SD_TILE_PC(pc, p0);
            int xv[SD_RC];
            double vv[SD_RC], zv[SD_RC];
            SD_OWN(i) { xv[i] = xs[pc[i]]; vv[i] = va[pc[i]]; }
            SD_OWN(i) zv[i] = Zt[max(xv[i], 0)];
            SD_OWN(i) { vv[i] = vv[i] / nrm; zv[i] = xv[i] >= 0 ? (zv[i] - zmean) / nrm : 0.0; }
            SD_OWN(i) if (SD_IN(p0, i)) { btc[pc[i]] = vv[i]; kbc[pc[i]] = zv[i]; }
        }
        SD_MARK(1);
        // gY0_cc[t] = sum_p KB_cc[p] Y0[p][t];  m_j = KB_cc . BT_j.  Y0[p][t] = Y[ys_p][t] - ymean[t] on the included
        // positions and KB is zero on the others, so the sum is taken over ROWS of the shared Y (S x T, row-major: 8 T
        // contiguous bytes per position, resident in L2 for every resample of the launch) instead of streaming the
        // resample's own copy of Y0 from HBM: sum_p KB[p] Y[ys_p][t] - ymean[t] sum_p KB[p]
        {
            double ksum = 0.0;
            for (int t0 = 0; t0 < T; t0 += 8) {
                double g8[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (int p0 = 0; p0 < S; p0 += SD_TILE) {
                    SD_TILE_PC(pc, p0);
                    SD_OWN(i) {
                        const double kv = kbc[pc[i]], kb = SD_IN(p0, i) ? kv : 0.0;
                        const double* yr = Ysrc + (size_t)ys[pc[i]] * T + t0;
                        if (t0 == 0) ksum += kb;
#pragma unroll
                        for (int u = 0; u < 8; ++u) g8[u] += kb * yr[min(u, T - 1 - t0)];
                    }
                }
                wave_sum4(g8[0], g8[1], g8[2], g8[3]);
                wave_sum4(g8[4], g8[5], g8[6], g8[7]);
                if (t0 == 0) ksum = wave_sum(ksum);
                if (lane == 0)
                    for (int u = 0; u < 8 && t0 + u < T; ++u) gv[t0 + u] = g8[u] - ym[t0 + u] * ksum;
            }
        }
        for (int j0 = 0; j0 < cc; j0 += 4) {
            const double* b0 = BT + (size_t)min(j0, cc - 1) * S;
            const double* b1 = BT + (size_t)min(j0 + 1, cc - 1) * S;
            const double* b2 = BT + (size_t)min(j0 + 2, cc - 1) * S;
            const double* b3 = BT + (size_t)min(j0 + 3, cc - 1) * S;
            double s4[4] = {0.0, 0.0, 0.0, 0.0};
            for (int p0 = 0; p0 < S; p0 += SD_TILE) {
                SD_TILE_PC(pc, p0);
                SD_OWN(i) {
                    const double kv = kbc[pc[i]], kb = SD_IN(p0, i) ? kv : 0.0;
                    s4[0] += kb * b0[pc[i]]; s4[1] += kb * b1[pc[i]]; s4[2] += kb * b2[pc[i]]; s4[3] += kb * b3[pc[i]];
                }
            }
            wave_sum4(s4[0], s4[1], s4[2], s4[3]);
            if (lane == 0)
                for (int u = 0; u < 4 && j0 + u < cc; ++u) mj[j0 + u] = s4[u];
        }
        SD_MARK(2);
        wave_sync();
        for (int t = lane; t < T; t += 64) {
            double g = gv[t];
            for (int j = 0; j < cc; ++j) g -= mj[j] * G[(size_t)j * T + t];
            gn[t] = g;
            G[(size_t)cc * T + t] = g;
            gY0[(size_t)cc * T + t] = gv[t];
        }
        wave_sync();
        for (int idx = lane; idx < T * T; idx += 64) {
            const int t1 = idx / T, t2 = idx - t1 * T;
            H[idx] -= gn[t1] * gn[t2];
        }
    }
    SD_MARK(3);
    if (c >= k) return;

    // ---- open component c: leading eigenpair of H (symmetric PSD) by one-sided Jacobi on a
    // ---- copy.  The rotations need not be accumulated: at convergence column j of the copy is
    // ---- H v_j = lambda_j v_j, so the eigenvector is that column normalised.
    for (int idx = lane; idx < T * T; idx += 64) Hw[(idx % T) * ldh + idx / T] = H[idx];
    wave_sync();
    SD_MARK(4);
    double lam;
    if constexpr (!JAC) {
        // the leading eigenpair alone (Householder + multisection + inverse iteration); the [S] scatter buffer,
        // idle until the end of the launch, is its workspace
        lam = wave_top_eig(Hw, T, ldh, lane, buf, cv);
        SD_MARK(5);
        for (int t = lane; t < T; t += 64) a.cvec[((size_t)r * T + t) * k + c] = cv[t];
    } else {
        // rows per lane of a column (4 lanes per pair): 8 covers T <= 32, 16 covers T <= 64, 36 the LDS limit of T.
        // The 16-row variant is back (round 6): round 5 had seen it return a wrong leading vector at T = 44 / 56 > S and
        // removed it "not understood"; at HEAD -- the solver source is byte-identical to that commit but for this line --
        // it does not: tools/jacobi16_probe.{sh,py} ran it under seven code-generation variants (as it was, __shfl_xor
        // instead of the DPP butterflies, an explicit lgkmcnt(0) before wave_sync, -O1, 20 rows per lane, the
        // amdgpu_waves_per_eu(1, 2) attribute of the build it was first seen wrong in) on the failing shapes, rank
        // deficient and full rank, original fit and the whole front-end call: every variant is right to 1e-14 and
        // BIT-IDENTICAL to the 36-row instantiation -- as it must be: a masked row adds an exact zero to alpha / beta /
        // gamma, so the instantiations execute the same arithmetic in the same order ("c5 solver").
        if constexpr (TC == 0) wave_jacobi_cols<8>(Hw, T, T, ldh, lane, 1e-15);
#if defined(PLSX_JV) && PLSX_JV == 5                    // (probe variants: tools/jacobi16_probe.sh)
        else if constexpr (TC == 1) wave_jacobi_cols<20>(Hw, T, T, ldh, lane, 1e-15);
#elif defined(PLSX_JV) && PLSX_JV == 7
        else if constexpr (TC == 1) wave_jacobi_cols<36>(Hw, T, T, ldh, lane, 1e-15);
#else
        else if constexpr (TC == 1) wave_jacobi_cols<16>(Hw, T, T, ldh, lane, 1e-15);
#endif
        else wave_jacobi_cols<36>(Hw, T, T, ldh, lane, 1e-15);
        SD_MARK(5);
        for (int col = lane; col < T; col += 64) {
            double s = 0.0;
            for (int i = 0; i < T; ++i) { const double x = Hw[col * ldh + i]; s += x * x; }
            gv[col] = sqrt(s);
        }
        wave_sync();
        int best = 0;
        for (int col = 1; col < T; ++col) if (gv[col] > gv[best]) best = col;
        lam = gv[best];
        for (int t = lane; t < T; t += 64) {
            cv[t] = Hw[best * ldh + t] / lam;
            a.cvec[((size_t)r * T + t) * k + c] = cv[t];
        }
    }
    const double si = sqrt(lam);
    wave_sync();
    for (int j0 = 0; j0 < c; j0 += 4) {        // gc_j = g_j . c, lanes over t (each reads its own entries of G)
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int t = lane; t < T; t += 64) {
            const double cvt = cv[t];
#pragma unroll
            for (int u = 0; u < 4; ++u) s4[u] += G[(size_t)min(j0 + u, c - 1) * T + t] * cvt;
        }
        wave_sum4(s4[0], s4[1], s4[2], s4[3]);
        if (lane == 0)
            for (int u = 0; u < 4 && j0 + u < c; ++u) gc[j0 + u] = s4[u];
    }
    wave_sync();
    SD_MARK(6);
    // a = Yd c / s, t = Z c / s in factored form.  Every lane keeps the entries of its own
    // positions: XW row c doubles as the work vector t, WD row c as a, `va` as beta.
    double* vt = a.XW + ((size_t)r * k + c) * S;
    double* wd = a.WD + ((size_t)r * k + c) * S;
    double n2 = 0.0, asum = 0.0;
    const __amdgpu_buffer_rsrc_t rsY = sd_rsrc(Y0), rsZ = sd_rsrc(Z0), rsB = sd_rsrc(BT), rsK = sd_rsrc(KB);
    const int rowb = S * 8;
    const bool wts = a.weights != 0;
    double ymcv = 0.0;                         // ymean . c (every lane: T reads of the wave's LDS / its own means)
    for (int t = 0; t < T; ++t) ymcv += ym[t] * cv[t];
    for (int p0 = 0; p0 < S; p0 += SD_TILE) {
        SD_TILE_PC(pc, p0);
        int vo[SD_RC];
        SD_OWN(i) vo[i] = pc[i] * 8;
        double ya[SD_RC], za[SD_RC];
        SD_OWN(i) { ya[i] = 0.0; za[i] = 0.0; }
        if (wts) {
            // Yd c: rows of the shared Y again (see the closing half), Z c: the resample's own Z0, T-major
            int yo[SD_RC];
            SD_OWN(i) yo[i] = ys[pc[i]] * T;
            for (int t = 0; t < T; ++t) {
                const double cvt = cv[t];
                const int so = t * rowb;
                double yv[SD_RC], zv[SD_RC];
                SD_OWN(i) { yv[i] = Ysrc[(size_t)yo[i] + t]; zv[i] = sd_ld(rsZ, vo[i], so); }
                SD_OWN(i) { ya[i] += yv[i] * cvt; za[i] += zv[i] * cvt; }
            }
            {
                int xq[SD_RC];
                SD_OWN(i) xq[i] = xs[pc[i]];
                SD_OWN(i) ya[i] = xq[i] >= 0 ? ya[i] - ymcv : 0.0;
            }
            for (int j = 0; j < c; ++j) {
                const double g = gc[j];
                const int so = j * rowb;
                double bv[SD_RC], kv[SD_RC];
                SD_OWN(i) { bv[i] = sd_ld(rsB, vo[i], so); kv[i] = sd_ld(rsK, vo[i], so); }
                SD_OWN(i) { ya[i] -= bv[i] * g; za[i] -= kv[i] * g; }
            }
        } else {
            // permutations: t = Z c / s alone (a = Yd c / s only feeds the weights and the scores)
            for (int t = 0; t < T; ++t) {
                const double cvt = cv[t];
                const int so = t * rowb;
                double zv[SD_RC];
                SD_OWN(i) zv[i] = sd_ld(rsZ, vo[i], so);
                SD_OWN(i) za[i] += zv[i] * cvt;
            }
            for (int j = 0; j < c; ++j) {
                const double g = gc[j];
                const int so = j * rowb;
                double kv[SD_RC];
                SD_OWN(i) kv[i] = sd_ld(rsK, vo[i], so);
                SD_OWN(i) za[i] -= kv[i] * g;
            }
        }
        int xv[SD_RC];
        SD_OWN(i) xv[i] = xs[pc[i]];
        SD_OWN(i) {
            ya[i] /= si; za[i] /= si;
            if (SD_IN(p0, i)) {
                n2 += za[i] * za[i];
                if (xv[i] >= 0) asum += ya[i];
            }
        }
        if (wts) { SD_OWN(i) if (SD_IN(p0, i)) wd[pc[i]] = ya[i]; }
        SD_OWN(i) if (SD_IN(p0, i)) vt[pc[i]] = za[i];
    }
    SD_MARK(7);
    const double normt = sqrt(wave_sum(n2));
    const double amean = wave_sum(asum) / ninc;
    double mu = 0.0;
    for (int p0 = 0; wts && p0 < S; p0 += SD_TILE) {
        SD_TILE_PC(pc, p0);
        double an[SD_RC];
        SD_OWN(i) {
            const int x = xs[pc[i]];
            const double w = wd[pc[i]], kc = kcpos[pc[i]];
            const double ac = (SD_IN(p0, i) && x >= 0) ? w - amean : 0.0;
            an[i] = ac / normt;
            mu += ac * kc;
        }
        SD_OWN(i) if (SD_IN(p0, i)) wd[pc[i]] = an[i];
    }
    mu = wave_sum(mu) / ninc;                  // mean over positions of the un-centred product X[xs] r
    // y_loadings q = Y0^T t = (H0 c - sum_j gY0_j gc_j) / (s |t|)  -> pctvar
    double q2 = 0.0;
    for (int t = lane; t < T; t += 64) {
        double s = 0.0;
        for (int u = 0; u < T; ++u) s += H0[(size_t)t * T + u] * cv[u];
        for (int j = 0; j < c; ++j) s -= gY0[(size_t)j * T + t] * gc[j];
        s /= si * normt;
        q2 += s * s;
    }
    q2 = wave_sum(q2);
    if (lane == 0) a.pctvar[(size_t)r * k + c] = q2 / ssY;
    SD_MARK(8);
    // beta starts as t / |t| (in `va`); XW row c = (t + mu) / |t| is final
    for (int p0 = 0; p0 < S; p0 += SD_TILE) {
        SD_TILE_PC(pc, p0);
        double b0v[SD_RC], x0v[SD_RC];
        SD_OWN(i) {
            const int x = xs[pc[i]];
            const double z = vt[pc[i]];
            b0v[i] = z / normt;
            x0v[i] = x >= 0 ? (z + mu) / normt : 0.0;
        }
        SD_OWN(i) if (SD_IN(p0, i)) { va[pc[i]] = b0v[i]; vt[pc[i]] = x0v[i]; }
    }
    if (c == k - 1) return;                    // last component: no basis vector, no product with K
    SD_MARK(9);
    // Gram-Schmidt against the previous basis pairs (v_j^T v = (K beta_j)^T beta), twice: the
    // coefficients of four basis vectors are taken together (block Gram-Schmidt: classical
    // inside a block of four, modified across blocks), so a pass is c / 4 reductions deep
    // The second pass is only run when the first one removed more than half of the squared norm (va enters with norm
    // one): otherwise what the first pass left of the earlier directions is below eps sqrt(2) already (the
    // re-orthogonalisation criterion of Daniel, Gragg, Kaufman and Stewart).
    double left = 1.0;
    for (int rep = 0; rep < 2 && (rep == 0 || left < 0.5); ++rep)
        for (int j0 = 0; j0 < c; j0 += 4) {
            const int j1 = min(j0 + 1, c - 1), j2 = min(j0 + 2, c - 1), j3 = min(j0 + 3, c - 1);
            const double *k0 = KB + (size_t)j0 * S, *k1 = KB + (size_t)j1 * S, *k2 = KB + (size_t)j2 * S,
                         *k3 = KB + (size_t)j3 * S;
            const double *b0 = BT + (size_t)j0 * S, *b1 = BT + (size_t)j1 * S, *b2 = BT + (size_t)j2 * S,
                         *b3 = BT + (size_t)j3 * S;
            double cf[4] = {0.0, 0.0, 0.0, 0.0};
            for (int p0 = 0; p0 < S; p0 += SD_TILE) {
                SD_TILE_PC(pc, p0);
                SD_OWN(i) {
                    const double bv = va[pc[i]], b = SD_IN(p0, i) ? bv : 0.0;
                    cf[0] += k0[pc[i]] * b; cf[1] += k1[pc[i]] * b; cf[2] += k2[pc[i]] * b; cf[3] += k3[pc[i]] * b;
                }
            }
            wave_sum4(cf[0], cf[1], cf[2], cf[3]);
            if (j0 + 1 >= c) cf[1] = 0.0;
            if (j0 + 2 >= c) cf[2] = 0.0;
            if (j0 + 3 >= c) cf[3] = 0.0;
            double nn = 0.0;
            for (int p0 = 0; p0 < S; p0 += SD_TILE) {
                SD_TILE_PC(pc, p0);
                double bb[SD_RC];
                SD_OWN(i) {
                    double b = va[pc[i]];
                    b -= cf[0] * b0[pc[i]]; b -= cf[1] * b1[pc[i]]; b -= cf[2] * b2[pc[i]]; b -= cf[3] * b3[pc[i]];
                    bb[i] = b;
                    nn += SD_IN(p0, i) ? b * b : 0.0;
                }
                SD_OWN(i) if (SD_IN(p0, i)) va[pc[i]] = bb[i];
            }
            if (rep == 0 && j0 + 4 >= c) left = wave_sum(nn);
        }
    SD_MARK(10);
    double bs = 0.0;
    for (int p0 = 0; p0 < S; p0 += SD_TILE) {
        SD_TILE_PC(pc, p0);
        SD_OWN(i) {
            const int x = xs[pc[i]];
            const double b = va[pc[i]];
            bs += (SD_IN(p0, i) && x >= 0) ? b : 0.0;
        }
    }
    const double bmean = wave_sum(bs) / ninc;
    for (int p0 = 0; p0 < S; p0 += SD_TILE) {
        SD_TILE_PC(pc, p0);
        double bc[SD_RC];
        SD_OWN(i) {
            const int x = xs[pc[i]];
            const double b = va[pc[i]];
            bc[i] = x >= 0 ? b - bmean : 0.0;
        }
        SD_OWN(i) if (SD_IN(p0, i)) va[pc[i]] = bc[i];
    }
    SD_MARK(11);
    // centred beta (consumed by the next launch) scattered to subject space for GEMM c
    if constexpr (GL) {
        wave_global_sync();
        sd_scatter_g(a.sfirst + (size_t)r * S, a.scnt + (size_t)r * S, S, lane, a.Wt + (size_t)r * S,
                     [&](int p) { return va[p]; });
    } else {
        sd_scatter(buf, xs, S, lane, a.Wt + (size_t)r * S, [&](int p) { return va[p]; });
    }
    SD_MARK(12);
}

// Outputs for the bootstrap: y_loadings = Y[ys]^T (X[xs] W), Y NOT re-centred
// (regression.py:325); dual weights scattered into k_xprod's A operand.
// With a.Qs the sign alignment of regression.py:317-320 happens HERE, in dual space:
//   flip_c = sign(corr(w_c, w0_c)) = sign(sum_b w_c[b] w0c_c[b]),  w_c = X0_r^T wd_c
//          = sign(sum_p wd_c[p] (Xc w0c_c)[xs_p]) = sign(sum_p WD[c][p] Qs[xs_p][c])
// (w0c centred over the features, wd_c centred over the positions), so the feature pass can
// accumulate the aligned weights directly (k_xprod EPI = 2) instead of writing them, forming
// their cross-Gram with the original and reading them back for the sign and the sums.
// dynamic LDS: k + S doubles per wave (GL: k -- the scatters go through sd_scatter_g).
template <int RC, int TC, bool GL = false>
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SD_WPE)))
void k_sd_final(SdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double sm_sd[];
    const int S = a.S, T = a.T, k = a.k, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: scalar pointers
    const int r = blockIdx.x * (blockDim.x >> 6) + wave;
    if (r >= a.nres) return;
    double* flip = sm_sd + (size_t)wave * (GL ? k : k + S);      // [k] signs + [S] scatter buffer
    const int* xs = a.xs + (size_t)r * S;
    const int* ys = a.ys + (size_t)r * S;
    const double* Ysrc = a.Yc + (size_t)r * a.y_stride;
    const double* XW = a.XW + (size_t)r * k * S;
    const double* WD = a.WD + (size_t)r * k * S;
    for (int c0 = 0; c0 < k; c0 += 4) {
        double s4[4] = {1.0, 1.0, 1.0, 1.0};
        if (a.Qs) {
            const double *w0 = WD + (size_t)min(c0, k - 1) * S, *w1 = WD + (size_t)min(c0 + 1, k - 1) * S,
                         *w2 = WD + (size_t)min(c0 + 2, k - 1) * S, *w3 = WD + (size_t)min(c0 + 3, k - 1) * S;
            s4[0] = s4[1] = s4[2] = s4[3] = 0.0;
            for (int p0 = 0; p0 < S; p0 += SD_TILE) {
                SD_TILE_PC(pc, p0);
                int xv[SD_RC];
                SD_OWN(i) xv[i] = xs[pc[i]];
                SD_OWN(i) {
                    const bool ok = SD_IN(p0, i) && xv[i] >= 0;
                    const double* q = a.Qs + (size_t)max(xv[i], 0) * k;
                    const double q0 = q[min(c0, k - 1)], q1 = q[min(c0 + 1, k - 1)], q2 = q[min(c0 + 2, k - 1)],
                                 q3 = q[min(c0 + 3, k - 1)];
                    s4[0] += ok ? w0[pc[i]] * q0 : 0.0; s4[1] += ok ? w1[pc[i]] * q1 : 0.0;
                    s4[2] += ok ? w2[pc[i]] * q2 : 0.0; s4[3] += ok ? w3[pc[i]] * q3 : 0.0;
                }
            }
            wave_sum4(s4[0], s4[1], s4[2], s4[3]);
        }
        if (lane == 0)
            for (int u = 0; u < 4 && c0 + u < k; ++u)
                flip[c0 + u] = (s4[u] > 0.0) ? 1.0 : ((s4[u] < 0.0) ? -1.0 : 0.0);
    }
    wave_sync();
    // y_loadings[t][c] = flip_c sum_p Y[ys_p][t] XW[c][p] over the included positions: on the matrix pipe (M = t, N = c)
    auto fy = [&](int t, int p, double (&v)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pp = min(p + j, S - 1);
            const int x = xs[pp], yy = ys[pp];
            const double yv = Ysrc[(size_t)yy * T + min(t, T - 1)];
            v[j] = (t < T && p + j < S && x >= 0) ? yv : 0.0;
        }
    };
    auto fw = [&](int c, int p, double (&v)[4]) {
        const double* src = XW + (size_t)min(c, k - 1) * S;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double w = src[min(p + j, S - 1)];
            v[j] = (c < k && p + j < S) ? w : 0.0;
        }
    };
    const int tt = (T + 15) >> 4, kt = (k + 15) >> 4;
#define SD_YL(MTL, NTL) {                                                                                          \
        d4 acc[MTL][NTL];                                                                                          \
        _Pragma("unroll") for (int i_ = 0; i_ < MTL; ++i_)                                                         \
            _Pragma("unroll") for (int j_ = 0; j_ < NTL; ++j_) acc[i_][j_] = (d4){0.0, 0.0, 0.0, 0.0};            \
        wave_mfma_nt<MTL, NTL>(acc, S, lane, fy, fw);                                                              \
        _Pragma("unroll") for (int mt = 0; mt < MTL; ++mt)                                                         \
            _Pragma("unroll") for (int nt = 0; nt < NTL; ++nt)                                                     \
                _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                    \
                    const int t = mt * 16 + (lane >> 4) + 4 * i, c = nt * 16 + (lane & 15);                        \
                    if (t < T && c < k) a.yload[((size_t)r * T + t) * k + c] = acc[mt][nt][i] * flip[c];          \
                }                                                                                                  \
    }
    if (TC == 0 && tt == 1 && kt == 1) SD_YL(1, 1)
    else if (TC == 0 && tt == 2 && kt == 1) SD_YL(2, 1)
    else if (TC == 1 && tt <= 4 && kt == 1) SD_YL(4, 1)
    else if (TC == 0 && tt <= 2 && kt <= 2) SD_YL(2, 2)
    else if (TC == 1 && tt <= 4 && kt <= 4) SD_YL(4, 4)
    else {
        for (int t = 0; t < T; ++t)
            for (int c0 = 0; c0 < k; c0 += 4) {
                const double *w0 = XW + (size_t)min(c0, k - 1) * S, *w1 = XW + (size_t)min(c0 + 1, k - 1) * S,
                             *w2 = XW + (size_t)min(c0 + 2, k - 1) * S, *w3 = XW + (size_t)min(c0 + 3, k - 1) * S;
                double s4[4] = {0.0, 0.0, 0.0, 0.0};
                for (int p0 = 0; p0 < S; p0 += SD_TILE) {
                    SD_TILE_PC(pc, p0);
                    SD_OWN(i) {
                        const int x = xs[pc[i]], yy = ys[pc[i]];
                        const double yv = Ysrc[(size_t)yy * T + t];
                        const double y = (SD_IN(p0, i) && x >= 0) ? yv : 0.0;
                        s4[0] += y * w0[pc[i]]; s4[1] += y * w1[pc[i]]; s4[2] += y * w2[pc[i]]; s4[3] += y * w3[pc[i]];
                    }
                }
                wave_sum4(s4[0], s4[1], s4[2], s4[3]);
                if (lane == 0)
                    for (int u = 0; u < 4 && c0 + u < k; ++u)
                        a.yload[((size_t)r * T + t) * k + c0 + u] = s4[u] * flip[c0 + u];
            }
    }
#undef SD_YL
    if (GL && a.Afrag) {
        const int g = r / a.lay.n, rr = r % a.lay.n;
        double* A = a.Afrag + (size_t)g * a.group_stride;
        const int* first = a.sfirst + (size_t)r * S;
        const int* nct = a.scnt + (size_t)r * S;
        for (int c = 0; c < k; ++c) {
            const double f = flip[c];
            const double* wdc = WD + (size_t)c * S;
            for (int i = lane; i < S; i += 64) {
                const int n = nct[i];
                double s = 0.0;
                if (n > 0) {
                    const double v = f * wdc[first[i]];
                    for (int m = 0; m < n; ++m) s += v;
                }
                A[afrag_off(rr * a.lay.Tp + c, i, a.lay.MT)] = s;
            }
        }
    } else if (a.Afrag) {
        const int g = r / a.lay.n, rr = r % a.lay.n;
        double* A = a.Afrag + (size_t)g * a.group_stride;
        // through the wave's LDS buffer, one component at a time (a subject drawn more than once receives bit-identical
        // addends, see sd_scatter), then plain stores: no global fp64 atomics (round 5)
        double* buf = flip + k;
        for (int c = 0; c < k; ++c) {
            const double f = flip[c];
            const double* wdc = WD + (size_t)c * S;
            for (int i = lane; i < S; i += 64) buf[i] = 0.0;
            wave_sync();
            for (int p = lane; p < S; p += 64) {
                const int x = xs[p];
                if (x >= 0) atomicAdd(&buf[x], f * wdc[p]);
            }
            wave_sync();
            for (int i = lane; i < S; i += 64) A[afrag_off(rr * a.lay.Tp + c, i, a.lay.MT)] = buf[i];
            wave_sync();
        }
    }
    if (a.Vd) {
        // dense, one row per component: scattered through the wave's LDS buffer (every entry written: no memset, no
        // global atomics)
        double* V = a.Vd + (size_t)r * k * S;
        double* buf = flip + k;
        for (int c = 0; c < k; ++c) {
            const double f = flip[c];
            const double* wdc = WD + (size_t)c * S;
            if constexpr (GL)
                sd_scatter_g(a.sfirst + (size_t)r * S, a.scnt + (size_t)r * S, S, lane, V + (size_t)c * S,
                             [&](int p) { return f * wdc[p]; });
            else
                sd_scatter(buf, xs, S, lane, V + (size_t)c * S, [&](int p) { return f * wdc[p]; });
        }
    }
}

// Usable test position p of a cross-validated fit: outside its training mask `pm` and not a masked (all-NaN) row of X
// or of the Y row the fit observes there -- p itself, under PERM row ysp[p] (`ysp`: the fit's `ys`): get_mask(X,
// Y[perm]).  The one definition k_sd_cv_score, k_sd_cv_class and k_sd_cv_auc share.
template <bool PERM>
__device__ __forceinline__ bool sd_cv_is_test(const SdArgs& a, const uint8_t* pm, const int* ysp, int p)
{
    return !pm[p] && (!a.okx || a.okx[p]) && (!a.oky || a.oky[PERM ? ysp[p] : p]);
}

// One step of the running prediction of a cross-validated fit, yhat_c = yhat_{c-1} + z_c q_c: the ONE expression
// k_sd_cv_score, k_sd_cv_class, k_sd_cv_auc and k_sd_cv_pred update their predictions with, so that what the last
// returns is what the others scored, classified and ranked.
__device__ __forceinline__ double sd_cv_step(double yhat, double z, double q) { return yhat + z * q; }

// The y-loadings q_j[t] = sum_p Y0[t][p] z_j[p] of four components (rows z0 .. z3 of the centred Z, clamped by the
// caller) as per-lane partial sums for k_sd_cv_pred, in the order of k_sd_cv_score's own loop below: a lane adds the
// products of the positions it owns in ascending order, whatever the tile, and the caller reduces with wave_sum4 -- the
// same sums, bit for bit.  (k_sd_cv_score keeps its loop in place, where it takes the test means of the scores along:
// routed through this function its instantiations come out of the compiler as other code, 100 instructions shorter
// at RC = 16 and 17 longer at RC = 8; DESIGN.md section 5, "Out-of-fold predictions".)
template <int RC>
__device__ __forceinline__ void sd_cv_q4(const double* y0t, const double* z0, const double* z1, const double* z2,
                                         const double* z3, int S, int lane, double (&q)[4])
{
    for (int p0 = 0; p0 < S; p0 += SD_TILE) {
        SD_TILE_PC(pc, p0);
        SD_OWN(i) {
            const bool in = SD_IN(p0, i);
            const double yv = y0t[pc[i]], y = in ? yv : 0.0;
            const double a0 = z0[pc[i]], a1 = z1[pc[i]], a2 = z2[pc[i]], a3 = z3[pc[i]];
            q[0] += y * a0; q[1] += y * a1; q[2] += y * a2; q[3] += y * a3;
        }
    }
}

// Cross-validation of one train / test split (plsx_simpls_crossval_batch), after the solver ran on the training rows
// (a.pmask: test positions excluded like masked rows) and Z = Vd . K was formed.  With wd_j the dual weights (centred
// over the training rows, zero elsewhere) and K of the bound, globally centred data,
//     (x_i - xbar_tr)^T w_j = Z_j[i] - mean_{p in tr} Z_j[p] = t_j[i]     for EVERY row i, training or test,
//     q_j = (Y_tr - ybar_tr)^T t_j = sum_p Y0[.][p] t_j[p]                (Y0 is zero off the training rows),
//     yhat_c[i] = ybar_tr + sum_{j <= c} t_j[i] q_j^T,   c = 1 .. k, nested
// -- what [1, x_i] @ simpls(X_tr, Y_tr, c)['beta'] predicts.  Per behaviour t and component count c the test rows give
// Pearson r (compute.efficient_corr), R^2 (sklearn r2_score, raw values) and the summed squared error; row 0 of the
// latter is the intercept-only model.  The residual y - yhat is accumulated directly (sum y^2 - 2 sum y yhat + sum yhat^2
// cancels when the model fits), the means are taken first (the mean of yhat_c over the test rows follows from the means
// of the scores), reductions are wave_sum4 in fixed order.  One wavefront per split, lanes over positions; no LDS on
// either route: the running prediction lives in the split's `va` (idle once the solver is through), every position
// of every S-long vector is only ever touched by the lane that owns it.  Four components at a time.
//
// PERM (plsx_simpls_crossval_perm_batch): the fit ran on (X, Y[ysrc]); the observed row of position p is row ys[p] of Y
// and the position is usable iff okx[p] and oky[ys[p]] -- get_mask(X, Y[perm]).  The loads of Y go through the fit's
// `ys` (a gather of rows of T doubles); everything else, the order of every reduction included, is the identity
// variant's, whose instantiations are what they were.  The usable test rows of the fit go out too (cvnte): under a
// permutation they are not the split's own.
template <int RC, bool PERM = false>
static __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SD_WPE)))
void k_sd_cv_score(SdArgs a)
{
    const int S = a.S, T = a.T, k = a.k, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: scalar pointers
    const int r = blockIdx.x * (blockDim.x >> 6) + wave;
    if (r >= a.nres) return;
    const int* xs = a.xs + (size_t)r * S;
    const uint8_t* pm = a.pmask + (size_t)r * S;
    const double* Y0 = a.Y0 + (size_t)r * S * T;
    const double* ym = a.ymean + (size_t)r * T;
    // identity sources: the observed row of position p is row p of the fit's own Y (y_stride = 0: of the bound Y)
    const double* Yc = PERM ? a.Yc : a.Yc + (size_t)r * a.y_stride;
    const int* ysp = a.ys + (size_t)r * S;                 // (PERM: ... is row ys[p])
    auto yrow = [&](int p) { if constexpr (PERM) return ysp[p]; else return p; };
    double* Z = a.cvZ + (size_t)r * k * S;
    double* yh = a.va + (size_t)r * S;
    double* out_r = a.cvr + (size_t)r * k * T;
    double* out_r2 = a.cvr2 + (size_t)r * k * T;
    double* out_sse = a.cvsse + (size_t)r * (k + 1) * T;
    const double ninc = a.scal[(size_t)r * 4];
    auto is_test = [&](int p) { return sd_cv_is_test<PERM>(a, pm, ysp, p); };
    // ---- scores of every position, centred by their training mean (in place)
    for (int j0 = 0; j0 < k; j0 += 4) {
        double* z0 = Z + (size_t)min(j0, k - 1) * S;
        double* z1 = Z + (size_t)min(j0 + 1, k - 1) * S;
        double* z2 = Z + (size_t)min(j0 + 2, k - 1) * S;
        double* z3 = Z + (size_t)min(j0 + 3, k - 1) * S;
        double m[4] = {0.0, 0.0, 0.0, 0.0};
        for (int p0 = 0; p0 < S; p0 += SD_TILE) {
            SD_TILE_PC(pc, p0);
            SD_OWN(i) {
                const bool tr = SD_IN(p0, i) && xs[pc[i]] >= 0;
                const double a0 = z0[pc[i]], a1 = z1[pc[i]], a2 = z2[pc[i]], a3 = z3[pc[i]];
                m[0] += tr ? a0 : 0.0; m[1] += tr ? a1 : 0.0; m[2] += tr ? a2 : 0.0; m[3] += tr ? a3 : 0.0;
            }
        }
        wave_sum4(m[0], m[1], m[2], m[3]);
#pragma unroll
        for (int u = 0; u < 4; ++u) m[u] /= ninc;
        for (int p0 = 0; p0 < S; p0 += SD_TILE) {
            SD_TILE_PC(pc, p0);
            SD_OWN(i) {
                const double a0 = z0[pc[i]], a1 = z1[pc[i]], a2 = z2[pc[i]], a3 = z3[pc[i]];
                if (SD_IN(p0, i)) {
                    z0[pc[i]] = a0 - m[0];
                    if (j0 + 1 < k) z1[pc[i]] = a1 - m[1];
                    if (j0 + 2 < k) z2[pc[i]] = a2 - m[2];
                    if (j0 + 3 < k) z3[pc[i]] = a3 - m[3];
                }
            }
        }
    }
    double cnt = 0.0;
    for (int p = lane; p < S; p += 64) cnt += is_test(p) ? 1.0 : 0.0;
    const double nte = wave_sum(cnt);
    if constexpr (PERM)
        if (lane == 0) a.cvnte[r] = nte;
    for (int t = 0; t < T; ++t) {
        const double ymt = ym[t];
        // observed test values: mean, then the sums of squares about it and about the training mean
        double sy = 0.0;
        for (int p = lane; p < S; p += 64) sy += is_test(p) ? Yc[(size_t)yrow(p) * T + t] : 0.0;
        const double ybar = wave_sum(sy) / nte;
        double syy = 0.0, se0 = 0.0;
        for (int p = lane; p < S; p += 64) {
            const bool te = is_test(p);
            const double y = Yc[(size_t)yrow(p) * T + t];
            const double d = y - ybar, e = y - ymt;
            syy += te ? d * d : 0.0;
            se0 += te ? e * e : 0.0;
        }
        syy = wave_sum(syy);
        se0 = wave_sum(se0);
        if (lane == 0) out_sse[t] = se0;
        const double* y0t = Y0 + (size_t)t * S;
        double mhat = ymt;                                 // mean of the running prediction over the test rows
        for (int c0 = 0; c0 < k; c0 += 4) {
            const double* z0 = Z + (size_t)min(c0, k - 1) * S;
            const double* z1 = Z + (size_t)min(c0 + 1, k - 1) * S;
            const double* z2 = Z + (size_t)min(c0 + 2, k - 1) * S;
            const double* z3 = Z + (size_t)min(c0 + 3, k - 1) * S;
            // y-loadings q_c[t] of the four components and the test means of their scores
            double q[4] = {0.0, 0.0, 0.0, 0.0}, mt[4] = {0.0, 0.0, 0.0, 0.0};
            for (int p0 = 0; p0 < S; p0 += SD_TILE) {
                SD_TILE_PC(pc, p0);
                SD_OWN(i) {
                    const bool in = SD_IN(p0, i), te = in && is_test(pc[i]);
                    const double yv = y0t[pc[i]], y = in ? yv : 0.0;
                    const double a0 = z0[pc[i]], a1 = z1[pc[i]], a2 = z2[pc[i]], a3 = z3[pc[i]];
                    q[0] += y * a0; q[1] += y * a1; q[2] += y * a2; q[3] += y * a3;
                    mt[0] += te ? a0 : 0.0; mt[1] += te ? a1 : 0.0; mt[2] += te ? a2 : 0.0; mt[3] += te ? a3 : 0.0;
                }
            }
            wave_sum4(q[0], q[1], q[2], q[3]);
            wave_sum4(mt[0], mt[1], mt[2], mt[3]);
            double mh[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c0 + u >= k) q[u] = 0.0;               // (a clamped row: the prediction stays as it is)
                mhat += (mt[u] / nte) * q[u];
                mh[u] = mhat;
            }
            double se[4] = {0.0, 0.0, 0.0, 0.0}, shh[4] = {0.0, 0.0, 0.0, 0.0}, shy[4] = {0.0, 0.0, 0.0, 0.0};
            const bool more = c0 + 4 < k;
            for (int p0 = 0; p0 < S; p0 += SD_TILE) {
                SD_TILE_PC(pc, p0);
                SD_OWN(i) {
                    const bool te = SD_IN(p0, i) && is_test(pc[i]);
                    const double y = Yc[(size_t)yrow(pc[i]) * T + t];
                    const double zz[4] = {z0[pc[i]], z1[pc[i]], z2[pc[i]], z3[pc[i]]};
                    double pred = c0 == 0 ? ymt : yh[pc[i]];
                    const double dy = y - ybar;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        pred = sd_cv_step(pred, zz[u], q[u]);
                        const double e = y - pred, d = pred - mh[u];
                        se[u] += te ? e * e : 0.0;
                        shh[u] += te ? d * d : 0.0;
                        shy[u] += te ? d * dy : 0.0;
                    }
                    if (more && te) yh[pc[i]] = pred;
                }
            }
            wave_sum4(se[0], se[1], se[2], se[3]);
            wave_sum4(shh[0], shh[1], shh[2], shh[3]);
            wave_sum4(shy[0], shy[1], shy[2], shy[3]);
            if (lane == 0)
                for (int u = 0; u < 4 && c0 + u < k; ++u) {
                    const double rr = shy[u] / sqrt(shh[u] * syy);
                    out_r[(size_t)(c0 + u) * T + t] = rr > 1.0 ? 1.0 : (rr < -1.0 ? -1.0 : rr);      // (NaN stays NaN)
                    out_r2[(size_t)(c0 + u) * T + t] = 1.0 - se[u] / syy;
                    out_sse[(size_t)(c0 + u + 1) * T + t] = se[u];
                }
        }
    }
}

// The class prediction of a cross-validated fit (PLS-DA), after k_sd_cv_score centred Z in place: what k_sd_cv_class
// takes the argmax of and k_sd_cv_auc ranks, defined HERE ONCE for both so that their counts speak of the same numbers.
// The bound Y is the indicator matrix of G = T classes minus its column means over all S rows (a.cfreq = n_g / S), a.cls
// the class code of every row; so the fit's Y0[g][p] = [class of p is g] - f_g on its training positions, with
// f_g = ymean[g] + cfreq[g] the class frequency among them, and zero elsewhere.  Per component count c = 1 .. k:
//     q_c[g]     = sum_p Y0[g][p] z_c[p] = s_g - f_g sum_h s_h,   s_g = sum of z_c over the training positions of class g
//                  (Y0 is not read: one pass over z_c and the class codes instead of G passes over S doubles each -- the
//                  batch's Y0, 8 G S bytes per fit, does not stay in cache between the component counts)
//     yhat_c[p]  = yhat_{c-1}[p] + z_c[p] q_c                  (yhat_0 = f: the prediction k_sd_cv_score scores, plus the
//                                                               column means that the global centring of the bound
//                                                               indicators took away -- the classes are read off the
//                                                               RAW indicators' prediction)
// One wavefront per fit r, lanes over positions.  f, s_g / q_c: GB registers per lane (GB the compile-time bound of G:
// 4, 16 or 32).  The role of every position is one int in the first half of the fit's `va` (S ints in S doubles, idle
// once k_sd_cv_score is through), written and read by the lane that owns p only.  PERM as for k_sd_cv_score: rows of Y
// and their classes go through the fit's `ys`.  Each kernel keeps the running prediction yhat its own way.

// role of position p: its class on a training position, 64 + its class on a usable test position, -1 otherwise
template <bool PERM>
__device__ __forceinline__ void sd_cv_roles(const SdArgs& a, int r, int lane, int* role)
{
    const int S = a.S;
    const int* xs = a.xs + (size_t)r * S;
    const uint8_t* pm = a.pmask + (size_t)r * S;
    const int* ysp = a.ys + (size_t)r * S;
    for (int p = lane; p < S; p += 64) {
        const bool te = sd_cv_is_test<PERM>(a, pm, ysp, p);
        role[p] = (xs[p] >= 0 || te) ? (a.cls[PERM ? ysp[p] : p] | (te ? 64 : 0)) : -1;
    }
}

// f_g, the class frequencies among the fit's training positions: yhat_0
template <int GB>
__device__ __forceinline__ void sd_cv_class_f(const SdArgs& a, int r, double (&f)[GB])
{
    const int G = a.T;
    const double* ym = a.ymean + (size_t)r * G;
#pragma unroll
    for (int g = 0; g < GB; ++g) f[g] = g < G ? ym[g] + a.cfreq[g] : 0.0;
}

// q_c[g] of component c from its centred scores zc: one pass for s_g, reduced four classes at a time in fixed order.
// (s is an array of the helper's own, copied out at the end: accumulated through the out-parameter, the compiler
// keeps it in another form than the kernels' own arrays and k_sd_cv_class<16> takes 141 VGPRs instead of 123.)
template <int GB>
__device__ __forceinline__ void sd_cv_class_q(const int* role, const double* zc, int S, int G, int lane,
                                              const double (&f)[GB], double (&q)[GB])
{
    double s[GB];
#pragma unroll
    for (int g = 0; g < GB; ++g) s[g] = 0.0;
    for (int p = lane; p < S; p += 64) {
        const int rl = role[p];
        const double z = zc[p];
#pragma unroll
        for (int g = 0; g < GB; ++g) s[g] += rl == g ? z : 0.0;
    }
#pragma unroll
    for (int g = 0; g < GB; g += 4)
        if (g < G) wave_sum4(s[g], s[g + 1], s[g + 2], s[g + 3]);
    double sall = 0.0;
#pragma unroll
    for (int g = 0; g < GB; ++g) sall += s[g];
#pragma unroll
    for (int g = 0; g < GB; ++g) q[g] = s[g] - f[g] * sall;
}

// Classification of the test rows of one fit (plsx_simpls_cv_class_begin), on the prediction above:
//     conf[c][class of p][first maximum of yhat_c[p]] += 1     for every usable test position p
// The first maximum is numpy's argmax: the lowest index on a tie.  The running prediction of position p lives in the
// fit's Z0 rows -- [G][S], idle once the solver is through -- touched by the lane that owns p only, and the G x G
// counters of the open c in the wave's LDS slice (integer atomics: exact in any order).  After each c the non-zero
// counters are added to the fit's block with integer atomics: under PERM the n splits of a permutation share one
// block, which was zeroed when it was appended.
template <int GB, bool PERM>
static __global__ __launch_bounds__(256)
void k_sd_cv_class(SdArgs a)
{
    __shared__ int sm_cnt[4][GB * GB];
    const int S = a.S, G = a.T, k = a.k, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: scalar pointers
    const int r = blockIdx.x * 4 + wave;
    if (r >= a.nres) return;
    const double* Z = a.cvZ + (size_t)r * k * S;
    double* yh = a.Z0 + (size_t)r * S * G;
    int* role = reinterpret_cast<int*>(a.va + (size_t)r * S);
    const long long blk = (a.cls_f0 + r) / a.cls_n - a.cls_f0 / a.cls_n;       // (64-bit, as the pair list itself)
    int* out = a.conf + (size_t)blk * k * G * G;
    int* cnt = sm_cnt[wave];
    sd_cv_roles<PERM>(a, r, lane, role);
    double f[GB];
    sd_cv_class_f(a, r, f);
    for (int c = 0; c < k; ++c) {
        const double* zc = Z + (size_t)c * S;
        double q[GB];
        sd_cv_class_q(role, zc, S, G, lane, f, q);
        for (int i = lane; i < G * G; i += 64) cnt[i] = 0;
        wave_sync();
        for (int p = lane; p < S; p += 64) {
            const int rl = role[p];
            if (rl < 64) continue;
            const double z = zc[p];
            double best = 0.0;
            int arg = 0;
#pragma unroll
            for (int g = 0; g < GB; ++g)
                if (g < G) {
                    const double v = sd_cv_step(c == 0 ? f[g] : yh[(size_t)g * S + p], z, q[g]);
                    if (c + 1 < k) yh[(size_t)g * S + p] = v;
                    if (g == 0 || v > best) { best = v; arg = g; }
                }
            atomicAdd(&cnt[(rl - 64) * G + arg], 1);
        }
        wave_sync();
        for (int i = lane; i < G * G; i += 64) {
            const int v = cnt[i];
            if (v) atomicAdd(&out[(size_t)c * G * G + i], v);
        }
        wave_sync();
    }
}

// What lanes of this wave stored to global memory is visible to its other lanes, and no more than that: a fence of
// workgroup scope (the wave's stores have reached the compute unit's write-through L1, which its loads go through)
// instead of wave_global_sync()'s device-wide one, whose write-back of L2 is paid by every wave that calls it
// ("PLS-DA: AUC").
__device__ __forceinline__ void wave_cu_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// 64-bit integer sum over the wave (exact in any order)
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One-vs-rest AUC counts of the test rows of one fit (plsx_simpls_cv_auc_begin), behind k_sd_cv_score and, where that
// series is open too, k_sd_cv_class in stream order.  Per component count c and class g, with pos the usable test
// positions of true class g, neg the other usable test positions and v[p] = yhat_c[p][g], the class prediction defined
// above k_sd_cv_class (sd_cv_roles, sd_cv_class_f, sd_cv_class_q: the same helpers, hence the same numbers),
//     u2    = sum over i in pos, j in neg of (2 if v[i] > v[j], 1 if v[i] == v[j], else 0)       twice Mann-Whitney's U
//     pairs = |pos| |neg|
// A comparison with a NaN is false both ways: the pair counts in `pairs` and adds nothing to u2.  Where things live
// beyond the roles (all of it idle once k_sd_cv_score and k_sd_cv_class are through): the usable test positions listed
// CLASS BY CLASS in the second half of the fit's `va` (S more ints), where the list of class g starts in the wave's LDS
// slice, the running prediction of listed position i in the fit's Z0 rows, [G][S] indexed by the place in the list --
// so the positives of a class are contiguous and a lane that owns one is never idle because its neighbour's position
// belongs to another class.  Per class the lanes own the
// positives, 64 at a time, and walk the negatives, which the wave stages 64 at a time in its LDS slice (a read of one
// address by every lane); a lane without a positive, and a staged place without a negative, hold a NaN and count
// nothing.  Per-lane counts are 32-bit (at most ceil(S / 64) S comparisons per lane and class), their sum over the wave
// 64-bit, and one lane adds u2 and pairs to the fit's block with 64-bit integer atomics: under PERM the n splits of a
// permutation share one block, which was zeroed when it was appended.  The list and the predictions are written by one
// lane and read by another through global memory: wave_cu_sync() between.
template <int GB, bool PERM>
static __global__ __launch_bounds__(256)
void k_sd_cv_auc(SdArgs a)
{
    __shared__ double sm_stage[4][64];
    __shared__ int sm_start[4][GB + 1];
    const int S = a.S, G = a.T, k = a.k, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: scalar pointers
    const int r = blockIdx.x * 4 + wave;
    if (r >= a.nres) return;
    const double* Z = a.cvZ + (size_t)r * k * S;
    double* yh = a.Z0 + (size_t)r * S * G;
    int* role = reinterpret_cast<int*>(a.va + (size_t)r * S);                  // (S ints in the first half of the fit's S doubles)
    int* list = role + S;                                                      // (... and S ints in the second)
    const long long blk = (a.cls_f0 + r) / a.cls_n - a.cls_f0 / a.cls_n;       // (64-bit, as the pair list itself)
    unsigned long long* out = reinterpret_cast<unsigned long long*>(a.auc) + (size_t)blk * k * G * 2;
    double* stage = sm_stage[wave];
    int* start = sm_start[wave];
    const double nan = __builtin_nan("");
    sd_cv_roles<PERM>(a, r, lane, role);
    // the usable test positions, class by class and ascending within a class: list[start[g] .. start[g + 1])
    int nl = 0;
    for (int g = 0; g < G; ++g) {
        if (lane == 0) start[g] = nl;
        for (int p0 = 0; p0 < S; p0 += 64) {
            const int p = p0 + lane;
            const bool hit = p < S && role[p] == (64 | g);
            const unsigned long long m = __ballot(hit);
            if (hit) list[nl + __popcll(m & ((1ull << lane) - 1ull))] = p;     // (nl + rank < the S usable positions at most)
            nl += __popcll(m);
        }
    }
    if (lane == 0) start[G] = nl;
    wave_cu_sync();
    double f[GB];
    sd_cv_class_f(a, r, f);
    for (int c = 0; c < k; ++c) {
        const double* zc = Z + (size_t)c * S;
        double q[GB];
        sd_cv_class_q(role, zc, S, G, lane, f, q);
        // the running prediction of the listed positions
        for (int i = lane; i < nl; i += 64) {
            const double z = zc[list[i]];
#pragma unroll
            for (int g = 0; g < GB; ++g)
                if (g < G) {
                    const double v = sd_cv_step(c == 0 ? f[g] : yh[(size_t)g * S + i], z, q[g]);
                    yh[(size_t)g * S + i] = v;
                }
        }
        wave_cu_sync();
        for (int g = 0; g < G; ++g) {
            const int s0 = start[g], npos = start[g + 1] - s0, nneg = nl - npos;
            if (npos == 0 || nneg == 0) continue;                              // (wave-uniform)
            const double* vg = yh + (size_t)g * S;
            unsigned long long u2 = 0;
            for (int i0 = 0; i0 < npos; i0 += 64) {
                const double vi = i0 + lane < npos ? vg[s0 + i0 + lane] : nan;
                unsigned gt = 0, eq = 0;
                for (int t0 = 0; t0 < nneg; t0 += 64) {
                    const int t = t0 + lane;                                   // the t-th negative: the list without [s0, s0 + npos)
                    const double vj = t < nneg ? vg[t < s0 ? t : t + npos] : nan;
                    wave_sync();                                               // (the reads of the last 64 are through)
                    stage[lane] = vj;
                    wave_sync();
#pragma unroll
                    for (int u = 0; u < 64; ++u) {
                        const double w = stage[u];
                        gt += vi > w ? 1u : 0u;
                        eq += vi == w ? 1u : 0u;
                    }
                }
                u2 += 2ull * gt + eq;
            }
            u2 = wave_sum_u64(u2);
            if (lane == 0) {
                atomicAdd(&out[((size_t)c * G + g) * 2], u2);
                atomicAdd(&out[((size_t)c * G + g) * 2 + 1], (unsigned long long)npos * (unsigned long long)nneg);
            }
        }
        wave_cu_sync();                                                    // (this c's reads before the next c's writes)
    }
}

// The out-of-fold predictions of an open series (plsx_simpls_cv_pred_begin): which fits of the batch are kept and where.
struct SdPredArgs {
    double* pred;               // slots [T][S] of the caller's stack, from the batch's first kept fit on
    double* ytrue;              // the same slots of the observed values, or nullptr
    int* ncomp_out;             // [slots] the component count used, or nullptr
    const int* ncomp_in;        // [slots] the component count to use (the nested selection's; 0: undefined), or nullptr: c
    int c;                      // ... the count of every slot
    int unit, slots;            // slot i is fit i * unit of the batch (nested: the outer member of group i)
};

// The predictions themselves, behind k_sd_cv_score (and k_sd_cv_class / k_sd_cv_auc / k_sd_cvn_select where they run):
// slot [t][p] = yhat_c[p][t] of the c-component model on the usable test positions p of the fit, NaN on every other
// position -- all S positions of all T rows are written.  One wavefront per kept fit, lanes over positions, no LDS on
// either solver route; the running prediction lives in the slot itself, touched by the lane that owns p only.
//   GB = 0 (regression): q_j[t] from the fit's Y0 and the centred Z by sd_cv_q4 -- four components at a time, wave_sum4,
//     the order of k_sd_cv_score's own loop -- then yhat = ybar_tr, yhat = sd_cv_step(yhat, z_j, q_j[t]) for j ascending; a row
//     beyond c in the last group of four has q = 0 and leaves yhat as it is, as a row beyond k does there.
//   GB > 0 (PLS-DA, the bound of G as in k_sd_cv_class): the prediction of the RAW indicators by sd_cv_roles,
//     sd_cv_class_f and sd_cv_class_q, one component at a time as in k_sd_cv_class (the roles are written to the first
//     half of the fit's `va` again: the same ints).
// ytrue: row p of the fit's own Y (y_stride) at the same positions.
template <int GB>
static __global__ __launch_bounds__(256)
void k_sd_cv_pred(SdArgs a, SdPredArgs pa)
{
    constexpr int RC = 8;                                  // (the tile of sd_cv_q4; the sums do not depend on it)
    const int S = a.S, T = a.T, k = a.k, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: scalar pointers
    const int slot = blockIdx.x * 4 + wave;
    if (slot >= pa.slots) return;
    const int r = slot * pa.unit;
    int c = pa.ncomp_in ? pa.ncomp_in[slot] : pa.c;
    c = c < 0 ? 0 : (c > k ? k : c);
    if (pa.ncomp_out && lane == 0) pa.ncomp_out[slot] = c;
    const uint8_t* pm = a.pmask + (size_t)r * S;
    const int* ysp = a.ys + (size_t)r * S;
    const double* Z = a.cvZ + (size_t)r * k * S;
    double* out = pa.pred + (size_t)slot * T * S;
    const double nan = __builtin_nan("");
    if (pa.ytrue) {
        const double* Yc = a.Yc + (size_t)r * a.y_stride;
        double* yt = pa.ytrue + (size_t)slot * T * S;
        for (int t = 0; t < T; ++t)
            for (int p = lane; p < S; p += 64)
                yt[(size_t)t * S + p] = sd_cv_is_test<false>(a, pm, ysp, p) ? Yc[(size_t)p * T + t] : nan;
    }
    if (c == 0) {                                          // (an undefined group of the nested selection)
        for (int i = lane; i < T * S; i += 64) out[i] = nan;
        return;
    }
    if constexpr (GB == 0) {
        const double* Y0 = a.Y0 + (size_t)r * S * T;
        const double* ym = a.ymean + (size_t)r * T;
        for (int t = 0; t < T; ++t) {
            const double ymt = ym[t];
            const double* y0t = Y0 + (size_t)t * S;
            double* o = out + (size_t)t * S;
            for (int c0 = 0; c0 < c; c0 += 4) {
                const double* z0 = Z + (size_t)min(c0, k - 1) * S;
                const double* z1 = Z + (size_t)min(c0 + 1, k - 1) * S;
                const double* z2 = Z + (size_t)min(c0 + 2, k - 1) * S;
                const double* z3 = Z + (size_t)min(c0 + 3, k - 1) * S;
                double q[4] = {0.0, 0.0, 0.0, 0.0};
                sd_cv_q4<RC>(y0t, z0, z1, z2, z3, S, lane, q);
                wave_sum4(q[0], q[1], q[2], q[3]);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (c0 + u >= c) q[u] = 0.0;
                const bool last = c0 + 4 >= c;
                for (int p = lane; p < S; p += 64) {
                    double pred = c0 == 0 ? ymt : o[p];
                    pred = sd_cv_step(pred, z0[p], q[0]);
                    pred = sd_cv_step(pred, z1[p], q[1]);
                    pred = sd_cv_step(pred, z2[p], q[2]);
                    pred = sd_cv_step(pred, z3[p], q[3]);
                    o[p] = (last && !sd_cv_is_test<false>(a, pm, ysp, p)) ? nan : pred;
                }
            }
        }
    } else {
        const int G = T;
        int* role = reinterpret_cast<int*>(a.va + (size_t)r * S);
        sd_cv_roles<false>(a, r, lane, role);
        double f[GB];
        sd_cv_class_f(a, r, f);
        for (int j = 0; j < c; ++j) {
            const double* zc = Z + (size_t)j * S;
            double q[GB];
            sd_cv_class_q(role, zc, S, G, lane, f, q);
            const bool last = j + 1 == c;
            for (int p = lane; p < S; p += 64) {
                const bool te = role[p] >= 64;
                const double z = zc[p];
#pragma unroll
                for (int g = 0; g < GB; ++g)
                    if (g < G) {
                        const double v = sd_cv_step(j == 0 ? f[g] : out[(size_t)g * S + p], z, q[g]);
                        out[(size_t)g * S + p] = (last && !te) ? nan : v;
                    }
            }
        }
    }
}

// Cross-validation under permuted Y: the (permutation, split) fits f0 .. f0 + ms - 1 of the pair list, fit f = permutation
// f / n under split f % n (64-bit: P n overflows an int long before memory does).  The solver's per-fit Y sources and
// position masks are expanded here from the m permutation rows and the n mask rows, so 5 S bytes per fit never leave
// the host.  grid (ceil(S / 256), ms).
static __global__ __launch_bounds__(256)
void k_sd_cvp_expand(const int* __restrict__ perm, const uint8_t* __restrict__ masks, int S, int n, long long f0,
                     int* __restrict__ ysrc, uint8_t* __restrict__ pmask)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S) return;
    const long long f = f0 + blockIdx.y;
    const long long pi = f / n, si = f % n;
    ysrc[(size_t)blockIdx.y * S + p] = perm[(size_t)pi * S + p];
    pmask[(size_t)blockIdx.y * S + p] = masks[(size_t)si * S + p];
}

// ... and their reduction over the splits: out_r / out_r2 [.][k][T] and out_mse [.][k + 1] of permutation pi take the
// scores of its fits in this batch, added ONE BY ONE IN SPLIT ORDER to what the earlier batches left there (the entry
// starts from zero), and are divided by n once the last split is in.  The running sum is carried through the output
// itself, so a permutation whose splits straddle solver batches is summed in exactly the association of one that does
// not: the same bits whatever the batch size.  One thread per output entry, no atomics.  mse of a fit: the squared
// errors summed over the behaviours in ascending t, over the fit's own usable test rows.  grid (ceil(E / 256), perms
// touched), E = 2 k T + k + 1; pi0 = f0 / n.
static __global__ __launch_bounds__(256)
void k_sd_cvp_reduce(const double* __restrict__ r, const double* __restrict__ r2, const double* __restrict__ sse,
                     const double* __restrict__ nte, int k, int T, int n, long long f0, int ms,
                     double* __restrict__ out_r, double* __restrict__ out_r2, double* __restrict__ out_mse)
{
    const int kT = k * T, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * kT + k + 1) return;
    const long long pi = f0 / n + blockIdx.y;
    const long long lo = pi * n > f0 ? pi * n : f0, end = (pi + 1) * n < f0 + ms ? (pi + 1) * n : f0 + ms;
    const bool last = end == (pi + 1) * n;
    if (e < 2 * kT) {
        const double* src = e < kT ? r + e : r2 + (e - kT);
        double* dst = e < kT ? out_r + (size_t)pi * kT + e : out_r2 + (size_t)pi * kT + (e - kT);
        double acc = *dst;
        for (long long f = lo; f < end; ++f) acc += src[(size_t)(f - f0) * kT];
        *dst = last ? acc / n : acc;
    } else {
        const int c = e - 2 * kT;
        double* dst = out_mse + (size_t)pi * (k + 1) + c;
        double acc = *dst;
        for (long long f = lo; f < end; ++f) {
            const double* row = sse + ((size_t)(f - f0) * (k + 1) + c) * T;
            double s = 0.0;
            for (int t = 0; t < T; ++t) s += row[t];
            acc += s / nte[f - f0];
        }
        *dst = last ? acc / n : acc;
    }
}

// Nested cross-validation (plsx_simpls_crossval_nested_batch, plsx_simpls_crossval_nested_perm_batch): inner splits
// inside the training rows of every outer split choose the component count, the outer test rows score the chosen model.
// The position masks carry CODES: 1 = training row, 0 = test row, 2 = on neither side (the outer test rows under an
// inner fold) -- k_sd_init includes a position iff its code is 1, sd_cv_is_test takes it iff its code is 0.  The fit
// list: fit f = group f / (1 + ni), member f % (1 + ni); group g = permutation g / n under outer split g % n; member 0
// the outer fit, members 1 .. ni the inner fits (64-bit, as the pair list of k_sd_cvp_expand).  The codes come as
// [n][1 + ni][S].  perm = nullptr: the identity (the observed data).  grid (ceil(S / 256), ms).
static __global__ __launch_bounds__(256)
void k_sd_cvn_expand(const int* __restrict__ perm, const uint8_t* __restrict__ codes, int S, int n, int ni, long long f0,
                     int* __restrict__ ysrc, uint8_t* __restrict__ pmask)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S) return;
    const long long f = f0 + blockIdx.y;
    const long long g = f / (1 + ni), mem = f % (1 + ni);
    const long long pi = g / n, si = g % n;
    ysrc[(size_t)blockIdx.y * S + p] = perm ? perm[(size_t)pi * S + p] : p;
    pmask[(size_t)blockIdx.y * S + p] = codes[((size_t)si * (1 + ni) + mem) * S + p];
}

// ... the selection of a group, next to its fits: from the scores k_sd_cv_score left for the group's 1 + ni fits
//     inner_mse[c] = (sum over the inner members j = 1 .. ni, ascending, of (sum_t sse_j[c][t], t ascending) / nte_j) / ni,
//                    c = 0 .. k -- the per-fit term of k_sd_cvp_reduce; row 0 the intercept-only model
//     best = 1; for c = 2 .. k: if inner_mse[c] < inner_mse[best] then best = c    (first minimum; a NaN is never smaller)
//     ncomp = best, or 0 where inner_mse[best] is not finite: the group is undefined and its scores are NaN
//     r[t], r2[t] = the outer member's at c = ncomp;  mse = (sum_t sse_0[ncomp][t]) / nte_0
// One wavefront per group: lanes over c for inner_mse (kept in the wave's slice of LDS, (k + 1) doubles), one lane
// selects, lanes over t copy.  No atomics, every sum in a fixed order.  nte = nullptr (the fits were scored by the
// identity variant, which does not write it): the usable test rows of a fit are counted here from its codes -- an
// integer, so the same double k_sd_cv_score<., true> sums.  out_inner: [groups][k + 1] or nullptr.
// grid ceil(groups / 4), dynamic LDS 4 (k + 1) doubles.  The three parts below are shared with k_sd_cvn_class_select.

// the usable test rows of fit f of the batch (wave-uniform)
__device__ __forceinline__ double sd_cvn_usable_tests(const double* __restrict__ nte, const uint8_t* __restrict__ codes,
                                                      const uint8_t* __restrict__ okx, const uint8_t* __restrict__ oky,
                                                      int S, int lane, size_t f)
{
    if (nte) return nte[f];
    const uint8_t* c = codes + f * S;
    int cnt = 0;
    for (int p = lane; p < S; p += 64) cnt += (c[p] == 0 && (!okx || okx[p]) && (!oky || oky[p])) ? 1 : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
    return (double)cnt;
}

// inner_mse[0 .. k] of group g into im (the wave's LDS slice) and, where asked for, out_inner
__device__ __forceinline__ void sd_cvn_inner_mse(const double* __restrict__ sse, const double* __restrict__ nte,
                                                 const uint8_t* __restrict__ codes, const uint8_t* __restrict__ okx,
                                                 const uint8_t* __restrict__ oky, int S, int k, int T, int ni, int g,
                                                 int lane, double* im, double* __restrict__ out_inner)
{
    const size_t fit0 = (size_t)g * (1 + ni);
    for (int c0 = 0; c0 <= k; c0 += 64) {
        const int c = c0 + lane;
        double acc = 0.0;
        for (int j = 1; j <= ni; ++j) {
            const double nj = sd_cvn_usable_tests(nte, codes, okx, oky, S, lane, fit0 + j);    // (wave-uniform)
            if (c <= k) {
                const double* row = sse + ((fit0 + j) * (k + 1) + c) * T;
                double s = 0.0;
                for (int t = 0; t < T; ++t) s += row[t];
                acc += s / nj;
            }
        }
        if (c <= k) {
            im[c] = acc / ni;
            if (out_inner) out_inner[(size_t)g * (k + 1) + c] = acc / ni;
        }
    }
}

// the outer member's scores at c = best, or NaN and ncomp = 0 for an undefined group; n0: its usable test rows
__device__ __forceinline__ void sd_cvn_copy(const double* __restrict__ r, const double* __restrict__ r2,
                                            const double* __restrict__ sse, int k, int T, int ni, int g, int lane, int best,
                                            bool defined, double n0, double* __restrict__ out_r, double* __restrict__ out_r2,
                                            double* __restrict__ out_mse, int* __restrict__ out_nc)
{
    const size_t fit0 = (size_t)g * (1 + ni), kT = (size_t)k * T;
    const double nan = __builtin_nan("");
    for (int t = lane; t < T; t += 64) {
        out_r[(size_t)g * T + t] = defined ? r[fit0 * kT + (size_t)(best - 1) * T + t] : nan;
        out_r2[(size_t)g * T + t] = defined ? r2[fit0 * kT + (size_t)(best - 1) * T + t] : nan;
    }
    if (lane == 0) {
        const double* row = sse + (fit0 * (k + 1) + best) * T;
        double s = 0.0;
        for (int t = 0; t < T; ++t) s += row[t];
        out_mse[g] = defined ? s / n0 : nan;
        out_nc[g] = defined ? best : 0;
    }
}

static __global__ __launch_bounds__(256)
void k_sd_cvn_select(const double* __restrict__ r, const double* __restrict__ r2, const double* __restrict__ sse,
                     const double* __restrict__ nte, const uint8_t* __restrict__ codes, const uint8_t* __restrict__ okx,
                     const uint8_t* __restrict__ oky, int S, int k, int T, int ni, int groups,
                     double* __restrict__ out_r, double* __restrict__ out_r2, double* __restrict__ out_mse,
                     int* __restrict__ out_nc, double* __restrict__ out_inner)
{
    extern __shared__ __attribute__((aligned(16))) double sm_cvn[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = blockIdx.x * 4 + wave;
    if (g >= groups) return;
    double* im = sm_cvn + (size_t)wave * (k + 1);
    sd_cvn_inner_mse(sse, nte, codes, okx, oky, S, k, T, ni, g, lane, im, out_inner);
    const double n0 = sd_cvn_usable_tests(nte, codes, okx, oky, S, lane, (size_t)g * (1 + ni));
    wave_sync();
    int best = 1;
    for (int c = 2; c <= k; ++c)
        if (im[c] < im[best]) best = c;
    const double vbest = im[best];
    const bool defined = vbest - vbest == 0.0;                                 // (finite: neither NaN nor an infinity)
    sd_cvn_copy(r, r2, sse, k, T, ni, g, lane, best, defined, n0, out_r, out_r2, out_mse, out_nc);
}

// The selection of a group on COUNTS (PLS-DA; plsx_simpls_cvn_class_begin), in place of k_sd_cvn_select: fconf
// [fits][k][G][G] int32 and, where AUC counts are asked for, fauc [fits][k][G][2] int64 are the blocks k_sd_cv_class /
// k_sd_cv_auc have just counted for every fit of the batch (block = fit), G = T.  Per group and c = 1 .. k
//     pooled[c]  = sum over the inner members j = 1 .. ni, ascending, of fconf_j[c]            (integers; out_iconf)
//     rule 1, accuracy:           crit[c] = trace(pooled[c]) / total(pooled[c])                (one division)
//     rule 2, balanced accuracy:  crit[c] = (0.0 + recall_0 + recall_1 + ...) / #classes, recall_g = pooled[g][g] / rowsum_g
//                                 over the classes with rowsum_g > 0 in ascending g, one by one
//     rule 0, mse:                k_sd_cvn_select's own rule on inner_mse (same helper, same bits)
//     best = 1; for c = 2 .. k: if crit[c] > crit[best] then best = c      (first maximum; a NaN never wins)
//     ncomp = best, or 0 where crit[best] is NaN -- the pooled block has no counted row: the group is undefined, its
//     scores are NaN and its counts zero
//     out_conf / out_auc = the OUTER member's block at c = ncomp; r, r2, mse, inner_mse as k_sd_cvn_select writes them.
// One wavefront per group; the pooled block of the open c, its row sums and its diagonal live in the wave's LDS slice;
// every lane forms the criterion from them in the same fixed order, lane 0 keeps it.  Integer sums and divisions only:
// no atomics, nothing to contract.  grid ceil(groups / 4), dynamic LDS 4 (2 (k + 1) doubles + (G G + 2 G) ints).
static __global__ __launch_bounds__(256)
void k_sd_cvn_class_select(const double* __restrict__ r, const double* __restrict__ r2, const double* __restrict__ sse,
                           const double* __restrict__ nte, const uint8_t* __restrict__ codes,
                           const uint8_t* __restrict__ okx, const uint8_t* __restrict__ oky, int S, int k, int T, int ni,
                           int groups, int rule, const int* __restrict__ fconf, const long long* __restrict__ fauc,
                           double* __restrict__ out_r, double* __restrict__ out_r2, double* __restrict__ out_mse,
                           int* __restrict__ out_nc, double* __restrict__ out_inner, int* __restrict__ out_conf,
                           long long* __restrict__ out_auc, int* __restrict__ out_iconf)
{
    extern __shared__ __attribute__((aligned(16))) double sm_cvn[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = blockIdx.x * 4 + wave;
    if (g >= groups) return;
    const int G = T, GG = G * G;
    double* im = sm_cvn + (size_t)wave * 2 * (k + 1);
    double* cr = im + (k + 1);
    int* pool = reinterpret_cast<int*>(sm_cvn + (size_t)8 * (k + 1)) + (size_t)wave * (GG + 2 * G);
    int* rows = pool + GG;
    int* diag = rows + G;
    const size_t fit0 = (size_t)g * (1 + ni);
    sd_cvn_inner_mse(sse, nte, codes, okx, oky, S, k, T, ni, g, lane, im, out_inner);
    const double n0 = sd_cvn_usable_tests(nte, codes, okx, oky, S, lane, fit0);
    if (rule != 0 || out_iconf)
        for (int c = 1; c <= k; ++c) {
            for (int i = lane; i < GG; i += 64) {
                int v = 0;
                for (int j = 1; j <= ni; ++j) v += fconf[((fit0 + j) * k + (c - 1)) * GG + i];
                pool[i] = v;
                if (out_iconf) out_iconf[((size_t)g * k + (c - 1)) * GG + i] = v;
            }
            wave_sync();
            for (int a = lane; a < G; a += 64) {
                int s = 0;
                for (int b = 0; b < G; ++b) s += pool[a * G + b];
                rows[a] = s;
                diag[a] = pool[a * G + a];
            }
            wave_sync();
            double crit;
            if (rule == 1) {
                int trace = 0, total = 0;
                for (int a = 0; a < G; ++a) { trace += diag[a]; total += rows[a]; }
                crit = (double)trace / (double)total;
            } else {
                double sum = 0.0;
                int present = 0;
                for (int a = 0; a < G; ++a)
                    if (rows[a] > 0) { sum += (double)diag[a] / (double)rows[a]; ++present; }
                crit = sum / (double)present;
            }
            if (lane == 0) cr[c] = crit;
            wave_sync();                                                       // (this c's reads before the next c's writes)
        }
    wave_sync();
    int best = 1;
    bool defined;
    if (rule == 0) {
        for (int c = 2; c <= k; ++c)
            if (im[c] < im[best]) best = c;
        const double vbest = im[best];
        defined = vbest - vbest == 0.0;                                        // (finite: neither NaN nor an infinity)
    } else {
        for (int c = 2; c <= k; ++c)
            if (cr[c] > cr[best]) best = c;
        const double vbest = cr[best];
        defined = vbest == vbest;                                              // (NaN: no counted row in the pooled block)
    }
    sd_cvn_copy(r, r2, sse, k, T, ni, g, lane, best, defined, n0, out_r, out_r2, out_mse, out_nc);
    for (int i = lane; i < GG; i += 64)
        out_conf[(size_t)g * GG + i] = defined ? fconf[(fit0 * k + (best - 1)) * GG + i] : 0;
    if (out_auc)
        for (int i = lane; i < 2 * G; i += 64)
            out_auc[(size_t)g * 2 * G + i] = defined ? fauc[(fit0 * k + (best - 1)) * 2 * G + i] : 0;
}

// ... and the reduction over the outer splits, after the selection: out_r / out_r2 [.][T], out_mse [.] of permutation pi
// take the selected scores of its groups in this batch, added ONE BY ONE IN SPLIT ORDER to what the earlier batches left
// there (the entry starts from zero) and divided by n once the last split is in -- the device of k_sd_cvp_reduce: the
// same bits wherever a batch ends.  out_cnt [.][k] int32: how many of the permutation's splits chose c = 1 .. k (an
// undefined group counts nowhere).  One thread per output entry, no atomics.  g0: the batch's first group, mg of them.
// grid (ceil(E / 256), perms touched), E = 2 T + 1 + k.
static __global__ __launch_bounds__(256)
void k_sd_cvn_reduce(const double* __restrict__ r, const double* __restrict__ r2, const double* __restrict__ mse,
                     const int* __restrict__ nc, int k, int T, int n, long long g0, int mg,
                     double* __restrict__ out_r, double* __restrict__ out_r2, double* __restrict__ out_mse,
                     int* __restrict__ out_cnt)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * T + 1 + k) return;
    const long long pi = g0 / n + blockIdx.y;
    const long long lo = pi * n > g0 ? pi * n : g0, end = (pi + 1) * n < g0 + mg ? (pi + 1) * n : g0 + mg;
    const bool last = end == (pi + 1) * n;
    if (e <= 2 * T) {
        const double* src = e < T ? r + e : (e < 2 * T ? r2 + (e - T) : mse);
        const int stride = e < 2 * T ? T : 1;
        double* dst = e < T ? out_r + (size_t)pi * T + e : (e < 2 * T ? out_r2 + (size_t)pi * T + (e - T) : out_mse + pi);
        double acc = *dst;
        for (long long g = lo; g < end; ++g) acc += src[(size_t)(g - g0) * stride];
        *dst = last ? acc / n : acc;
    } else {
        const int c = e - 2 * T;                                               // 1 .. k
        int* dst = out_cnt + (size_t)pi * k + (c - 1);
        int acc = *dst;
        for (long long g = lo; g < end; ++g) acc += nc[g - g0] == c ? 1 : 0;
        *dst = acc;
    }
}

// ... and of the selected counts of k_sd_cvn_class_select next to it: out_conf [.][G][G] int32 and out_auc [.][G][2]
// int64 (or nullptr) of permutation pi take the blocks of its groups in this batch, added to what the earlier batches
// left there (the entry starts from zero).  Integers: the same result wherever a batch ends.  One thread per entry, no
// atomics.  grid (ceil(E / 256), perms touched), E = G G + 2 G.
static __global__ __launch_bounds__(256)
void k_sd_cvn_class_reduce(const int* __restrict__ conf, const long long* __restrict__ auc, int G, int n, long long g0,
                           int mg, int* __restrict__ out_conf, long long* __restrict__ out_auc)
{
    const int GG = G * G, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= GG + 2 * G) return;
    const long long pi = g0 / n + blockIdx.y;
    const long long lo = pi * n > g0 ? pi * n : g0, end = (pi + 1) * n < g0 + mg ? (pi + 1) * n : g0 + mg;
    if (e < GG) {
        int* dst = out_conf + (size_t)pi * GG + e;
        int acc = *dst;
        for (long long g = lo; g < end; ++g) acc += conf[(size_t)(g - g0) * GG + e];
        *dst = acc;
    } else if (out_auc) {
        const int i = e - GG;
        long long* dst = out_auc + (size_t)pi * 2 * G + i;
        long long acc = *dst;
        for (long long g = lo; g < end; ++g) acc += auc[(size_t)(g - g0) * 2 * G + i];
        *dst = acc;
    }
}

// Split-half reliability of the SIMPLS components (plsx_simpls_split_half_batch), after the solver ran on ALL usable
// rows of an arrangement (X, Y[ysrc]).  With t_c the scores (XW, which carries them plus a constant), q_c = Y0^T t_c the
// y-loadings, K = Xc Xc^T and r = Xc 1_B of the bound data, a split into halves H1 / H2 of the usable positions gives
//     g_{h,c}[p] = sum_t (Y[ys_p][t] - ybar_h[t]) q_c[t] = yq_c[p] - mean_{H_h} yq_c     on H_h, 0 elsewhere,
//                  yq_c[p] = sum_t Y0[t][p] q_c[t]        (the centring of the fit drops out with the half mean)
//     D_h^T q_c  = Xc^T g_{h,c}                            (B-long: never formed)
//     ucorr[c]   = corr_f(D_1^T q_c, D_2^T q_c)            from g1^T K g2, g1^T K g1, g2^T K g2 and g_h^T r:
//                  sum_f u1 u2 - (sum_f u1)(sum_f u2) / B = g1^T K g2 - (g1^T r)(g2^T r) / B
//     D_h w_c    = sum_{p in H_h} Y0[.][p] (t_c[p] - mean_{H_h} t_c)                  (T-long)
//     vcorr[c]   = corr_t(D_1 w_c, D_2 w_c)
// -- compute.efficient_corr of both pairs, clipped to [-1, 1]; a side without variance gives the NaN numpy gives.  A
// position is usable iff the solver kept it (xs >= 0: okx[p] and oky[ys_p]); unusable rows belong to neither half.
struct ShArgs {
    int S, T, k, B;
    int nres;                   // arrangements of the solver batch
    int ns, s0, nsg;            // splits per arrangement; first split and number of splits of this group
    long long a0;               // the batch's first arrangement in the call's list
    const int* xs;              // [nres][S] solver state
    const double* Y0;           // [nres][T][S]
    const double* XW;           // [nres][k][S]
    const uint8_t* masks;       // (np, ns, S) 1 = first half
    const double* rsum;         // [S] row sums of Xc over the B features
    double* q;                  // [nres][k][T]
    double* yq;                 // [nres][k][S]
    double* G;                  // [nres nsg][k][2][S] half vectors g_{1,c}, g_{2,c}
    const double* KG;           // [nres nsg][k][2][S] their products with K
    double* ucorr;              // (np, ns, k)
    double* vcorr;
};

// r = Xc 1_B: one wavefront per row, fixed order.
static __global__ __launch_bounds__(256)
void k_row_sum(const double* __restrict__ Xc, int ldx, int S, int B, double* __restrict__ out)
{
    const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= S) return;
    const double* row = Xc + (size_t)p * ldx;
    double s = 0.0;
    for (int f = lane; f < B; f += 64) s += row[f];
    s = wave_sum(s);
    if (lane == 0) out[p] = s;
}

// q_c = Y0^T XW_c (Y0 sums to zero over the usable positions and is zero elsewhere: the constant XW carries drops
// out) and yq_c = Y0 q_c of one arrangement.  One wavefront per arrangement, four components per reduction.
static __global__ __launch_bounds__(256)
void k_sd_sh_prep(ShArgs a)
{
    const int S = a.S, T = a.T, k = a.k, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = blockIdx.x * (blockDim.x >> 6) + wave;
    if (r >= a.nres) return;
    const double* Y0 = a.Y0 + (size_t)r * S * T;
    const double* XW = a.XW + (size_t)r * k * S;
    double* q = a.q + (size_t)r * k * T;
    double* yq = a.yq + (size_t)r * k * S;
    for (int t = 0; t < T; ++t) {
        const double* y0t = Y0 + (size_t)t * S;
        for (int c0 = 0; c0 < k; c0 += 4) {
            const double *w0 = XW + (size_t)min(c0, k - 1) * S, *w1 = XW + (size_t)min(c0 + 1, k - 1) * S,
                         *w2 = XW + (size_t)min(c0 + 2, k - 1) * S, *w3 = XW + (size_t)min(c0 + 3, k - 1) * S;
            double s4[4] = {0.0, 0.0, 0.0, 0.0};
            for (int p = lane; p < S; p += 64) {
                const double y = y0t[p];
                s4[0] += y * w0[p]; s4[1] += y * w1[p]; s4[2] += y * w2[p]; s4[3] += y * w3[p];
            }
            wave_sum4(s4[0], s4[1], s4[2], s4[3]);
            if (lane == 0)
                for (int u = 0; u < 4 && c0 + u < k; ++u) q[(size_t)(c0 + u) * T + t] = s4[u];
        }
    }
    wave_global_sync();                        // q, as lane 0 wrote it
    for (int c = 0; c < k; ++c) {
        const double* qc = q + (size_t)c * T;
        for (int p = lane; p < S; p += 64) {
            double s = 0.0;
            for (int t = 0; t < T; ++t) s += Y0[(size_t)t * S + p] * qc[t];
            yq[(size_t)c * S + p] = s;
        }
    }
}

// The half vectors of one (arrangement, split): G[c][h][p] = yq_c[p] - mean_{H_h} yq_c on H_h, zero elsewhere (every
// entry written).  One wavefront per (arrangement, split) of the group, two components per reduction.
static __global__ __launch_bounds__(256)
void k_sd_sh_expand(ShArgs a)
{
    const int S = a.S, k = a.k, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long w = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
    if (w >= (long long)a.nres * a.nsg) return;
    const int r = (int)(w / a.nsg), s = (int)(w % a.nsg);
    const int* xs = a.xs + (size_t)r * S;
    const uint8_t* m = a.masks + ((size_t)(a.a0 + r) * a.ns + a.s0 + s) * S;
    const double* yq = a.yq + (size_t)r * k * S;
    double* G = a.G + (size_t)w * k * 2 * S;
    double c1 = 0.0, c2 = 0.0;
    for (int p = lane; p < S; p += 64) {
        const bool ok = xs[p] >= 0;
        c1 += (ok && m[p]) ? 1.0 : 0.0;
        c2 += (ok && !m[p]) ? 1.0 : 0.0;
    }
    const double n1 = wave_sum(c1), n2 = wave_sum(c2);
    for (int c0 = 0; c0 < k; c0 += 2) {
        const int cb = min(c0 + 1, k - 1);
        const double *ya = yq + (size_t)c0 * S, *yb = yq + (size_t)cb * S;
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int p = lane; p < S; p += 64) {
            const bool ok = xs[p] >= 0, h1 = ok && m[p], h2 = ok && !m[p];
            const double va = ya[p], vb = yb[p];
            s4[0] += h1 ? va : 0.0; s4[1] += h2 ? va : 0.0; s4[2] += h1 ? vb : 0.0; s4[3] += h2 ? vb : 0.0;
        }
        wave_sum4(s4[0], s4[1], s4[2], s4[3]);
        const double ma1 = s4[0] / n1, ma2 = s4[1] / n2, mb1 = s4[2] / n1, mb2 = s4[3] / n2;
        double* ga = G + (size_t)c0 * 2 * S;
        double* gb = G + (size_t)cb * 2 * S;
        for (int p = lane; p < S; p += 64) {
            const bool ok = xs[p] >= 0, h1 = ok && m[p], h2 = ok && !m[p];
            const double va = ya[p], vb = yb[p];
            ga[p] = h1 ? va - ma1 : 0.0;
            ga[S + p] = h2 ? va - ma2 : 0.0;
            if (cb != c0) {
                gb[p] = h1 ? vb - mb1 : 0.0;
                gb[S + p] = h2 ? vb - mb2 : 0.0;
            }
        }
    }
}

// ucorr and vcorr of one (arrangement, split) from G, KG = G . K, r and the fit's Y0 / XW.  One wavefront per
// (arrangement, split); reductions are wave_sum / wave_sum4 in fixed order, no atomics, no LDS.  The T-vectors D_h w_c
// are formed twice (their means over t first, then the centred sums): T S flop per half and component, nothing kept.
static __global__ __launch_bounds__(256)
void k_sd_sh_score(ShArgs a)
{
    const int S = a.S, T = a.T, k = a.k, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long w = (long long)blockIdx.x * (blockDim.x >> 6) + wave;
    if (w >= (long long)a.nres * a.nsg) return;
    const int r = (int)(w / a.nsg), s = (int)(w % a.nsg);
    const int* xs = a.xs + (size_t)r * S;
    const uint8_t* m = a.masks + ((size_t)(a.a0 + r) * a.ns + a.s0 + s) * S;
    const double* Y0 = a.Y0 + (size_t)r * S * T;
    const double* XW = a.XW + (size_t)r * k * S;
    const double* G = a.G + (size_t)w * k * 2 * S;
    const double* KG = a.KG + (size_t)w * k * 2 * S;
    double* out_u = a.ucorr + ((size_t)(a.a0 + r) * a.ns + a.s0 + s) * k;
    double* out_v = a.vcorr + ((size_t)(a.a0 + r) * a.ns + a.s0 + s) * k;
    const double nB = (double)a.B;
    auto clip = [](double v) { return v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v); };      // (NaN stays NaN)
    double c1 = 0.0, c2 = 0.0;
    for (int p = lane; p < S; p += 64) {
        const bool ok = xs[p] >= 0;
        c1 += (ok && m[p]) ? 1.0 : 0.0;
        c2 += (ok && !m[p]) ? 1.0 : 0.0;
    }
    const double n1 = wave_sum(c1), n2 = wave_sum(c2);
    for (int c = 0; c < k; ++c) {
        const double *g1 = G + (size_t)c * 2 * S, *g2 = g1 + S, *k1 = KG + (size_t)c * 2 * S, *k2 = k1 + S;
        double s11 = 0.0, s22 = 0.0, s12 = 0.0, r1 = 0.0, r2 = 0.0;
        for (int p = lane; p < S; p += 64) {
            const double u = g1[p], v = g2[p], rs = a.rsum[p];
            s11 += u * k1[p]; s22 += v * k2[p]; s12 += u * k2[p];
            r1 += u * rs; r2 += v * rs;
        }
        wave_sum4(s11, s22, s12, r1);
        r2 = wave_sum(r2);
        const double v11 = s11 - r1 * r1 / nB, v22 = s22 - r2 * r2 / nB, v12 = s12 - r1 * r2 / nB;
        if (lane == 0) out_u[c] = clip(v12 / sqrt(v11 * v22));
        // the scores' half means, then D_h w_c[t] = sum_{p in H_h} Y0[t][p] (t_c[p] - mean_h)
        const double* xw = XW + (size_t)c * S;
        double x1 = 0.0, x2 = 0.0;
        for (int p = lane; p < S; p += 64) {
            const bool ok = xs[p] >= 0;
            const double x = xw[p];
            x1 += (ok && m[p]) ? x : 0.0;
            x2 += (ok && !m[p]) ? x : 0.0;
        }
        const double mx1 = wave_sum(x1) / n1, mx2 = wave_sum(x2) / n2;
        auto dw = [&](int t, double& d1, double& d2) {
            const double* y0t = Y0 + (size_t)t * S;
            double e1 = 0.0, e2 = 0.0;
            for (int p = lane; p < S; p += 64) {
                const bool ok = xs[p] >= 0;
                const double y = y0t[p], x = xw[p];
                e1 += (ok && m[p]) ? y * (x - mx1) : 0.0;
                e2 += (ok && !m[p]) ? y * (x - mx2) : 0.0;
            }
            d1 = wave_sum(e1); d2 = wave_sum(e2);
        };
        double sa1 = 0.0, sa2 = 0.0;
        for (int t = 0; t < T; ++t) {
            double d1, d2;
            dw(t, d1, d2);
            sa1 += d1; sa2 += d2;
        }
        const double m1 = sa1 / T, m2 = sa2 / T;
        double q11 = 0.0, q22 = 0.0, q12 = 0.0;
        for (int t = 0; t < T; ++t) {
            double d1, d2;
            dw(t, d1, d2);
            d1 -= m1; d2 -= m2;
            q11 += d1 * d1; q22 += d2 * d2; q12 += d1 * d2;
        }
        if (lane == 0) out_v[c] = clip(q12 / sqrt(q11 * q22));
    }
}

// Coefficients of the c-component model of one bootstrap (plsx_simpls_coef_begin), after the solver chain of its batch.
// With wd_j the dual weights (position space, centred over the included positions) and t_j the unit-norm scores,
//     q_j = (Y_r - ybar_r)^T t_j = sum_p Y0[.][p] XW[j][p]      simpls y_loadings (Y0 sums to zero over the included
//                                                               positions and is zero elsewhere: the mean XW carries drops out)
//     beta_c = W[:, :c] Q[:, :c]^T = Xc^T A,   A[t] = scatter(sum_{j < c} q_j[t] wd_j)   (T rows in subject space)
// -- a product of t_j and wd_j, so the signs of the components cancel and no alignment is needed.  The T x c products
// q go through the matrix pipe where they fit two tiles each way (wave_mfma_nt, as k_sd_final's y-loadings), otherwise
// four at a time through wave_sum4; both in fixed order.  The scatter is sd_scatter / sd_scatter_g: a subject drawn
// more than once receives bit-identical addends.  One wavefront per resample; dynamic LDS per wave: cf_c doubles (the
// q_j[t] of the row being written) + S (the scatter buffer; GL: none).
template <int RC, bool GL>
static __global__ __launch_bounds__(256)
void k_sd_coef(SdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double sm_sd[];
    const int S = a.S, T = a.T, k = a.k, cc = a.cf_c, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: scalar pointers
    const int rl = blockIdx.x * (blockDim.x >> 6) + wave;
    if (rl >= a.cf_n) return;
    const int r = a.cf_r0 + rl;
    double* qt = sm_sd + (size_t)wave * (GL ? cc : cc + S);      // [cc] q_j[t] of the open row + [S] scatter buffer
    const int* xs = a.xs + (size_t)r * S;
    const double* Y0 = a.Y0 + (size_t)r * S * T;
    const double* XW = a.XW + (size_t)r * k * S;
    const double* WD = a.WD + (size_t)r * k * S;
    double* q = a.cfq + (size_t)rl * cc * T;
    double* A = a.cfA + (size_t)rl * T * S;
    auto rows = [&](const double* M, int nrows) {
        return [=](int t, int p, double (&v)[4]) {
            const double* src = M + (size_t)min(t, nrows - 1) * S;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double x = src[min(p + j, S - 1)];
                v[j] = (t < nrows && p + j < S) ? x : 0.0;
            }
        };
    };
    const int tt = (T + 15) >> 4, kt = (cc + 15) >> 4;
#define SD_CQ(MTL, NTL) {                                                                                          \
        d4 acc[MTL][NTL];                                                                                          \
        _Pragma("unroll") for (int i_ = 0; i_ < MTL; ++i_)                                                         \
            _Pragma("unroll") for (int j_ = 0; j_ < NTL; ++j_) acc[i_][j_] = (d4){0.0, 0.0, 0.0, 0.0};            \
        wave_mfma_nt<MTL, NTL>(acc, S, lane, rows(Y0, T), rows(XW, cc));                                           \
        _Pragma("unroll") for (int mt = 0; mt < MTL; ++mt)                                                         \
            _Pragma("unroll") for (int nt = 0; nt < NTL; ++nt)                                                     \
                _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                    \
                    const int t = mt * 16 + (lane >> 4) + 4 * i, c = nt * 16 + (lane & 15);                        \
                    if (t < T && c < cc) q[(size_t)c * T + t] = acc[mt][nt][i];                                    \
                }                                                                                                  \
    }
    if (tt == 1 && kt == 1) SD_CQ(1, 1)
    else if (tt == 2 && kt == 1) SD_CQ(2, 1)
    else if (tt <= 2 && kt <= 2) SD_CQ(2, 2)
    else {
        for (int t = 0; t < T; ++t) {
            const double* y0t = Y0 + (size_t)t * S;
            for (int c0 = 0; c0 < cc; c0 += 4) {
                const double *w0 = XW + (size_t)min(c0, cc - 1) * S, *w1 = XW + (size_t)min(c0 + 1, cc - 1) * S,
                             *w2 = XW + (size_t)min(c0 + 2, cc - 1) * S, *w3 = XW + (size_t)min(c0 + 3, cc - 1) * S;
                double s4[4] = {0.0, 0.0, 0.0, 0.0};
                for (int p0 = 0; p0 < S; p0 += SD_TILE) {
                    SD_TILE_PC(pc, p0);
                    SD_OWN(i) {
                        const double yv = y0t[pc[i]], y = SD_IN(p0, i) ? yv : 0.0;
                        s4[0] += y * w0[pc[i]]; s4[1] += y * w1[pc[i]]; s4[2] += y * w2[pc[i]]; s4[3] += y * w3[pc[i]];
                    }
                }
                wave_sum4(s4[0], s4[1], s4[2], s4[3]);
                if (lane == 0)
                    for (int u = 0; u < 4 && c0 + u < cc; ++u) q[(size_t)(c0 + u) * T + t] = s4[u];
            }
        }
    }
#undef SD_CQ
    wave_global_sync();                        // q, as the other lanes wrote it
    for (int t = 0; t < T; ++t) {
        for (int j = lane; j < cc; j += 64) qt[j] = q[(size_t)j * T + t];
        wave_sync();
        auto value = [&](int p) {
            double s = 0.0;
            for (int j = 0; j < cc; ++j) s += qt[j] * WD[(size_t)j * S + p];
            return s;
        };
        if constexpr (GL)
            sd_scatter_g(a.sfirst + (size_t)r * S, a.scnt + (size_t)r * S, S, lane, A + (size_t)t * S, value);
        else
            sd_scatter(qt + cc, xs, S, lane, A + (size_t)t * S, value);
        wave_sync();
    }
}

// VIP stack of one bootstrap (plsx_simpls_vip_keep), after the solver chain of its batch.  With wd_a the dual weights
// (position space, centred over the included positions, zero elsewhere), w_a = X0_r^T wd_a = Xc^T scatter(wd_a) the
// x_weights and t_a = X0_r w_a = K_r wd_a the unit-norm scores,
//     |w_a|^2 = wd_a^T K_r wd_a = a_a^T K a_a = sum_p WD[a][p] XW[a][p]     (a_a = scatter(wd_a); XW = t_a plus a constant,
//                                                                          which the centred wd_a does not see)
//     ssq_a   = |q_a|^2 = |Y0^T t_a|^2 = pctvar[a] . sum Y0^2               (k_sd_step left it; the common factor
//                                                                          sum Y0^2 cancels in ssq_a / sum_j ssq_j)
//     G[a]    = sqrt(ssq_a / (|w_a|^2 sum_{j < c} ssq_j)) . a_a,    VIP[f]^2 = B sum_a (Xc[:, f]^T G[a])^2
// -- the quadratic form with K costs 2 S flop per component here because the solver already holds K_r wd_a; no pass over
// K, no product.  Squares of w_a and q_a: the signs and the order of the components do not matter, no alignment.  A
// model without explained variance or a component of zero weight norm gives 0 / 0 = NaN rows, as numpy's formula
// does.  Reductions are wave_sum in fixed order; the scatter is sd_scatter / sd_scatter_g (a subject drawn more than
// once receives bit-identical addends, both routes write the same bits).  One wavefront per resample; dynamic LDS per
// wave: S doubles (the scatter buffer; GL: none).
template <bool GL>
static __global__ __launch_bounds__(256)
void k_sd_vip(SdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double sm_sd[];
    const int S = a.S, k = a.k, cc = a.vp_c, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: scalar pointers
    const int r = blockIdx.x * (blockDim.x >> 6) + wave;
    if (r >= a.nres) return;
    const int* xs = a.xs + (size_t)r * S;
    const double* XW = a.XW + (size_t)r * k * S;
    const double* WD = a.WD + (size_t)r * k * S;
    const double* pv = a.pctvar + (size_t)r * k;
    double* G = a.vpG + (size_t)r * cc * S;
    double tot = 0.0;
    for (int j = 0; j < cc; ++j) tot += pv[j];
    for (int j = 0; j < cc; ++j) {
        const double* wd = WD + (size_t)j * S;
        const double* xw = XW + (size_t)j * S;
        double s = 0.0;
        for (int p = lane; p < S; p += 64) s += (xs[p] >= 0) ? wd[p] * xw[p] : 0.0;
        const double f = sqrt(pv[j] / (wave_sum(s) * tot));
        auto value = [&](int p) { return f * wd[p]; };
        if constexpr (GL)
            sd_scatter_g(a.sfirst + (size_t)r * S, a.scnt + (size_t)r * S, S, lane, G + (size_t)j * S, value);
        else
            sd_scatter(sm_sd + (size_t)wave * S, xs, S, lane, G + (size_t)j * S, value);
    }
}

// Bootstrap sign alignment (regression.py:317-320): flip_c = sign(corr(w_c, w0_c))
// = sign(sum_b w_c[b] * (w0_c[b] - mean w0_c)); P[r][c][c'] = W_r[c] . W0c[c'].
// Writes M = diag(flip) in k_urot's fragment order and flips the y_loadings.
static __global__ void k_simpls_signs(const double* __restrict__ P, int k, int T, int nks_t, int LT,
                               double* __restrict__ Mfrag, double* __restrict__ yload)
{
    const int r = blockIdx.x;
    const int tot = nks_t * LT * 64;
    for (int idx = threadIdx.x; idx < tot; idx += blockDim.x) {
        const int lane = idx & 63, lt = (idx >> 6) % LT, ks = (idx >> 6) / LT;
        const int t = ks * 4 + (lane >> 4), l = lt * 16 + (lane & 15);
        double v = 0.0;
        if (t < k && l < k && t == l) {
            const double d = P[((size_t)r * k + t) * k + t];
            v = (d > 0.0) ? 1.0 : ((d < 0.0) ? -1.0 : 0.0);
        }
        Mfrag[(size_t)r * tot + idx] = v;
    }
    for (int idx = threadIdx.x; idx < T * k; idx += blockDim.x) {
        const int c = idx % k;
        const double d = P[((size_t)r * k + c) * k + c];
        const double f = (d > 0.0) ? 1.0 : ((d < 0.0) ? -1.0 : 0.0);
        yload[(size_t)r * T * k + idx] *= f;
    }
}
