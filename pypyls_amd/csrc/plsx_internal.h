// plsx_internal.h -- what the translation units of libplsx.so share: the context, error / launch macros,
// small host helpers and the prototypes of the launch layers.  Nothing here is part of the C ABI (include/plsx.h).
//
// Translation units (compiled in parallel by pypyls_amd/_build.py, one code object each):
//   plsx_core.hip        context, plsx_set_data, plsx_set_contrasts, options, timing, permutations, PLS-C bootstraps, finishing, generators
//   plsx_xprod.hip       k_xprod launches (dense blocks, moment blocks, accumulating / quadratic-form epilogues), the row normalisation of multiblock PLS
//   plsx_compact.hip     k_xprod_compact launches (one bootstrap / split per block)
//   plsx_gram.hip        k_nt_gemm, k_dual_gp, k_gram4, k_gram, k_gram_lds
//   plsx_small.hip       k_small, k_refine_gram, k_rotate_rows; plsx_smallql{1,2}.hip: k_small_ql (plsx_smallql.h)
//   plsx_urot.hip        k_urot, k_ucorr_partial
//   plsx_split.hip       split-half and cross-validation
//   plsx_simpls_api.hip  SIMPLS regression: the solver batch (run_simpls_dual on an SdRequest), products with K (sd_times_K), one cross-validation body (cv_fit_score), the count series of PLS-DA (CountSeries)
//   plsx_cvperm.hip      permutation null of the behavioural cross-validation in dual space: plsx_crossval_perm_batch (plsx_k_cvperm.h)
//   plsx_weightsci.hip   percentile intervals of the PLS-C x_weights: plsx_boot_keep, plsx_boot_weights_ci
//   plsx_permweights.hip permutation test of the PLS-C x_weights: plsx_perm_weights_build, plsx_perm_weights_test (plsx_k_permweights.h)
//   plsx_confound.hip    confound regression of the SIMPLS front end: plsx_simpls_set_confounds, the fold-wise K_s and Y_s of its cross-validation (plsx_k_confound.h)
//   plsx_confound_behav.hip  confound regression of the PLS-C front end: plsx_residualize, plsx_set_confounds, the fold copies X_s of its cross-validation (plsx_k_confound_behav.h)
//   plsx_comm.hip        the exported collective (RCCL through dlopen)
#pragma once
#include "plsx_kernels.h"
#include <chrono>
#include "../../include/plsx.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

struct Buf {
    void* p = nullptr;
    size_t bytes = 0;
};

// Route / layout switches (plsx_set_option).  Every route computes the same statistics -- they exist for A/B
// measurements and so that the tests can pin each kernel variant against the others and the oracle.  None is
// read from the environment: a host that wants PLSX_<NAME>=1 to mean something translates it itself
// (pypyls_amd.engine.options_from_env, used by bench.py and the tests only).
enum {
    OPT_NO_REFINE = 0, OPT_MIN_BATCH, OPT_INBLOCK_MOMENTS, OPT_NO_COMPACT_BOOT, OPT_COMPACT_BOOT_ALWAYS,
    OPT_SEPMOM_ALWAYS, OPT_NO_GRAM4, OPT_UROT_GENERIC, OPT_UROT_NO_TAIL4, OPT_NO_FIXED_X, OPT_NO_DUAL_PERM,
    OPT_TWO_PASS_BOOT, OPT_SPLIT_INBLOCK, OPT_NO_SPLIT_FUSE, OPT_SPLIT_TWO_READERS, OPT_EXPECT_RESAMPLES,
    OPT_SIMPLS_JACOBI, OPT_PERCENTILE_SORT, OPT_QUAD_SUMS, OPT_SPLIT_READER8, OPT_SIMPLS_GLOBAL,
    OPT_CROSSCOV_SPARSE, OPT_NO_MOMENT_ROWS, OPT_NO_PERM_PROJECT, OPT_NO_COMPACT_WIDE, OPT_COMPACT_WIDE_ALWAYS, OPT_COUNT
};
static const char* const kOptionNames[OPT_COUNT] = {
    "no_refine", "min_batch", "inblock_moments", "no_compact_boot", "compact_boot_always",
    "sepmom_always", "no_gram4", "urot_generic", "urot_no_tail4", "no_fixed_x", "no_dual_perm",
    "two_pass_boot", "split_inblock", "no_split_fuse", "split_two_readers", "expect_resamples",
    "simpls_jacobi", "percentile_sort", "quad_sums", "split_reader8", "simpls_global",
    "crosscov_sparse", "no_moment_rows", "no_perm_project", "no_compact_wide", "compact_wide_always"};

// k-steps per LDS stage of the 4-tile compact cross-product blocks (T' = 49 .. 64: the headline shape).  A/B lever of
// tools/ckt_probe.sh (measured: profiles/r06_compact_kt.txt); other tile counts keep 12 / MT.
#ifndef PLSX_CKT
#define PLSX_CKT 3
#endif
// ... and of the same blocks with four column tiles per wave (compact_boot_wide; measured:
// profiles/compact_wide_compare.txt)
#ifndef PLSX_CKTW
#define PLSX_CKTW 2
#endif

// A series of count blocks that rides along plsx_simpls_crossval_batch / plsx_simpls_crossval_perm_batch, appended to the
// caller's buffer: one block per split or permutation (plsx_simpls_api.hip: count_begin, count_reserve, count_launch).
struct CountSeries {
    const char* what;                                   // what a block counts, in the refusal of a call that does not fit
    const char* entry;                                  // the entry that opens the series, in that refusal and its own
    int active = 0;
    char* base = nullptr;                               // the caller's buffer
    long long cap = 0, n = 0;                           // blocks it holds / blocks appended
    size_t blk_bytes = 0;                               // bytes of one block (fixed when the series opens)
};
// an open series of counts ends (plsx_set_data, plsx_simpls_set_classes, a second _begin, its _end); the buffer stays
// the caller's
inline void count_close(CountSeries& s)
{
    s.active = 0; s.base = nullptr; s.cap = 0; s.n = 0;
}

// The series of out-of-fold predictions that rides along plsx_simpls_crossval_batch, plsx_simpls_crossval_confound_batch
// and the outer fits of plsx_simpls_crossval_nested_batch (plsx_simpls_cv_pred_begin; plsx_simpls_api.hip: pred_reserve,
// pred_launch): one slot [T][S] per observed fit, appended to the caller's stack.
struct PredSeries {
    int active = 0;
    int c = 0;                                          // the component count of every slot; 0: the nested selection's
    int* ncomp = nullptr;                               // the caller's [cap] int32 of the counts used, or nullptr
    double* pred = nullptr;                             // the caller's stack [cap][T][S]
    double* ytrue = nullptr;                            // ... and that of the observed values, or nullptr
    long long cap = 0, n = 0;                           // slots it holds / slots appended
};
inline void pred_close(PredSeries& s) { s = PredSeries(); }

// The counts of the nested cross-validation of PLS-DA (plsx_simpls_cvn_class_begin; plsx_simpls_api.hip: cvn_entry): the
// per-fit blocks of k_sd_cv_class / k_sd_cv_auc stay in the batch's scratch, the selection (k_sd_cvn_class_select) keeps
// the outer member's block at the selected component count -- one block [G][G] int32 (and [G][2] int64) per outer split
// of plsx_simpls_crossval_nested_batch, per permutation (summed over its outer splits) of the permuted entry, appended
// to the caller's buffers.
struct NestedCounts {
    int active = 0;
    int rule = 0;                                       // PLSX_CVN_SELECT_*: what the selection maximises (mse: minimises)
    int* conf = nullptr;                                // the caller's [cap][G][G] int32
    long long* auc = nullptr;                           // ... [cap][G][2] int64, or nullptr: no AUC counts
    int* inner = nullptr;                               // ... [cap][k][G][G] int32 pooled inner counts (observed entry), or nullptr
    long long cap = 0, n = 0;                           // blocks they hold / blocks appended
};
inline void ncls_close(NestedCounts& s) { s = NestedCounts(); }

struct plsx_ctx {
    int device = 0;
    std::string err;
    int opt[OPT_COUNT] = {};
    bool has_data = false, has_orig = false;
    // problem
    int method = 0, S = 0, B = 0, T = 0, J = 0, n_groups = 0, n_cond = 1, mc = 0, cov = 0;
    int Tp = 0, Tpp = 0, L = 0, Kpad = 0, nks = 0, Bx = 0, Bpad = 0;
    // plan.  momrows: the group carries per-cell moment rows (feature mean / std of the
    // resampled rows come out of the same pass); scaled: the epilogue also applies 1/std
    // to R (correlation mode).  Covariance mode keeps the rows for cross-validation's zmap.
    int MT = 24, npg = 0, w0 = 0, sq0 = 0, nmom_pad = 0, scaled = 0, momrows = 0, Gcap = 0, Galloc = 0;
    int nks_t = 0, LT = 0, cv_mom = 0;
    int afrag_group0 = 0;                               // first group of Afrag a prebuilt cross-product launch reads
    // separate-moments layout of the correlation mode (sepmom): data-only groups of MTd tiles holding
    // npg_d resamples, the feature moments of all (resample, cell) pairs from moment-only blocks
    int sepmom = 0, MTd = 0, npg_d = 0, sepmom_used = 0;
    size_t group_stride_d = 0;
    Buf out_row_d, mom_idx_d, Afrag_m, momn_m, scale;
    Buf Afrag_c, rank_c, rowtab_c, m1_c, m2_c, out_row_c, mom_idx_c, mask_c;     // compact blocks (one split / bootstrap per block)
    int has_compact_maps = 0;
    size_t group_stride = 0;
    // sliced layout (T' > PLSX_BLOCK_TP): gps groups per resample, 0 = plain
    int gps = 0;
    Buf row_slice, row_local, slice_cell0, cell_momrow;
    std::vector<int> h_slice_row0, h_slice_rows, h_slice_cell0, h_slice_ncell;
    // fixed-X fast path (behavioral permutations): pre-scaled features, no moment tiles
    int fix = 0, has_Xn = 0, MTf = 25, npgf = 0;
    size_t group_stride_f = 0;
    long long strideR = 0;
    std::vector<int> h_cell_start, h_cell_len;
    // device buffers
    Buf Xc, xmean, Y, cell_of_row, cell_start, cell_len, out_row, mom_idx, mom_n;
    Buf Afrag, R, Gm, Pm, part, Mfrag, U0T, V0, d0, tmpW;
    Buf Rfull, Vp, dp, Mvd, Cm, srcx, srcy, part2;     // split-half scratch
    Buf Kmat, swork, spct, sc;                          // SIMPLS: K = Xc Xc^T, dual-solver scratch
    Buf momout, R2, cvc, Qm, Vs, ds, ybar, pred;        // cross-validation scratch
    Buf lvsc;                                           // plsx_crossval_lv_batch: x- and y-scores of a pass's test rows, 2 x [splits][S][L]
    Buf Xn, out_row_f, mom_idx_f;                       // fixed-X fast path
    Buf Kd, Ad, Wd;                                     // dual permutation path (S x S kernel)
    Buf Zcv;                                            // SIMPLS cross-validation: Z = Vd . K, the scores of a batch of splits [n][k][S]
    // SIMPLS cross-validation under permuted Y (plsx_simpls_crossval_perm_batch): the (permutation, split) fits of a solver
    // batch -- their Y sources [n][S] int32 and training masks [n][S] bytes, expanded on the device -- and their scores
    // r, R^2 [n][k][T], sse [n][k + 1][T], usable test rows [n]
    Buf cvpsrc, cvpfit;
    // SIMPLS split-half reliability (plsx_simpls_split_half_batch): r = Xc 1_B [S] of the bound data (formed by the first
    // call after a binding), the y-loadings and yq = Y0 q of a solver batch ([n][k][T] + [n][k][S]), the half vectors of
    // a group of splits [n nsg][k][2][S] and their products with K
    Buf shrsum, shq, shG, shKG;
    int has_shrsum = 0;
    Buf Qs;                                             // SIMPLS: Xc . W0c^T (S x k), sign alignment of the bootstrap in dual space
    Buf ScT, out_row_w;                                 // single-pass bootstrap (unscaled modes): scores^T (L x S), row -> l map
    int npg_w = 0;                                      // resamples per group of the W operand (MT * 16 / L)
    Buf gws;                                            // small-solver workspace (T' > PLSX_JACOBI_TP)
    Buf status;                                         // device words: [0] numerical status bits of the small solvers, [1] refined, [2] graded but unrefined resamples
    Buf pflags;                                         // plsx_percentile_ci: series the selection kernel left to the full sort
    Buf flipws;                                         // plsx_svd_flip: column maxima, their rows, the signs
    Buf refV, refLam, refK0, refPart, refPartP, refH, Yrot;                   // graded spectra: parked eigenvectors / eigenvalues / first small rank, partial refined Grams
    int graded = 0;                                     // the ORIGINAL spectrum has live LVs below PLSX_REFINE_TAU d_max: no dual-space routes
    long long n_refined = 0, n_unrefined = 0;           // host copies of status[1], status[2] since the last plsx_numeric_report
    Buf cellS, rowc, out_row_s;                         // fused split-half: cell moments of X, row constants, row map
    Buf ccon, sFt;                                      // one-pass split reader: column constants [pair][4][Bpad], cell std [J][Bpad]
    int split_blocks_l = 0, split_reader_l = 0;         // the last split-half pass, as plsx_last_timing [19] / [20] report it
    int has_sFt = 0, split_raw = 0;                     // split_raw: the last compact split pass left raw first-half sums (one slot per split)
    int has_cellS = 0;
    // non-rotated PLS (plsx_set_contrasts): nc > 0 live contrasts; V dense (T' x L, zero padded), V in fragment order,
    // the chunk partials of k_contrast_norms [nres][nchunk][L]
    int nc = 0;
    Buf Cv, Cfrag, cpart;
    Buf mbpart;                                         // multiblock PLS: chunk partials of the row norms [nres][T'][nchunk]
    // projected permutations (perm_projected, plsx_core.hip): the row-norm partials of a launch [column block][group][row]
    Buf ppart;
    int orig_all_live = 0;                              // every LV of the original is live (plsx_set_original)
    int last_perm_projected = 0;                        // the last permutation batch took the projected route (plsx_last_timing [22])
    int dual = 0, dual_ok = 0, has_Kd = 0;              // has_Kd: the S x S kernel of the bound data is current
    Buf okx, oky;                                       // regression: usable-row masks (NaN rows)
    Buf psum, psq;                                      // k_urot resample-split partials
    // quadratic-form route of the bootstrap sums (plsx_boot_begin / plsx_boot_finish): C_l = sum_b v_bl v_bl^T
    // (L x S x S), sum_b V_b (L x S), the batch's V dense and transposed, A operand / partials of the closing pass
    Buf Cq, Vsumq, Vdq, Vtq, Afrag_q, qpart;
    int quad_active = 0;                                // 1: a series is open on the quadratic-form route
    long long quad_n = 0, series_total = 0;             // bootstraps accumulated / announced in the open series
    // coefficient series of the SIMPLS bootstrap (plsx_simpls_coef_begin / _finish): a second accumulator set of the
    // same route -- C_t = sum_b a_bt a_bt^T (T x S x S), sum_b A_b (T x S) -- fed by k_sd_coef: the batch's A dense
    // [n][T][S] and its y-loadings q [n][c][T].  The weights' own series (above) never sees it.
    Buf Cc, Asumc, Adc, Qc;
    int coef_active = 0, coef_c = 0;                    // 1: a coefficient series is open; its component count
    long long coef_n = 0;                               // bootstraps accumulated in it
    // plsx_simpls_coef_keep: the open series also keeps every A_b, appended [keep_n][T][S] to the caller's buffer
    double* keepA = nullptr;
    long long keep_cap = 0, keep_n = 0;
    Buf cichunk;                                        // plsx_simpls_coef_ci / plsx_simpls_vip_ci: one chunk of features' series [fc][T][n] / [fc][n]
    // plsx_simpls_vip_keep: every bootstrap a batch solves also leaves its scaled dual weights, appended [vip_n][vip_c][S]
    // to the caller's buffer (k_sd_vip); independent of the coefficient series
    double* vipG = nullptr;
    long long vip_cap = 0, vip_n = 0;
    int vip_c = 0;
    // plsx_boot_keep: every bootstrap a plsx_boot_batch call solves also leaves the first wkeep_m columns of its rotation
    // operand M_b, appended [wkeep_n][wkeep_m][T'] to the caller's buffer (k_keep_M); plsx_boot_weights_ci: the dual weights
    // W [n][m][S], the draw counts [n][S] and the scale table of a chunk of features [J][fc][n]
    double* wkeep = nullptr;
    long long wkeep_cap = 0, wkeep_n = 0;
    int wkeep_m = 0;
    Buf wciW, wciCnt, wciScale;
    // plsx_perm_weights_build / plsx_perm_weights_test: the operands W_p of a piece of permutations [n][m][S] (pwW), of
    // mean-centred PLS the design's averaging weights A (T' x round_up(S, 8), pwA), V0^T A (m x S, pwVA) and the builder's
    // index counters [n][2][S] (pwInv), the table
    // 1 / s_f of the bound features (pwRsd; pw_rsd: current for this binding); pw_Xn: Xn was formed for this pass by a
    // binding that keeps none (option "no_fixed_x").  The partial maxima share cppart.
    Buf pwW, pwA, pwVA, pwInv, pwRsd;
    int pw_rsd = 0, pw_Xn = 0;
    // plsx_simpls_coef_perm_begin: a permutation series of the coefficients rides along plsx_simpls_perm_batch -- the
    // caller's observed coefficients (B, T), counts (B, T) and maxima [cperm_n][T] (appended), the batch's A_p dense
    // [m][T][S] (cpA), the partial maxima of a chunk of feature blocks (cppart), the feature scale s_f (colsd)
    int cperm_active = 0, cperm_c = 0, cperm_std = 0;
    const double* cperm_obs = nullptr;
    int* cperm_count = nullptr;
    double* cperm_max = nullptr;
    long long cperm_cap = 0, cperm_n = 0;
    Buf cpA, cppart, colsd;
    // plsx_simpls_vip_perm_begin: a permutation series of the VIP scores rides along plsx_simpls_perm_batch, open or not
    // whatever the coefficient series is -- the caller's observed scores (B,), counts (B,) and maxima [vperm_n] (appended),
    // the batch's scaled dual weights dense [m][vperm_c][S] (vpG, k_sd_vip), the counts of every run of permutation
    // tiles [runs][Bpad] int32 (vpcnt); the partial maxima share cppart
    int vperm_active = 0, vperm_c = 0;
    const double* vperm_obs = nullptr;
    int* vperm_count = nullptr;
    double* vperm_max = nullptr;
    long long vperm_cap = 0, vperm_n = 0;
    Buf vpG, vpcnt;
    // plsx_simpls_set_classes: one class code per row of the bound regression data (the context's own copy), G = T
    // classes; plsx_simpls_cv_class_begin: a series of confusion counts rides along plsx_simpls_crossval_batch /
    // plsx_simpls_crossval_perm_batch -- blocks [k][G][G] int32 appended to the caller's buffer (k_sd_cv_class)
    Buf cls, clsfreq;                                   // the codes [S] and the class frequencies n_g / S [G]
    int has_cls = 0;
    CountSeries cls_series{"confusion counts", "plsx_simpls_cv_class_begin"};
    // plsx_simpls_cv_auc_begin: a second series on the same two calls, open or not whatever the first is -- blocks
    // [k][G][2] int64 appended to the caller's buffer (k_sd_cv_auc): twice the Mann-Whitney U of every class against the
    // rest, and the pairs it was counted over
    CountSeries auc_series{"AUC counts", "plsx_simpls_cv_auc_begin"};
    // plsx_simpls_cvn_class_begin: the selected counts of the nested entries; cvncnt: the per-fit blocks of a batch
    // ([nb][k][G][2] int64 where AUC counts are asked for, [nb][k][G][G] int32) and the selected ones of its groups
    NestedCounts ncls_series;
    Buf cvncnt;
    // plsx_simpls_cv_pred_begin: the predictions of the observed fits' test rows (k_sd_cv_pred), open or not whatever
    // the two series of counts are
    PredSeries pred_series;
    // plsx_crossval_pred_begin: the same for the behavioural cross-validation -- the `pred` scratch of every split of
    // plsx_crossval_batch / plsx_crossval_lv_batch / plsx_crossval_confound_batch goes out (k_cv_pred_export; c unused)
    PredSeries bpred_series;
    // plsx_simpls_set_confounds: cf_q > 0 confounds are bound -- Z~ = [1, Z - zbar] as [16][S] (cfZ) and the Cholesky
    // factor of Z~^T Z~ (cfL); per group of splits of the fold entries P_s, C_s, F_s [ns][q + 1][S], K_s [ns][S][S], the
    // usable test rows [ns], the rank status [ns], the fits' own Y [fits][S][T] and, under permutations, their scores
    // plsx_set_confounds (behavioural binding): the same cf_q / cfZ; the fold entries keep P_s of ALL the splits of a call
    // in cfP and report the splits per group of fold copies of the last call (cfb_group_l)
    int cf_q = 0, cfb_group_l = 0;
    Buf cfZ, cfL, cfP, cfC, cfF, cfK, cfnte, cfstat, cfY, cffit;
    bool has_okx = false, has_oky = false;
    int n_okx = 0;                                      // usable rows of X under the row masks (has_okx)
    double* mom_out_arg = nullptr;                      // set while a launch should export feature moments
    int ncomp = 0;
    // per-kernel-class timing (HIP events on the launch stream)
    int timing = 0;
    struct TimedEv { int cls; hipEvent_t e0, e1; };
    std::vector<TimedEv> events;
    long long timed_units = 0;
    double nt_flops = 0.0;                              // flop of the timed k_nt_gemm launches (products issued, symmetric ones by half)
    int quad_MT = 0, quad_gpl = 0, quad_series = 0;     // block height / blocks per LV of the last closing pass; series closed on that route while timing
    int last_compact_n = 0, last_compact_ktot = 0;   // compact launch behind the last run_xprod (0: none)
    int last_moment_rows = 0;                        // ... and whether its blocks formed the first moments themselves
    int last_compact_wide = 0;                       // ... and whether they held four column tiles per wave (256-column blocks)
    // how the last run_urot / Gram pass was launched (plsx_last_timing [12..18]; recorded whether or not timing is on)
    int urot_waves_l = 0, urot_splits_l = 0, urot_rps_l = 0;   // waves per block, resample splits, resamples per split
    int urot_nks_first = 0, urot_nks_last = 0, urot_tail_l = 0; // NKS template argument of the first / last L chunk's launch, TAIL
    int gram_chunks_l = 0, gram_kind_l = 0;             // column chunks; NB of k_gram4 (1..13), 0: k_gram, -1: k_gram_lds
    double scratch_gb = 48.0;                           // super-batch scratch budget
    long long R_geom[6] = {0, 0, 0, 0, 0, 0};           // (T', T'pp, Bpad, B, L, method) the R scratch was last zeroed under
    size_t R_zeroed_bytes = 0;
    double map_ms_per_gb = 0.0;                         // measured cost of mapping device memory (launch_groups), 0 = not yet
    int scratch_fixed = 0;                              // 1: always launch budget-sized super-batches
                          // resamples covered by the timed launches
    double last_ms = 0.0;
    int last_launches = 0;
    // the exported collective (plsx_comm.hip): an RCCL communicator of one rank per GPU, reached through dlopen
    void* comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    int comm_team = 0;                                  // 1: rank of a plsx_comm_init_all team (one process, several contexts)
};

namespace plsxi {


inline int fail(plsx_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg;
    return code;
}

// Nothing may unwind through the C ABI (include/plsx.h): every extern "C" entry with a body worth guarding is a
// function-try-block closed by PLSX_CATCH -- std::vector / std::string / std::thread inside the library can throw
// (host memory, thread limits), and so could anything added later.  The handlers themselves do not throw.
inline int fail_nothrow(plsx_ctx* c, int code, const char* what) noexcept
{
    if (c) {
        try { c->err = what ? what : "exception"; } catch (...) { }
    }
    return code;
}
#define PLSX_CATCH(ctxexpr)                                                                            \
    catch (const std::bad_alloc&) { return fail_nothrow(ctxexpr, PLSX_ERR_HIP, "out of host memory"); } \
    catch (const std::exception& ex_) { return fail_nothrow(ctxexpr, PLSX_ERR_STATE, ex_.what()); }      \
    catch (...) { return fail_nothrow(ctxexpr, PLSX_ERR_STATE, "unknown C++ exception inside libplsx"); }

#define HIPCHK(call)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(ctx, PLSX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define LAUNCHCHK()                                                                       \
    do {                                                                                  \
        hipError_t e_ = hipGetLastError();                                                \
        if (e_ != hipSuccess)                                                             \
            return fail(ctx, PLSX_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e_)); \
    } while (0)

inline int ensure(plsx_ctx* ctx, Buf& b, size_t bytes, bool zero = false)
{
    if (b.bytes < bytes) {
        if (b.p) HIPCHK(hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
        HIPCHK(hipMalloc(&b.p, bytes));
        b.bytes = bytes;
        if (zero) HIPCHK(hipMemset(b.p, 0, bytes));
    }
    return 0;
}

inline void release(Buf& b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

template <class T>
T* ptr(const Buf& b) { return static_cast<T*>(b.p); }

// Kernels that need more than the default 64 KB of dynamic LDS.  The attribute
// belongs to the (device, function) pair, so it is set on every launch path
// instead of being cached in a per-process flag (a second context on another
// GPU of the same process must not skip it); the call costs ~1 us.
template <class F>
hipError_t set_lds(F* fn, size_t bytes)
{
    if (bytes <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes);
}

// kernel classes of plsx_kernel_timing()
enum { KC_XPROD = 0, KC_GRAM, KC_SMALL, KC_UROT, KC_NT, KC_UCORR, KC_SIMPLS, KC_BUILD, KC_MOM, KC_CVSCORE, KC_COEF, KC_COEFPROD, KC_PCTL,
       KC_CONTRAST, KC_ROWNORM, KC_CVCLASS, KC_CVAUC, KC_WEIGHTSPROD, KC_CVPMOM, KC_CVPGRAM, KC_CVPW, KC_CVPG, KC_CVPMEAN, KC_CVFINAL, KC_CVLV, KC_CVPLV, KC_CFRESID, KC_CFPREP, KC_CFK, KC_CFY, KC_CFBX, KC_COUNT };
extern const char* const kKernelClassNames[KC_COUNT];

// Brackets the launches of one kernel class with two events when timing is on.
struct KTimer {
    plsx_ctx* c; int cls; hipStream_t st; hipEvent_t e0 = nullptr;
    KTimer(plsx_ctx* ctx, int k, hipStream_t s) : c(ctx), cls(k), st(s)
    {
        if (c->timing && hipEventCreate(&e0) == hipSuccess) (void)hipEventRecord(e0, st);
    }
    ~KTimer()
    {
        if (!e0) return;
        hipEvent_t e1 = nullptr;
        if (hipEventCreate(&e1) == hipSuccess) {
            (void)hipEventRecord(e1, st);
            c->events.push_back({cls, e0, e1});
        } else (void)hipEventDestroy(e0);
    }
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round_up(int a, int b) { return ceil_div(a, b) * b; }

// Physical cross-product groups of `rgroups` resample groups.
inline int phys_groups(const plsx_ctx* c, int rgroups) { return c->gps > 0 ? rgroups * c->gps : rgroups; }

// Dual-space routes (S x S kernel: permutations, single-pass bootstraps of the unscaled modes) never form R and
// so cannot refine a graded spectrum (run_small); a data set whose ORIGINAL spectrum is graded takes the feature pass.
inline int use_dual(const plsx_ctx* ctx) { return (ctx->dual && !ctx->graded) ? 1 : 0; }

#define NEED_DATA()                                                             \
    if (!ctx) return PLSX_ERR_ARG;                                              \
    if (!ctx->has_data) return fail(ctx, PLSX_ERR_STATE, "plsx_set_data has not been called")
#define NEED_ORIG()                                                             \
    NEED_DATA();                                                                \
    if (!ctx->has_orig) return fail(ctx, PLSX_ERR_STATE, "plsx_set_original has not been called")

struct MomLayout { int pairs, mt, groups; size_t stride; };

// Dynamic LDS of the A-operand builders with room for the occurrence chains of a cell's (k_build_A_behav) / of all S
// (k_build_A_mc) positions: 2 ints per position behind the 2 T doubles; *cap = ints granted (0: cells too large for
// the tables -> the kernel falls back to atomic adds).
inline size_t build_lds_behav(const plsx_ctx* ctx, int* cap)
{
    int ml = 0;
    for (int v : ctx->h_cell_len) ml = std::max(ml, v);
    const size_t base = (size_t)2 * ctx->T * 8, ints = (size_t)2 * ml;
    if (base + ints * 4 > 60 * 1024) { *cap = 0; return base; }
    *cap = (int)ints;
    return base + ints * 4;
}
inline size_t build_lds_mc(const plsx_ctx* ctx, int* cap)
{
    const size_t ints = (size_t)2 * ctx->S;
    if (ints * 4 > 60 * 1024) { *cap = 0; return 0; }
    *cap = (int)ints;
    return ints * 4;
}

// ---- plsx_core.hip ----
int plan_groups(plsx_ctx* c);
int upload_rowmaps(plsx_ctx* ctx);
int plan_sepmom(plsx_ctx* ctx);
int ensure_scratch(plsx_ctx* ctx, int groups);
int launch_groups(plsx_ctx* ctx, long long units, int per_group);
int balanced_batch(int n, int cap, int per_group);
void probe_map_cost(plsx_ctx* ctx);
int chip_slots(const void* kernel);
int pick_parts(long long units, int slots, int lo, int hi);
SmallArgs small_args(plsx_ctx* ctx, int mode);
bool plsc_single_pass(const plsx_ctx* ctx);
int note_spectrum(plsx_ctx* ctx, const double* d_sv, hipStream_t st, int* all_live = nullptr);
// One accumulator set of the quadratic-form route: C (L x S x S), Vsum (L x S), fed from Vd dense [m][L][S].  nullptr
// where a QuadSet is optional: the weights' own set (ctx->Cq, ctx->Vsumq, ctx->Vdq; L = LVs / components).
struct QuadSet { Buf* C; Buf* Vsum; const double* Vd; int L; };
int quad_accumulate(plsx_ctx* ctx, int m, hipStream_t st, const QuadSet* qs = nullptr);
bool quad_applicable(const plsx_ctx* ctx);
// non-rotated PLS: out_sv[r][l] = || R_r^T v_l || of the nres resamples in the cross-product scratch; Mfrag[r] = V
int run_contrast_norms(plsx_ctx* ctx, int nres, double* out_sv, hipStream_t st);
int run_contrast_fill(plsx_ctx* ctx, int nres, hipStream_t st);
// the two interpolated order statistics of nseries contiguous series of n values (plsx_percentile_ci's body)
int run_percentile(plsx_ctx* ctx, const double* d_data, long long nseries, int n, int i_lo, double g_lo, int i_hi,
                   double g_hi, double* d_lo, double* d_hi, hipStream_t st);
// an open coefficient series ends: with it what it was told to keep
inline void coef_close(plsx_ctx* ctx)
{
    ctx->coef_active = 0; ctx->coef_n = 0;
    ctx->keepA = nullptr; ctx->keep_cap = 0; ctx->keep_n = 0;
}
// a kept VIP stack ends (plsx_set_data, plsx_simpls_set_original, a second plsx_simpls_vip_keep)
inline void vip_close(plsx_ctx* ctx)
{
    ctx->vipG = nullptr; ctx->vip_cap = 0; ctx->vip_n = 0; ctx->vip_c = 0;
}
// a kept stack of rotation operands ends (plsx_set_data, plsx_set_original, plsx_boot_keep(ctx, NULL, 0, 0))
inline void wkeep_close(plsx_ctx* ctx)
{
    ctx->wkeep = nullptr; ctx->wkeep_cap = 0; ctx->wkeep_n = 0; ctx->wkeep_m = 0;
}
// an open permutation series of the coefficients ends (plsx_set_data, plsx_simpls_set_original, a second
// plsx_simpls_coef_perm_begin, plsx_simpls_coef_perm_end); the buffers stay the caller's
inline void cperm_close(plsx_ctx* ctx)
{
    ctx->cperm_active = 0; ctx->cperm_c = 0; ctx->cperm_std = 0;
    ctx->cperm_obs = nullptr; ctx->cperm_count = nullptr; ctx->cperm_max = nullptr;
    ctx->cperm_cap = 0; ctx->cperm_n = 0;
}
// an open permutation series of the VIP scores ends (plsx_set_data, plsx_simpls_set_original, a second
// plsx_simpls_vip_perm_begin, plsx_simpls_vip_perm_end); the buffers stay the caller's
inline void vperm_close(plsx_ctx* ctx)
{
    ctx->vperm_active = 0; ctx->vperm_c = 0;
    ctx->vperm_obs = nullptr; ctx->vperm_count = nullptr; ctx->vperm_max = nullptr;
    ctx->vperm_cap = 0; ctx->vperm_n = 0;
}
// ---- plsx_xprod.hip ----
int launch_xprod(plsx_ctx* ctx, int groups, hipStream_t st);
int launch_xprod_acc(plsx_ctx* ctx, const double* Afrag, size_t gstride, int groups, int L, hipStream_t st);
int run_xprod_fixed(plsx_ctx* ctx, const int* ysrc, int nres, hipStream_t st, const double* ystack);
// projected permutations: out_sv[r][l] = || row l of (V0^T A_r) Xn || -- no R, no Gram matrix, no small solver
int run_xprod_fixed_norms(plsx_ctx* ctx, const int* ysrc, int nres, hipStream_t st, const double* ystack, double* out_sv);
MomLayout moment_layout(const plsx_ctx* ctx, int npairs);
MomLayout moment2_layout(const plsx_ctx* ctx, int npairs);     // X^2-only blocks (EPI 9)
bool compact_boot_wide(const plsx_ctx* ctx);                   // the compact bootstrap blocks hold four column tiles per wave
int compact_boot_ksteps(int mt, bool wide);                    // k-steps per LDS stage of the compact bootstrap blocks
bool compact_moment_rows(const plsx_ctx* ctx);                 // the compact bootstrap blocks form m1 in their padding rows
int launch_moment_blocks_raw(plsx_ctx* ctx, const MomLayout& ml, SplitEpi se, hipStream_t st);   // EPI 6: raw m1, m2
int ensure_compact_maps(plsx_ctx* ctx);
// multiblock PLS: every row t < T' of the nres resamples in the cross-product scratch to unit norm over the B features
int run_mb_rownorm(plsx_ctx* ctx, int nres, hipStream_t st);
int run_xprod(plsx_ctx* ctx, const int* xsrc, const int* ysrc, int nres, hipStream_t st,
              bool prebuilt = false, const double* ystack = nullptr, long long ystride = -1, bool sparse_rows = false);
int launch_xprod_split(plsx_ctx* ctx, int groups, SplitEpi se, hipStream_t st);
int quad_finish(plsx_ctx* ctx, double* d_usum, double* d_usq, hipStream_t st, const QuadSet* qs = nullptr);
// Row blocks per LV of the closing pass of a bootstrap series (quad_finish): blocks of 8 tiles = 128 rows.  A block
// multiplies its rows of the symmetric C_l against the columns from its own first row on, so the work issued beyond
// the upper triangle is the lower halves of the diagonal blocks: 1.34 x the needed flop with 3 blocks of 21 tiles at
// S = 1000, 1.13 x with 8 blocks of 8 -- measured at c5 32.5 -> 26.8 ms per series (blocks of 12 tiles 28.5, of 6
// tiles 27.2, of 4 tiles 28.0, of 16 tiles 38.5: the time follows the issued work down to 8 tiles).
inline int quad_blocks(int tiles) { return tiles >= 8 ? ceil_div(tiles, 8) : 1; }
// ---- plsx_compact.hip ----
int launch_cboot(plsx_ctx* ctx, int nres, int nks_c, SplitEpi se, hipStream_t st);
int launch_csplit(plsx_ctx* ctx, int m, int nks_c, SplitEpi se, hipStream_t st, bool raw = false);
// ---- plsx_gram.hip ----
int run_nt(plsx_ctx* ctx, const double* A, long long strideA, int lda, int Ma,
           const double* B1, long long strideB1, int ldb1, int N1,
           const double* B2, long long strideB2, int ldb2, int N2, int K, int batch,
           double* C1, long long strideC1, int ldc1, double* C2, long long strideC2, int ldc2,
           hipStream_t st, bool sym = false, bool accumulate = false, bool one_chunk = false);
bool nt_sym_fits(int S);
int nt_strips(plsx_ctx* ctx, const double* A, int lda, int Ma, const double* Bm, int ldb, int N, int Kc,
              double* C, int ldc, hipStream_t st, bool one_chunk = false);
int form_gram_K(plsx_ctx* ctx, const double* X, int ldx, int S, int Kc, double* K, int ldk, hipStream_t st);
int run_dual_gp(plsx_ctx* ctx, int m, int Sd, const double* ScT, int L, hipStream_t st);
int run_gram_ex(plsx_ctx* ctx, int nres, int mode, const double* E, int Erows, double* Pout,
                hipStream_t st, const double* Rsrc = nullptr);
int run_gram(plsx_ctx* ctx, int nres, bool with_p, hipStream_t st);
// ---- plsx_small.hip ----
int run_small(plsx_ctx* ctx, SmallArgs a, int nres, hipStream_t st, const double* Rref = nullptr);
// ---- plsx_smallql1.hip / plsx_smallql2.hip ----
int launch_small_ql(plsx_ctx* ctx, const SmallArgs& a, int nres, size_t ws, size_t lds, hipStream_t st);
int launch_small_ql_refined(plsx_ctx* ctx, const SmallArgs& a, int nres, size_t ws, size_t lds, hipStream_t st);
// ---- plsx_urot.hip ----
int run_urot(plsx_ctx* ctx, int nres, double* usum, double* usq, double* out, hipStream_t st);
int launch_ucorr(plsx_ctx* ctx, dim3 grid, dim3 block, hipStream_t st, const double* M, int tpc,
                 double* part, int npairs);
int ucorr_slots();
// ---- plsx_weightsci.hip ----
// plsx_boot_keep's share of a solver batch: M_r of the `m` resamples whose operands the small solver just left in ctx->Mfrag
int wkeep_append(plsx_ctx* ctx, int m, hipStream_t st);
// ---- plsx_simpls_api.hip ----
bool simpls_single_pass(const plsx_ctx* ctx);
size_t simpls_global_lds_bytes(int T, int k);
bool simpls_onchip_fits(int S, int T, int k);
int simpls_form_K(plsx_ctx* ctx, hipStream_t st);
// ---- plsx_confound.hip ----
int cf_fold_prepare(plsx_ctx* ctx, const uint8_t* d_masks, int s0, int ns, hipStream_t st);
int cf_fold_Y(plsx_ctx* ctx, int ngc, const int32_t* d_perm, int mb, double* Ys, hipStream_t st);
int cf_expand_masks(plsx_ctx* ctx, const uint8_t* d_masks, int mb, int nfit, uint8_t* pmask, hipStream_t st);
int cf_cvp_acc(plsx_ctx* ctx, const double* r, const double* r2, const double* sse, int ngc, int mb, int n, bool last,
               double* out_r, double* out_r2, double* out_mse, hipStream_t st);
// ---- plsx_confound_behav.hip ----
int cfb_prepare(plsx_ctx* ctx, const char* who, const uint8_t* d_masks, int n, hipStream_t st);
int cfb_fold_X(plsx_ctx* ctx, int s0, int g, double* Xf, hipStream_t st);
int cfb_fold_Y(plsx_ctx* ctx, int s, const int32_t* d_perm, int mb, int nfit, double* Ys, hipStream_t st);
int cfb_identity(plsx_ctx* ctx, int* idx, int n, hipStream_t st);
// ---- plsx_split.hip ----
// the open series of plsx_crossval_pred_begin: room for m more slots (PLSX_ERR_ARG before anything is computed), and the
// export of the `pred` scratch [mm][S][T] of a pass into slots slot0 .. of this call (Y: the rows the pass observed,
// split i at Y + i * ystride)
int cv_pred_reserve(plsx_ctx* ctx, const char* who, int m);
int cv_pred_export(plsx_ctx* ctx, const double* pred, const uint8_t* masks, int mm, const double* Y, long long ystride,
                   long long slot0, hipStream_t st);
// ---- plsx_cvperm.hip ----
// both fold entries of the behavioural confound regression: d_perm_idx == nullptr (observed): the identity, m = 1, and
// the scores of every split instead of their mean
int cvperm_fold_entry(plsx_ctx* ctx, const char* who, const uint8_t* d_masks, int n, const int32_t* d_perm_idx, int m,
                      double* d_r, double* d_r2, double* d_lv, double* d_lv_pairs, bool observed, void* stream);

}  // namespace plsxi
