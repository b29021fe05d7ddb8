/*
 * plsx.h -- C ABI of the MI355X PLS-C resampling engine (libplsx.so).
 *
 * Drop-in boundary for the resampling seam of netneurolab/pypyls: the calls
 *     BasePLS.permutation / BasePLS.bootstrap / BasePLS.split_half
 * dispatch `_single_perm` / `_single_boot` once per resample through
 * `utils.get_par_func` (pyls/base.py:490-507, 644-650; pyls/utils.py:252-279).
 * This library replaces that per-resample dispatch by batched device work.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++ or torch types.
 *   - every `d_*` pointer is a DEVICE pointer owned by the caller (the Python
 *     host obtains them from torch tensors' data_ptr()); fp64, row-major
 *     C-order unless stated; index arrays int32.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *     Work is enqueued asynchronously; call plsx_sync() (or synchronise the
 *     stream yourself) before reading outputs.
 *   - every entry returns 0 on success or a negative plsx_status; the message
 *     is available from plsx_last_error().  No C++ exception crosses the ABI,
 *     the library never frees caller buffers.
 *   - one context per GPU, not shared between host threads.
 */
#ifndef PLSX_H_
#define PLSX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plsx_ctx plsx_ctx;

enum plsx_status {
    PLSX_OK = 0,
    PLSX_ERR_ARG = -1,       /* bad shape / flag / null pointer            */
    PLSX_ERR_UNSUPPORTED = -2, /* shape outside what the device path covers */
    PLSX_ERR_HIP = -3,       /* HIP runtime failure (incl. out of device or host memory) */
    PLSX_ERR_STATE = -4,     /* call order violated (e.g. no data set); a C++ exception caught at the boundary */
    PLSX_ERR_NUMERIC = -5    /* an eigen-solve of a finished batch did not converge (reported by plsx_sync) */
};

enum plsx_method {
    PLSX_BEHAVIORAL = 0,     /* pyls/types/behavioral.py  (R = stacked per-cell xcorr)   */
    PLSX_MEANCENTERED = 1,   /* pyls/types/meancentered.py (R = cell means - ref. mean)  */
    PLSX_REGRESSION = 2,     /* pyls/types/regression.py (SIMPLS); plsx_set_data takes
                                globally centred X / Y, n_groups = 1 and n_cond = n_components */
    PLSX_MULTIBLOCK = 3      /* task and behaviour blocks in one decomposition (no pyls counterpart; the Matlab
                                toolbox's method 4 in structure): R = [rownorm(R_meancentered); rownorm(R_behavioral)],
                                T' = J + J T rows -- the J task rows (group-major, then condition), then the behaviour
                                rows (group, condition, behaviour); rownorm divides a row by its L2 norm over the B
                                features (a zero row stays zero).  Needs d_Y; takes n_groups, n_cond, mean_centering and
                                PLSX_FLAG_COVARIANCE.  One resample with the moment rows of its cells must fit one
                                24-tile cross-product block (ceil(T'/16) + 2 ceil(J/16) <= 24; PLSX_ERR_UNSUPPORTED
                                otherwise).  plsx_crosscov_batch / plsx_perm_batch: an index array given as d_ysrc alone
                                (a permutation) also places the rows of X into the cells of the task block; d_xsrc, when
                                given, does that (bootstraps: both).  plsx_set_contrasts, plsx_split_half_batch[_y],
                                plsx_crossval_batch and plsx_perm_batch_y: not built (PLSX_ERR_UNSUPPORTED / _ARG) */
};

/* flags for plsx_set_data */
#define PLSX_FLAG_COVARIANCE 1u   /* xcorr(..., covariance=True), pyls/compute.py:86-87 */

/* Library / ABI version (major*1000 + minor). */
int plsx_version(void);

/* Largest stacked-Y dimension T' = J*T of behavioral PLS (rows of one resample;
 * above 352 they are sliced over several cross-product blocks).  Mean-centred
 * PLS (T' = J cells) and SIMPLS (T' = n_components) are limited to 352; multiblock
 * PLS (T' = J + J*T) to one 24-tile block: ceil(T'/16) + 2 ceil(J/16) <= 24. */
int plsx_max_tprime(void);

/* Create / destroy the per-GPU context (streams, scratch).               */
int plsx_ctx_create(int device, plsx_ctx** out);
int plsx_ctx_destroy(plsx_ctx* ctx);
const char* plsx_last_error(const plsx_ctx* ctx);
int plsx_sync(plsx_ctx* ctx);

/*
 * Bind the data set.  Replaces what BasePLS.__init__ stores in self.inputs /
 * self.dummy (pyls/base.py:254-283).
 *   d_X          (S, B) fp64
 *   d_Y          (S, T) fp64, NULL for PLSX_MEANCENTERED (required for PLSX_MULTIBLOCK)
 *   d_cell_of_row (S,) int32, cell index in [0, J): group-major then condition
 *                (pyls/utils.py:178-197)
 *   n_groups * n_cond == J
 *   mean_centering in {0,1,2} (pyls/compute.py:267-317), ignored for behavioral;
 *                the task block of PLSX_MULTIBLOCK uses it
 * The library keeps its own centred, padded copy; the caller may release d_X /
 * d_Y afterwards.
 * PLSX_REGRESSION also forms K = X0 X0^T (S x S doubles) here and refuses
 * (PLSX_ERR_UNSUPPORTED) when K does not fit in free device memory, or when
 * the T x T work of one wave's slice of LDS, 8 (T^2 + 5 T + 2 k) bytes, exceeds
 * 158 KB.  S has no other bound: beyond 8 (T^2 + S) <= 158 KB (S ~ 20 000 at
 * T = 10) the component steps keep their S-long data in device scratch (the
 * route the "simpls_global" option forces at any S).
 */
int plsx_set_data(plsx_ctx* ctx, int method, const double* d_X, const double* d_Y,
                  const int32_t* d_cell_of_row, int S, int B, int T,
                  int n_groups, int n_cond, int mean_centering, unsigned flags,
                  void* stream);

/* Number of latent variables L = min(T', B) and T' for the bound data set. */
int plsx_num_lv(const plsx_ctx* ctx);
int plsx_tprime(const plsx_ctx* ctx);

/*
 * Cross-covariance matrices of resampled data -- gen_covcorr
 * (pyls/types/behavioral.py:27-52, pyls/types/meancentered.py:50-73) applied
 * to (X[xsrc], Y[ysrc]) for n resamples at once.
 *   d_xsrc, d_ysrc  (n, S) int32: row of X / of Y placed at each position;
 *                   NULL means the identity; an entry of -1 in d_xsrc drops the
 *                   position (split-half masks, pyls/base.py:760-762).
 *   d_R             (n, T', B) fp64 out
 * Mainly a test / inspection hook: the batched entries below keep R on chip /
 * in library scratch.
 */
int plsx_crosscov_batch(plsx_ctx* ctx, const int32_t* d_xsrc, const int32_t* d_ysrc,
                        int n, double* d_R, void* stream);

/*
 * Test / inspection hook: rows [row0, row0 + nrows) of slot `slot` of the cross-product scratch as the last batch
 * left them, at their full pitch -- d_out (nrows, Bpad) fp64 with Bpad = (B + L) rounded up to 128: the B features,
 * the L score columns of gen_distrib, zero padding.  A slot has T' rounded up to 4 rows; those >= T' read zero.
 * PLSX_ERR_ARG for rows or a slot the scratch does not hold (it is mapped by the first batch after plsx_set_data).
 */
int plsx_scratch_read(plsx_ctx* ctx, int slot, int row0, int nrows, double* d_out, void* stream);

/*
 * Decomposition of the un-resampled data -- BasePLS.svd (pyls/base.py:401-437
 * -> pyls/compute.py:10-52) without the sign convention (the host applies
 * sklearn's svd_flip rule and hands the result back via plsx_set_original).
 *   d_xw (B, L), d_sv (L,), d_yw (T', L)  out
 */
int plsx_decompose(plsx_ctx* ctx, double* d_xw, double* d_sv, double* d_yw, void* stream);

/*
 * Non-rotated PLS: the effects are the caller's contrasts over the rows of R (cell-major: group, then condition, then
 * behaviour -- the row order of y_weights), nothing is decomposed and nothing is rotated.  Called after plsx_set_data;
 * plsx_decompose / plsx_set_original follow as usual.
 *   d_C  (T', Lc) fp64, unit columns (the host normalises); copied before the call returns
 *   Lc   1 .. min(T', B).  Lc = 0 or d_C = NULL returns the context to SVD mode; so does plsx_set_data.
 * Internally C is zero-padded to the context's L = min(T', B) columns: every layout stays as it is, the columns >= Lc
 * of every result are zero and the host slices [:Lc].  While contrasts are set, with V = C:
 *   plsx_decompose         Z = R^T V (B, L); d_sv[l] = ||Z[:, l]||; d_xw[:, l] = Z[:, l] / d_sv[l] (0 where the norm
 *                          is 0); d_yw = V.  The contrast fixes the sign: plsx_svd_flip is not called.
 *   plsx_perm_batch[_y]    d_out_sv[p][l] = ||R_p^T v_l||; `rotate` is ignored.  Feature pass: one pass over R_p
 *                          (k_contrast_norms: fixed chunking of the features, fixed summation order -- the same bits
 *                          whatever the batch size, the scratch budget or the team); dual route: v_l^T G_p v_l.
 *   plsx_boot_batch        accumulates U_b = R_b^T V and its squares (with plsx_boot_begin / _finish as usual);
 *                          d_distrib as usual.
 *   plsx_split_half_batch[_y], plsx_crossval_batch   PLSX_ERR_UNSUPPORTED.
 * A contrast whose singular value lies below 1e-3 of the largest takes the binding off the dual-space routes, as a
 * graded spectrum does (plsx_set_original).  PLSX_ERR_ARG for data bound for regression or Lc out of range.
 */
int plsx_set_contrasts(plsx_ctx* ctx, const double* d_C, int Lc, void* stream);

/* Fix the original decomposition used for Procrustes alignment
 * (`original=` of _single_perm / _single_boot, pyls/base.py:505,648). */
int plsx_set_original(plsx_ctx* ctx, const double* d_xw, const double* d_sv,
                      const double* d_yw, void* stream);

/* Sign convention of compute.svd (pyls/compute.py:43-50, sklearn's svd_flip applied to the decomposed matrix):
 * in place on the DEVICE copies of the decomposition -- when T' <= B the entry of largest magnitude of every
 * x_weights column becomes positive, otherwise that of every y_weights column; both factors get the same signs.
 * d_xw (B, L), d_yw (T', L) as plsx_decompose wrote them.  (The host may equally apply the rule itself.)
 * Data bound for regression: d_xw (B, k) x_weights, d_yw (T, k) the right vectors of plsx_simpls_decompose; the
 * x side leads when B > T (compute.svd of the T x B cross-product, pyls/types/regression.py:103, compute.py:43-50). */
int plsx_svd_flip(plsx_ctx* ctx, double* d_xw, double* d_yw, void* stream);

/* d_out[i][k] = d_in[i][k] * d_scale[k] on (rows, cols) row-major arrays (in place allowed): the device side of
 * `x_weights @ singvals` (pyls/types/behavioral.py:201, the `orig` of compute.boot_rel). */
int plsx_scale_columns(plsx_ctx* ctx, const double* d_in, long long rows, int cols, const double* d_scale,
                       double* d_out, void* stream);

/* d_dst (cols, rows) = d_src (rows, cols)^T, both dense row-major: the (n_boot, T' L) bootstrap distributions
 * as the (T' L, n_boot) series plsx_percentile_ci and PLSResults' (T', L, n_boot) layout want them. */
int plsx_transpose(plsx_ctx* ctx, const double* d_src, int rows, int cols, double* d_dst, void* stream);

/* d_out[r][c] = d_in[r][c] - mean(d_in[r][:]) on (rows, cols) row-major arrays (in place allowed; fixed summation
 * order): the column-centred original x_weights that plsx_simpls_set_original takes, formed on the device from the
 * (k, B) output of plsx_simpls_decompose (the centring inside compute.efficient_corr(x_weights, original), pyls/types/regression.py:318-319). */
int plsx_center_rows(plsx_ctx* ctx, const double* d_in, int rows, long long cols, double* d_out, void* stream);

/* Centred projection (X - colmean(X)) @ W for W given as (B, L): the device
 * part of `x_scores = X @ x_weights` (pyls/base.py:364).  d_out (S, L). */
int plsx_project(plsx_ctx* ctx, const double* d_W, int L, double* d_out, void* stream);
/* Column means of X, (B,) out. */
int plsx_colmean(plsx_ctx* ctx, double* d_mean, void* stream);

/*
 * Permutation null -- BasePLS.permutation / _single_perm with
 * use_permind=True (pyls/base.py:601-712).
 *   d_perm_idx (n, S) int32  one permutation per ROW (transpose of the
 *              reference's (S, P) permsamples)
 *   rotate     Procrustes-rotate onto the original y_weights (base.py:696-700)
 *              or return the raw singular values (:702)
 *   d_out_sv   (n, L) out
 */
int plsx_perm_batch(plsx_ctx* ctx, const int32_t* d_perm_idx, int n, int rotate,
                    double* d_out_sv, void* stream);

/*
 * Same with pre-permuted behaviour matrices instead of index vectors
 * (`permindices=False`: surrogate / spatially-constrained null models,
 * pyls/base.py:636-639, 691-692; pyls/structures.py:115-120).
 *   d_ystack (n, S, T) fp64: the Y matrix of every permutation
 */
int plsx_perm_batch_y(plsx_ctx* ctx, const double* d_ystack, int n, int rotate,
                      double* d_out_sv, void* stream);

/*
 * Bootstrap -- BasePLS.bootstrap / _single_boot (pyls/base.py:439-576).
 *   d_boot_idx (n, S) int32  one bootstrap sample per ROW
 *   d_usum, d_usq (B, L)  accumulated IN PLACE: += sum_r U_r, += sum_r U_r**2
 *                 with U_r the Procrustes-rotated, singular-value-scaled left
 *                 singular vectors (base.py:510-511, 570)
 *   d_distrib  (n, T', L) out: gen_distrib of every bootstrap (base.py:574)
 */
int plsx_boot_batch(plsx_ctx* ctx, const int32_t* d_boot_idx, int n,
                    double* d_usum, double* d_usq, double* d_distrib, void* stream);

/*
 * A SERIES of bootstrap batches that accumulate into the same (d_usum, d_usq) -- the whole `for i in range(n_boot)`
 * of BasePLS.bootstrap (pyls/base.py:490-511) on this rank -- may be announced, so that the library can move the
 * pass over the B features out of the loop:
 *   plsx_boot_begin(ctx, n_total)   before the first batch; n_total = bootstraps this context will see until
 *                                   plsx_boot_finish
 *   plsx_boot_batch / plsx_simpls_boot_batch ...  as ever
 *   plsx_boot_finish(ctx, d_usum, d_usq)   after the last batch, before d_usum / d_usq are read: adds what the
 *                                   series still owes them; a no-op when every batch already accumulated in place
 * Where the rotated bootstrap weights are linear in the bound, unscaled feature matrix -- U_b = Xc^T V_b with V_b
 * (S x L) known in dual space: mean-centred PLS and covariance-mode behavioral PLS (single-pass route), SIMPLS --
 *   sum_b U_b = Xc^T (sum_b V_b),     sum_b U_b[j,l]^2 = x_j^T C_l x_j,     C_l = sum_b v_bl v_bl^T   (S x S)
 * so a series of n_total >~ 0.85 S .. 1.25 S bootstraps (the closing pass uses the symmetry of C_l in row blocks;
 * B well above S features) accumulates C_l (a batched S x S product per batch) and passes the
 * features ONCE, in plsx_boot_finish (2 S^2 L B flop), instead of once per bootstrap (2 S L B n_total): the same
 * sums to rounding.  Between begin and finish of such a series the batches do NOT touch d_usum / d_usq
 * (plsx_boot_route() = 1); d_distrib / d_yload are written per batch as ever.  Without plsx_boot_begin, for short
 * series, correlation-mode behavioral PLS (the features are re-scaled per bootstrap) and with option "quad_sums" = -1
 * every batch accumulates in place (route 0).  plsx_set_original / plsx_set_data end an open series.
 */
int plsx_boot_begin(plsx_ctx* ctx, long long n_total, void* stream);
int plsx_boot_finish(plsx_ctx* ctx, double* d_usum, double* d_usq, void* stream);
int plsx_boot_route(const plsx_ctx* ctx);

/*
 * Percentile intervals of the rotated bootstrap weights of PLS-C (behavioral and mean-centred PLS; no reference
 * counterpart: the (B, L, n_boot) series is 400 GB at B = 200 000, L = 50, n_boot = 5000).  With A_b (T' x S) the
 * cross-product operand of bootstrap b in subject space (count-weighted, zero outside a row's own cell) and M_b
 * (T' x L) the rotation operand of the small solver, W_b = M_b^T A_b (L x S) and what plsx_boot_batch adds into
 * d_usum for bootstrap b is
 *   U_b[f][l] = sum_g sigma_{b,g}(f) . sum_{s in cell g} W_b[l][s] . Xc[s][f]
 * sigma = 1 in the unscaled modes (mean-centred PLS, PLSX_FLAG_COVARIANCE); in correlation mode sigma_{b,g}(f) is
 * 1 / std (ddof 1) of feature f over the rows bootstrap b draws into cell g, from the raw moments as the cross-product
 * epilogues form it, and 0 for a cell-constant feature.  The units are those of x_weights @ diag(singvals).
 *
 *   plsx_boot_keep          d_M (capacity, m, T') fp64, dense: every bootstrap that later plsx_boot_batch calls solve
 *                           leaves the first m columns of M_b, transposed, appended in submission order -- on every
 *                           bootstrap route (general feature pass, compact blocks, single-pass / quadratic-form,
 *                           T' > 64, graded resamples after their refinement).  Bootstrap-major, so that the stacks
 *                           of several contexts concatenate.  d_usum, d_usq, d_distrib keep their bits.  A batch that
 *                           no longer fits returns PLSX_ERR_ARG before it computes anything.  plsx_set_data,
 *                           plsx_set_original and plsx_boot_keep(ctx, NULL, 0, 0) end the keeping; the buffer stays
 *                           the caller's.  PLSX_ERR_STATE without bound PLS-C data and a set original,
 *                           PLSX_ERR_UNSUPPORTED with contrasts or a multiblock binding, PLSX_ERR_ARG for m outside
 *                           1 .. L, a null buffer or capacity < 1.
 *   plsx_boot_weights_ci    d_boot_idx (n, S) int32 index rows, d_M (n, m, T') -- a kept stack, the gathered stacks
 *                           of several ranks, or ANY stack and index rows (the entry keeps no state of the series) --
 *                           -> d_lo / d_hi (B, m): the interpolated order statistics
 *                           (1 - g) x[i] + g x[i + 1] of {U_b[f][l] : b < n} at (i_lo, g_lo) and (i_hi, g_hi), as
 *                           plsx_percentile_ci takes them.  The pass rebuilds A_b from the index rows with the
 *                           builders of the bootstrap routes, forms W (n, m, S), and walks the features in chunks of
 *                           whole 128-feature blocks: per chunk the scale table sigma [cell][feature][bootstrap]
 *                           (correlation mode only, k_weights_scale), the series [feature][l][n] (k_weights_prod:
 *                           k_coef_prod's tile with the contraction run cell segment by cell segment, each segment's
 *                           partial tile multiplied by sigma before it joins the total), then the selection kernels
 *                           (option "percentile_sort" applies).  The (B, m, n) array never exists whole: a chunk's
 *                           series is 2 GB at most, and series, scale table, stack and W stay inside the scratch
 *                           budget and free device memory.  Every entry is one block's contraction in a fixed order
 *                           (cells ascending, subjects ascending): the same bits run to run and whatever the
 *                           chunking; no floating-point atomics.
 *                           Limits: PLSX_ERR_UNSUPPORTED (context still usable, sizes in plsx_last_error) for
 *                           n > 16384, when not even the smallest chunk fits, for m T' > 20448 (the LDS of the
 *                           dual-weight kernel) and for a multiblock binding; PLSX_ERR_ARG for n < 1, m outside
 *                           1 .. L, an index outside 0 .. n - 1, a null pointer; PLSX_ERR_STATE without bound PLS-C
 *                           data.
 */
int plsx_boot_keep(plsx_ctx* ctx, double* d_M, long long capacity, int m);
int plsx_boot_weights_ci(plsx_ctx* ctx, const int32_t* d_boot_idx, const double* d_M, int n, int m, int i_lo,
                         double g_lo, int i_hi, double g_hi, double* d_lo, double* d_hi, void* stream);

/*
 * Permutation test of the PLS-C x_weights (behavioral and mean-centred PLS; no reference counterpart: the (B, L, n_perm)
 * series is 400 GB at B = 200 000, L = 50, n_perm = 5000).  With V0 (T' x m) the first m columns of the observed
 * y_weights (with contrasts: of the normalised contrasts) and R_p the cross-covariance matrix of permutation p --
 * gen_covcorr of make_permutation: behavioral PLS moves the rows of Y against X, mean-centred PLS the rows of X across
 * the cells -- the null is
 *   Z_p = R_p^T V0   (B x m),
 * the permuted cross-covariance read along the observed behavioural pattern.  Where the Procrustes rotation of the
 * permutation leg is exact (L = T', every LV live) this is the rotated, singular-value-scaled permuted x_weights, whose
 * column norms are the rotated perm_singval; everywhere else R_p^T V0 is the definition.  The observed statistic is
 * Z = x_weights[:, :m] * singvals[:m], the units of plsx_boot_weights_ci.  Both entries keep no state of a series, take
 * ANY index rows with values in 0 .. S - 1 and leave the permutation leg's routes alone.
 *
 *   plsx_perm_weights_build d_perm_idx (n, S) int32, d_V (T', m) fp64 row-major -> d_W [n][m][S]: the subject-space
 *                           operand of every permutation, Z_p = W_p . Xf with Xf the resample-independent feature
 *                           matrix of the binding (the per-cell scaled X in correlation mode, else the centred X).
 *                           Behavioral PLS (k_perm_W_behav): W_p[l][s] = sum_t V0[j T + t][l] z_p(s, t) over the T
 *                           behaviours of s's cell j, z_p the scaled z-score of row perm[s] of Y among the rows the
 *                           permutation places in the cell (centred only with PLSX_FLAG_COVARIANCE), divided by
 *                           n_j - 1: the moment loops of the permutation leg's builders in their order, t ascending.
 *                           Mean-centred PLS (k_perm_VA, k_perm_W_mc): R_p = A X[perm] with A the averaging weights
 *                           of the design, so W_p[l][perm[s]] = (V0^T A)[l][s]; rows that repeat in the index row
 *                           are added in position order, rows it skips get 0.  One writer per entry, a fixed order,
 *                           no floating-point atomics.
 *   plsx_perm_weights_test  the same operands in pieces of at most 16384 permutations, each piece through the counting
 *                           feature pass of plsx_simpls_coef_perm_test (k_coef_perm_prod over Xf with T := m, then
 *                           k_coef_perm_max; the kernels are unchanged), the features in chunks of whole 128-feature
 *                           blocks: d_count (B, m) int32 += #{p < n : q_f |Z_p[f][l]| >= q_f |d_obs[f][l]|}, d_max
 *                           (n, m) = max_f q_f |Z_p[f][l]|.  q_f = 1, or with `standardise` 1 / s_f, s_f the standard
 *                           deviation (ddof 1) of feature f over all S rows about its grand mean (k_col_rsd, once
 *                           per binding), and 0 for a feature without variance (its count is then n).  A piece's
 *                           operands (8 m S bytes a permutation) and partial maxima (8 m bytes a permutation and
 *                           feature block) stay inside the scratch budget and free device memory.  Integer counts,
 *                           maxima, one owner per (f, l): the same bits whatever the piece size and the chunking,
 *                           and counts / maxima of disjoint sets of index rows add / concatenate.
 *   plsx_perm_weights_scale d_rsd (B,) <- the table q_f = 1 / s_f that `standardise` applies (0 for a feature without
 *                           variance), so that a host forms the observed side of the family-wise comparison with the
 *                           scale the maxima carry.  PLSX_ERR_STATE without bound PLS-C data, PLSX_ERR_ARG for a null
 *                           pointer.
 *   Statuses (both): PLSX_ERR_STATE without bound data or with a regression binding; PLSX_ERR_UNSUPPORTED (context
 *   still usable) for a multiblock binding and, _test only, when not even 64 permutations fit (plsx_last_error names the
 *   bytes); PLSX_ERR_ARG for a null pointer, n < 1, m < 1 or m > T'.
 */
int plsx_perm_weights_build(plsx_ctx* ctx, const int32_t* d_perm_idx, int n, const double* d_V, int m, double* d_W,
                            void* stream);
int plsx_perm_weights_test(plsx_ctx* ctx, const int32_t* d_perm_idx, int n, const double* d_V, int m, const double* d_obs,
                           int standardise, int32_t* d_count, double* d_max, void* stream);
int plsx_perm_weights_scale(plsx_ctx* ctx, double* d_rsd, void* stream);

/*
 * Split-half reliability -- BasePLS.split_half (pyls/base.py:714-770) for np
 * data arrangements (the original data and/or permuted data, base.py:705-708)
 * with ns split masks each.  For every arrangement the library decomposes
 * the full sample on the device (U, d, V of THAT arrangement, as
 * _single_perm does), then for every split computes the two half-sample
 * cross-covariance matrices D1, D2 and
 *     ucorr = efficient_corr(D1.T @ V/d, D2.T @ V/d)     (over the B features)
 *     vcorr = efficient_corr(D1 @ U/d,  D2 @ U/d)        (over the T' rows)
 *   d_perm_idx (np, S) int32, or NULL = one un-permuted arrangement per entry
 *   d_masks    (np, ns, S) uint8, 1 = row belongs to the first half
 *   d_ucorr, d_vcorr (np, ns, L) out: per-split correlations (caller averages
 *              over the ns splits, base.py:770)
 */
int plsx_split_half_batch(plsx_ctx* ctx, const int32_t* d_perm_idx, int np,
                          const uint8_t* d_masks, int ns,
                          double* d_ucorr, double* d_vcorr, void* stream);
/* Same with the arrangements given as pre-permuted behaviour matrices
 * (`permindices=False`, pyls/base.py:691-692 then :705-708): d_ystack (np, S, T),
 * d_perm_idx must be NULL. */
int plsx_split_half_batch_y(plsx_ctx* ctx, const int32_t* d_perm_idx, const double* d_ystack, int np,
                            const uint8_t* d_masks, int ns,
                            double* d_ucorr, double* d_vcorr, void* stream);

/* Route of the LAST split-half pass on this context: 1 = one reader pass over the raw first-half sums of the splits
 * (behavioral PLS in correlation mode with T' = 17 .. 52 (every value), L = T' and <= 7 cells: the compact cross-product
 * blocks store C_1 once per split and ONE kernel rebuilds both z-scored halves from it and forms both products),
 * 0 = both halves written and read by two kernels (every other shape / mode, and option "split_two_readers").
 * Same statistics to rounding either way. */
int plsx_split_route(const plsx_ctx* ctx);

/* Mean over the splits of an arrangement -- the `.mean(axis=-1)` that closes BasePLS.split_half
 * (pyls/base.py:770): d_in (np, ns, L) as plsx_split_half_batch wrote it -> d_out (np, L); NaN propagates. */
int plsx_mean_splits(plsx_ctx* ctx, const double* d_in, int np, int ns, int L, double* d_out, void* stream);

/*
 * Cross-validation -- BehavioralPLS.crossval / _single_crossval
 * (pyls/types/behavioral.py:82-170) with compute.rescale_test
 * (pyls/compute.py:129-151): for each of m train/test splits decompose the
 * training rows on the device, z-map the test rows with the training feature
 * mean / std of their cell, predict Y and score the prediction.
 *   d_masks (m, S) uint8, 1 = training row (gen_splits(..., test_size))
 *   d_r, d_r2 (m, T) out: Pearson r (efficient_corr) and r^2
 *                  (sklearn r2_score, multioutput='raw_values') per behaviour
 */
int plsx_crossval_batch(plsx_ctx* ctx, const uint8_t* d_masks, int m, double* d_r, double* d_r2,
                        void* stream);

/*
 * Permutation null of the cross-validation (no reference counterpart; the rule of plsx_simpls_crossval_perm_batch):
 * the whole cross-validation above, under the same n splits, for each of m permutations of the rows of Y, averaged
 * over the splits in split order.  A permutation leaves the feature side of a fit untouched, so the call forms ONE
 * S x S matrix per split -- the Gram product of the rows of X centred and scaled by that split's per-cell training
 * mean / std inside the contraction (k_cvp_moments, k_cvp_gram; with covariance one matrix whose test rows alone are
 * scaled) -- and every (permutation, split) fit is S x S work: A, W' = A M^T, G = W' A^T, the small solver, the
 * scores.  A feature whose training rows of a cell all hold the same bits has scale 0 (k_cell_scale's rule).
 *   d_masks    (n, S) uint8, 1 = training row
 *   d_perm_idx (m, S) int32: row p of permutation i is row d_perm_idx[i][p] of Y; every row a permutation of 0 .. S-1
 *   d_r, d_r2  (m, T) out: the means over the n splits of Pearson r and r^2; a NaN score of one (permutation, split)
 *              makes that permutation's mean NaN
 * The caller passes ALL of its permutations in one call: a split's matrix is formed once per call and is not kept
 * between calls.  Splits and permutations run in groups sized by free device memory and the scratch budget; the
 * chunking of the contraction follows (S, B) alone, so the bits of a result depend neither on the groups nor on how
 * the permutations are cut into calls.  The context is left as found (the call maps and frees its own matrices).
 * PLSX_ERR_ARG: not a behavioural binding, null pointers, n < 1 or m < 1.  PLSX_ERR_UNSUPPORTED (context still
 * usable): multiblock PLS, contrasts set, or one split's matrices with one permutation's operands and the scores do
 * not fit free device memory and the scratch budget (the message has the sizes).
 */
int plsx_crossval_perm_batch(plsx_ctx* ctx, const uint8_t* d_masks, int n, const int32_t* d_perm_idx, int m,
                             double* d_r, double* d_r2, void* stream);

/*
 * Out-of-sample score correlation of the latent variables (no reference counterpart; the train / test statistic of
 * the PLS / CCA stability literature): plsx_crossval_batch plus, from the same pass -- the cross-product, the
 * decompositions and Q run once -- for every split and LV l the Pearson correlation, over ALL test rows of the split
 * in row order, of
 *   x_score[p][l] = the z_l the prediction uses (zmap of the test row by the training mean / std of its cell, projected
 *                   through U_live = R^T V_live / d_live; a cell-constant feature has scale 0), and
 *   y_score[p][l] = (y_p - training mean of its cell j) / training std (ddof = 1; covariance: not divided)
 *                   . V[jT .. (j+1)T, l]   -- the normalisation R was built with
 * (k_cv_lv, after k_cv_final).  Both scores flip with the sign of the training SVD: no alignment.  LV l is the l-th
 * largest singular value of the split's fit; a per-LV value is only as stable as the gap around that singular value.
 *   d_r, d_r2  (m, T) out: bit for bit those of plsx_crossval_batch on the same masks
 *   d_lv       (m, L) out: clamped to [-1, 1]; NaN for an LV that is not live (d_l <= PLSX_RANK_RTOL d_1) and where
 *              either score has no variance over the test rows (0 / 0)
 * The sums run in one fixed order (lane partials over ascending rows, an xor tree; no atomics).  Arguments, refusals
 * and error codes as plsx_crossval_batch, d_lv required.
 */
int plsx_crossval_lv_batch(plsx_ctx* ctx, const uint8_t* d_masks, int m, double* d_r, double* d_r2, double* d_lv,
                           void* stream);

/*
 * plsx_crossval_perm_batch plus the score correlations above of every (permutation, split) fit (k_cvp_lv, on the z
 * that the scoring kernel of the fit left; no further S x S or feature-sized work).
 *   d_r, d_r2   (m, T) out: bit for bit those of plsx_crossval_perm_batch on the same masks and permutations
 *   d_lv        (m, L) out: the means over the n splits, in split order; one NaN makes a permutation's mean NaN
 *   d_lv_pairs  (m, n, L) out or NULL: the value of every (permutation, split); with NULL they live in scratch of the call
 * The fixed summation order makes the bits independent of the groups of splits and permutations, of the scratch budget
 * and of how the permutations are cut into calls.  The size model counts (S, L) more per permutation of a pass and
 * (m, n, L) for the call.  Refusals and error codes as plsx_crossval_perm_batch (d_lv required); the context is left
 * as found.
 */
int plsx_crossval_perm_lv_batch(plsx_ctx* ctx, const uint8_t* d_masks, int n, const int32_t* d_perm_idx, int m,
                                double* d_r, double* d_r2, double* d_lv, double* d_lv_pairs, void* stream);

/*
 * Confound regression of behavioural PLS (no reference counterpart).  Z (S, q), 1 <= q <= 15; the design is
 * Z~ = [1, Z - zbar] (q' = q + 1 columns: one intercept and common slopes over the whole cohort, whatever the groups
 * and conditions; the per-cell centring of PLS-C follows as always).
 *
 * plsx_residualize: A <- A - Z~ (Z~^T Z~)^-1 Z~^T A, in place, for the ncols columns of d_A (S rows, pitch lda) --
 * stateless, no binding needed or touched (k_cf_ztilde, k_cf_chol, k_cf_resid: lanes over the columns, sums over the
 * rows in ascending order, no atomics).  d_slopes (q, ld) out or NULL: the slopes on Z - zbar.  The caller
 * residualises its device copies of X and Y BEFORE plsx_set_data, so that everything a binding derives (K, the
 * fixed-X operands, the scale tables) is built from the residuals and every entry -- decomposition, permutations,
 * bootstraps, split-half -- runs on (X_r, Y_r); the regression is not refitted per resample.
 * PLSX_ERR_ARG: null pointers, S < 1, ncols < 1, lda < ncols, q outside 1 .. 15, or a Cholesky pivot of Z~^T Z~ at or
 * below 1e-10 of its diagonal entry (rank deficiency): nothing is written.
 *
 * plsx_set_confounds: binds Z~ for the two fold entries below; plsx_set_data clears it.  PLSX_ERR_ARG for a binding
 * that is not behavioural, a null d_Z, q outside 1 .. 15, rank deficiency.
 *
 * plsx_crossval_confound_batch: cross-validation with the confound regression fitted on the TRAINING rows of every
 * split and applied to all its rows.  With D the training indicator of split s, P_s = (Z~^T D Z~)^-1 Z~^T D and
 * M_s = I - Z~ P_s, the scores are those of the cross-validation on (M_s X_r, M_s Y_r); M_s M = M_s, so the bound
 * residuals serve.  PLS-C scales every feature by its per-cell training standard deviation, so no update of an S x S
 * kernel carries over: X_s exists, for one group of splits at a time (k_cf_fold_prep, then k_cfb_fold_X: B_s = P_s X_r
 * with lanes over the features and up to 4 x 16 register accumulators over ascending rows, then the copies
 * X_s = X_r - Z~ B_s by plain stores, padding columns as zeros; X_r is read twice per four splits, each copy written
 * once).  Each split then runs the dual-space body of plsx_crossval_perm_batch on its own copy -- tables
 * (k_cvp_moments), the scaled S x S matrix (k_cvp_gram), A from Y_s = M_s Y_r (k_cf_fold_Y), the small solver, the
 * scores -- under the identity arrangement, which is why the identity column of the entry below repeats the split
 * mean of this one to the bit.
 *   d_masks (m, S) uint8, 1 = training row;  d_r, d_r2 (m, T) out;  d_lv (m, L) out or NULL: the score correlations
 *   of the latent variables, as plsx_crossval_lv_batch defines them, on the same fold data
 * plsx_crossval_confound_perm_batch: its permutation null, Y_{s,p} = M_s (Y_r[perm_p]) against X_s (the residualised
 * Y is permuted and residualised again per fold); arguments and outputs as plsx_crossval_perm_lv_batch, d_lv and
 * d_lv_pairs or both NULL.
 * Both: every sum in a fixed order, no atomics -- the bits depend neither on the group size, the scratch budget nor on
 * how the permutations are cut into calls.  The size model of plsx_crossval_perm_batch with 8 S Bpad more per split
 * (the fold copy) and 8 S T more per permutation; the group shrinks down to one split, then PLSX_ERR_UNSUPPORTED with
 * the sizes.  Refusals and error codes as the counterparts without confounds; PLSX_ERR_STATE when no confounds are
 * bound; PLSX_ERR_ARG, naming the split by its index in the call, when Z~ is rank deficient on the training rows of
 * a split (checked for all splits before anything else runs).  The context is left as found.
 * plsx_crossval_confound_group: splits per group of fold copies of the last such call.
 */
int plsx_residualize(plsx_ctx* ctx, double* d_A, int lda, int ncols, int S, const double* d_Z, int q, double* d_slopes,
                     int ld, void* stream);
int plsx_set_confounds(plsx_ctx* ctx, const double* d_Z, int q, void* stream);
int plsx_crossval_confound_batch(plsx_ctx* ctx, const uint8_t* d_masks, int m, double* d_r, double* d_r2, double* d_lv,
                                 void* stream);
int plsx_crossval_confound_perm_batch(plsx_ctx* ctx, const uint8_t* d_masks, int n, const int32_t* d_perm_idx, int m,
                                      double* d_r, double* d_r2, double* d_lv, double* d_lv_pairs, void* stream);
int plsx_crossval_confound_group(plsx_ctx* ctx);

/*
 * SIMPLS regression (pyls/types/regression.py:56-186, 248-373), solved per
 * resample in the S-dimensional dual space (K = X0 X0^T); k = n_components.
 *   plsx_simpls_decompose   original data: d_xwT (k, B) x_weights transposed,
 *                           d_pctvar (k,) variance of Y explained, d_cvec (T, k)
 *                           right singular vectors (sign rule input),
 *                           d_yload (T, k) = Y^T (X W)
 *   plsx_simpls_set_original  d_w0cT (k, B): column-centred original x_weights,
 *                           transposed -- sign reference of the bootstrap
 *                           (regression.py:317-320)
 *   plsx_simpls_perm_batch  PLSRegression._single_perm (regression.py:329-373):
 *                           d_perm_idx (n, S) permutes Y; d_out (n, k) pctvar of Y
 *   plsx_simpls_boot_batch  PLSRegression._single_boot (regression.py:279-327):
 *                           d_usum/d_usq (B, k) += sign-aligned x_weights (and
 *                           squares); d_yload (n, T, k) = Yi^T (Xi W).
 *                           d_ystack (n, S, T) or NULL: a Y matrix per bootstrap
 *                           (3-D Y aggregated over its resampled third axis,
 *                           regression.py:308-310); rows are still gathered with
 *                           d_boot_idx.
 *   plsx_simpls_set_row_masks  d_okx / d_oky (S,) uint8, 1 = the row of X / of Y
 *                           is usable; positions whose source row is an all-NaN
 *                           row are dropped per resample (get_mask,
 *                           regression.py:48-53).  NULL = all rows usable.  The
 *                           bound X / Y must hold zeros in the masked rows.
 *   plsx_simpls_crossval_batch  cross-validated prediction per component count
 *                           (the reference has none for PLSRegression,
 *                           regression.py:237-238; per split this follows
 *                           BehavioralPLS._single_crossval, behavioral.py:126-170,
 *                           with simpls in place of the SVD).  For each of m
 *                           splits: SIMPLS with k components on the training rows,
 *                           centred by the training means; the test rows predicted
 *                           by the first c = 1 .. k components plus the intercept
 *                           ([1, x] @ simpls(X_tr, Y_tr, c)['beta']); each
 *                           prediction scored per behaviour.
 *                           d_masks (m, S) uint8, 1 = training row; rows masked by
 *                           plsx_simpls_set_row_masks are on neither side.
 *                           d_r, d_r2 (m, k, T) out: Pearson r (efficient_corr) and
 *                           R^2 (sklearn r2_score, raw values) of the c-component
 *                           model; d_sse (m, k + 1, T) out: squared error summed
 *                           over the test rows, row 0 = intercept only (yhat = the
 *                           training mean).  Valid once plsx_set_data bound
 *                           regression data; PLSX_ERR_STATE otherwise.  Every split
 *                           needs >= 2 usable test rows and k <= n_train - 1 (the
 *                           caller checks).  Bit-reproducible run to run.
 *   plsx_simpls_crossval_perm_batch  the null of that cross-validation under
 *                           permuted Y: for each of m permutations and each of the
 *                           SAME n splits, SIMPLS with k components on the training
 *                           positions of (X, Y[perm]) -- X keeps its rows, position
 *                           p takes row perm[p] of Y, as plsx_simpls_perm_batch --
 *                           the test positions predicted and scored exactly as
 *                           plsx_simpls_crossval_batch scores them, against the
 *                           permuted Y; then the PLAIN MEAN over the n splits.
 *                           d_masks (n, S) uint8, 1 = training row; d_perm_idx
 *                           (m, S) int32, one permutation of 0 .. S-1 per row.
 *                           d_r, d_r2 (m, k, T) out: mean over the splits of the
 *                           test-row Pearson r / R^2 of the c-component model;
 *                           d_mse (m, k + 1) out: mean over the splits of
 *                           sum_t sse / n_test, row 0 = intercept only.  With row
 *                           masks a position is usable iff okx[p] and oky[perm[p]]
 *                           (get_mask(X, Y[perm])), so n_test belongs to the
 *                           (permutation, split) pair and the division is done
 *                           here; a pair with fewer than two usable test rows
 *                           gives NaN.  The m n fits (counted in 64 bits) run in
 *                           solver batches sized like plsx_simpls_crossval_batch's;
 *                           their Y sources and masks are expanded on the device
 *                           (k_sd_cvp_expand), scored by k_sd_cv_score<., true>
 *                           and reduced by k_sd_cvp_reduce: split by split in
 *                           ascending order, the running sum carried in the output
 *                           across solver batches, divided by n after the last --
 *                           no floating-point atomics, the same bits whatever the
 *                           batch size or the scratch budget (plsx_set_scratch) and
 *                           however the permutations are spread over contexts.
 *                           Per-fit scores exist in scratch of one batch only.
 *                           No bound on m beyond the outputs.  PLSX_ERR_STATE
 *                           without bound regression data; PLSX_ERR_ARG for a null
 *                           pointer, n < 1 or m < 1.
 *   plsx_simpls_crossval_nested_batch  nested cross-validation of the component
 *                           count (no reference counterpart): inner splits inside the
 *                           training rows of every outer split choose c, the outer
 *                           test rows -- which took no part in the choice -- score
 *                           the chosen model.  d_codes (n, 1 + ni, S) uint8 holds
 *                           CODES: 1 = training row, 0 = test row, 2 = on neither
 *                           side.  Row 0 of group s is outer split s (1 / 0 only),
 *                           rows 1 .. ni its inner folds: 2 on every outer test row,
 *                           1 / 0 on the outer training rows (the caller checks).
 *                           The solver includes a position iff its code is 1, the
 *                           scores take it iff its code is 0; the masks of every
 *                           other entry hold 0 / 1 and mean what they meant.  The
 *                           n (1 + ni) fits go through the fit-and-score body of
 *                           plsx_simpls_crossval_batch; then, per group
 *                           (k_sd_cvn_select, one wavefront, no atomics),
 *                             inner_mse[c] = mean over the ni inner folds, ascending,
 *                               of sum_t sse[c][t] / n_test of the fold, c = 0 .. k
 *                               (row 0 the intercept-only model);
 *                             best = 1; for c = 2 .. k: if inner_mse[c] <
 *                               inner_mse[best]: best = c -- the first minimum, a NaN
 *                               is never smaller, c = 0 is no candidate;
 *                             ncomp = best, or 0 where inner_mse[best] is not finite:
 *                               the group is undefined and its scores are NaN.
 *                           d_r, d_r2 (n, T) out: the outer fit's test-row Pearson r
 *                           / R^2 at c = ncomp; d_mse (n,) its sum_t sse / n_test;
 *                           d_ncomp (n,) int32; d_inner_mse (n, k + 1).
 *   plsx_simpls_crossval_nested_perm_batch  its null under permuted Y: the WHOLE
 *                           procedure, selection included, for each of m
 *                           permutations (d_perm_idx (m, S) int32, as
 *                           plsx_simpls_crossval_perm_batch; usability is that of
 *                           the (permutation, fit) pair), each outer split scored at
 *                           the c selected inside that permutation; then the plain
 *                           mean over the n outer splits.  d_r, d_r2 (m, T), d_mse
 *                           (m,) out; d_ncomp_count (m, k) int32 out: how many outer
 *                           splits of permutation i chose c (an undefined group
 *                           counts nowhere and makes the means NaN).  Fit f =
 *                           ((permutation, outer split), member), counted in 64
 *                           bits, member 0 the outer fit (k_sd_cvn_expand).  Solver
 *                           batches hold whole groups of 1 + ni fits, sized like
 *                           plsx_simpls_crossval_perm_batch's, so the selection runs
 *                           next to the fits; k_sd_cvn_reduce adds a permutation's
 *                           groups in outer-split order into the running sums
 *                           carried in the outputs and divides by n after the last:
 *                           the same bits whatever the batch size or the scratch
 *                           budget and however the permutations are spread over
 *                           contexts.
 *                           Both nested entries: PLSX_ERR_STATE without bound
 *                           regression data or while a series of counts per split
 *                           (plsx_simpls_cv_class_begin / _auc_begin) is open -- the
 *                           nested counts have their own, plsx_simpls_cvn_class_begin;
 *                           PLSX_ERR_ARG for a null pointer or n, ni, m < 1;
 *                           PLSX_ERR_UNSUPPORTED, the context still usable, with
 *                           bound confounds and when one group of 1 + ni fits does
 *                           not fit half the scratch budget (the message has the
 *                           sizes).
 *   plsx_simpls_set_confounds  confound regression (no reference counterpart):
 *                           d_Z (S, q) nuisance variables, 1 <= q <= 15.  Call it
 *                           after plsx_set_data(PLSX_REGRESSION) and, with masked
 *                           rows, after plsx_simpls_set_row_masks (a row counts as
 *                           usable iff okx and oky say so; Z must be finite there).
 *                           Forms Z~ = [1, Z - zbar] over the usable rows and
 *                           residualises the bound Xc and Y in place, X_r = M X,
 *                           Y_r = M Y with M = I - Z~ (Z~^T Z~)^-1 Z~^T (k_cf_resid:
 *                           lanes over the features, sums over the rows in
 *                           ascending order, no atomics; masked rows are written as
 *                           zeros); d_gx (q, B) / d_gy (q, T) out, or NULL: the
 *                           slopes of X / Y on Z - zbar.  K is then formed again
 *                           from X_r (not updated: the update cancels where the
 *                           confounds carry most of the variance) and Z~ is kept
 *                           for the fold entries below.  Every entry that follows
 *                           -- decomposition, permutations, bootstraps, split-half,
 *                           the coefficient and VIP series -- runs on (X_r, Y_r);
 *                           the confound regression is not refitted per resample.
 *                           PLSX_ERR_STATE without bound regression data;
 *                           PLSX_ERR_ARG for a null d_Z, q outside 1 .. 15 or a
 *                           Cholesky pivot of Z~^T Z~ at or below 1e-10 of its
 *                           diagonal entry (rank deficiency; the bound data are
 *                           then untouched).  plsx_set_data clears it.
 *   plsx_simpls_crossval_confound_batch  plsx_simpls_crossval_batch with the
 *                           confound regression fitted on the training rows of
 *                           every split and applied to all its rows
 *                           (cross-validated confound regression): with D the
 *                           training indicator of split s, P_s = (Z~^T D Z~)^-1
 *                           Z~^T D and M_s = I - Z~ P_s, the fit and its scores are
 *                           those of plsx_simpls_crossval_batch on (M_s X, M_s Y).
 *                           M_s M = M_s, so the bound residuals serve; nothing
 *                           B-sized is touched: K_s = M_s K_r M_s^T = K_r - Z~ F_s^T
 *                           - F_s Z~^T with C_s = K_r P_s^T, E_s = P_s C_s,
 *                           F_s = C_s - Z~ E_s / 2 (k_cf_fold_prep, one k_nt_gemm,
 *                           k_cf_fold_F, k_cf_fold_K) and Y_s = M_s Y_r
 *                           (k_cf_fold_Y) go to the solver as the fit's own K and
 *                           Y.  Arguments and outputs as plsx_simpls_crossval_batch;
 *                           the test rows are scored on the fold-residualised Y.
 *                           Splits go in groups of as many K_s (8 S^2 bytes each,
 *                           with one fit's state) as fit half the scratch budget.
 *                           An open series of counts (PLS-DA) is not supported:
 *                           PLSX_ERR_STATE.
 *   plsx_simpls_crossval_confound_perm_batch  its null under permuted Y, as
 *                           plsx_simpls_crossval_perm_batch: Freedman-Lane's
 *                           arrangement (I - M) Y + Y_r[perm] collapses under M_s to
 *                           Y_{s,p} = M_s (Y_r[perm_p]) -- the residualised Y is
 *                           permuted and residualised again per fold.  The fits of
 *                           one split share K_s; a solver batch is [splits of a
 *                           group][permutations of a chunk].  Splits are processed
 *                           in ascending order, each permutation's running sum is
 *                           carried in the output and divided by n after the last
 *                           split (k_cf_cvp_acc: no atomics), so a call repeats to
 *                           the bit.  Row masks must not be bound with it (the
 *                           caller refuses).  Outputs as
 *                           plsx_simpls_crossval_perm_batch.
 *                           Both fold entries: PLSX_ERR_STATE before
 *                           plsx_simpls_set_confounds; PLSX_ERR_ARG for a null
 *                           pointer, n < 1, m < 1, or a split on whose training
 *                           rows Z~ is rank deficient (named in the message);
 *                           PLSX_ERR_UNSUPPORTED, the context still usable, on the
 *                           global route of the solver (the simpls_global option or
 *                           S beyond the on-chip bound: K_s would be gigabytes a
 *                           split) and when one K_s plus one fit does not fit half
 *                           the scratch budget.
 *   plsx_simpls_split_half_batch  split-half reliability of the SIMPLS components
 *                           (BasePLS.split_half, pyls/base.py:366-397, with SIMPLS
 *                           in place of the SVD): for each of np arrangements
 *                           (X, Y[perm]) -- d_perm_idx (np, S) int32, or NULL: the
 *                           identity, the observed data, for every arrangement --
 *                           SIMPLS with k components on all usable
 *                           rows gives W (B, k) and Q = y_loadings (T, k); each of
 *                           the arrangement's ns masks, d_masks (np, ns, S) uint8,
 *                           1 = first half, splits the usable rows into halves with
 *                           D_h = (Y_h - ybar_h)^T (X_h - xbar_h), and
 *                           d_ucorr[p][s][c] = efficient_corr(D_1^T q_c, D_2^T q_c)
 *                           over the B features, d_vcorr[p][s][c] =
 *                           efficient_corr(D_1 w_c, D_2 w_c) over the T behaviours
 *                           ((np, ns, k) each, the layout plsx_split_half_batch
 *                           writes; plsx_mean_splits averages them).  Nothing
 *                           B-sized is formed: D_h^T q_c = Xc^T g_{h,c} with g the
 *                           half-centred Y q_c, so ucorr follows from g_1^T K g_2,
 *                           g_h^T K g_h and g_h^T r (K = Xc Xc^T, r = Xc 1_B), two
 *                           products with K per (split, component), 4 S^2 k flop
 *                           per split.  With row masks a position is usable iff
 *                           okx[p] and oky[perm[p]]; unusable rows are in neither
 *                           half.  A side without variance gives NaN (T = 1:
 *                           vcorr).  Arrangements run in solver batches; the splits
 *                           of an arrangement go in groups where they do not fit
 *                           half the scratch budget (plsx_set_scratch) at once;
 *                           PLSX_ERR_UNSUPPORTED when one split does not.  Every
 *                           (arrangement, split) is computed on its own, in fixed
 *                           order, without atomics.  PLSX_ERR_STATE without bound
 *                           regression data; PLSX_ERR_ARG for a null pointer,
 *                           np < 1 or ns < 1.
 *   plsx_simpls_coef_begin / plsx_simpls_coef_finish
 *                           a coefficient series that rides along the bootstrap
 *                           batches: the model of the first c components,
 *                           Y ~ intercept + X . coefs, coefs = W[:, :c] Q[:, :c]^T
 *                           (B, T) with Q the simpls y_loadings of the resample
 *                           (beta of regression.py:149-151 without its intercept
 *                           row).  While a series is open every solver batch of
 *                           plsx_simpls_boot_batch also writes
 *                           A_b = sum_{j <= c} wd_j q_j^T dense in subject space
 *                           (kernel k_sd_coef; coefs_b = Xc^T A_b) and accumulates
 *                           sum_b A_b (T, S) and C_t = sum_b a_bt a_bt^T (T, S, S);
 *                           _finish passes the features ONCE:
 *                           d_bsum (B, T) += sum_b coefs_b = Xc^T sum_b A_b,
 *                           d_bsq (B, T) += sum_b coefs_b^2, [f][t] = x_f^T C_t x_f.
 *                           coefs depend on neither the signs nor the order of the
 *                           components: no alignment.  Everything else a batch
 *                           computes keeps its bits, on either route of the weights
 *                           (option quad_sums); row masks and d_ystack apply as ever.
 *                           Limits: _begin returns PLSX_ERR_ARG for c outside
 *                           1 .. k, PLSX_ERR_STATE without bound regression data or
 *                           before plsx_simpls_set_original, PLSX_ERR_UNSUPPORTED
 *                           (context still usable) when 8 T S^2 bytes plus the
 *                           partial tiles of the S x S products (16 T S^2) do not
 *                           fit in free device memory next to K or in the scratch
 *                           budget (plsx_set_scratch), or S > 23168.  _finish
 *                           without an open series: PLSX_ERR_STATE.  plsx_set_data
 *                           and plsx_simpls_set_original end an open series.
 *                           Fixed-order reductions: bit-reproducible run to run.
 *   plsx_simpls_coef_keep / plsx_simpls_coef_ci
 *                           percentile intervals of the coefficients.  The sums above
 *                           are quadratic forms; order statistics are not: they need
 *                           every bootstrap's coefs_b[f][t] = sum_s Xc[s][f] A_b[t][s].
 *                           _keep (after _begin, before the first batch of the
 *                           series): every bootstrap the open series sees is also
 *                           kept, appended in submission order to the caller's
 *                           d_A, `capacity` bootstraps of T S doubles, layout
 *                           [bootstrap][T][S] (bootstrap-major, so that shards of
 *                           several contexts concatenate; k_sd_coef writes each
 *                           A_b there instead of into scratch, the sums keep their
 *                           bits).  A plsx_simpls_boot_batch whose bootstraps no
 *                           longer fit returns PLSX_ERR_ARG before it computes
 *                           anything; _keep without an open series:
 *                           PLSX_ERR_STATE; _finish, plsx_set_data,
 *                           plsx_simpls_set_original and _begin end the keeping
 *                           with the series (the buffer stays the caller's).
 *                           _ci is stateless with respect to the series: for ANY
 *                           stack d_A [n][T][S] and the bound, centred features it
 *                           writes d_lo, d_hi (B, T): the two interpolated order
 *                           statistics -- virtual indices (i, g) as for
 *                           plsx_percentile_ci -- of { coefs_b[f][t] : b < n }.
 *                           Features go in chunks of whole 128-feature blocks;
 *                           per chunk kernel k_coef_prod (fp64 MFMA, M = features,
 *                           N = bootstraps of one behaviour, K = subjects) writes
 *                           the series [f][t][n] contiguous and the selection
 *                           kernels of plsx_percentile_ci reduce them (option
 *                           percentile_sort applies): the (B, T, n) array never
 *                           exists whole.  A chunk is at most 2 GB and, with the
 *                           stack, stays inside the scratch budget
 *                           (plsx_set_scratch) and free device memory.  Every
 *                           entry is one block's contraction in ascending s: the
 *                           same bits run to run and whatever the chunking.
 *                           Limits: PLSX_ERR_UNSUPPORTED (context still usable,
 *                           sizes in the message) for n > 16384 or when the stack
 *                           plus the smallest chunk (min(B, 128) features,
 *                           8 T n bytes each) does not fit; PLSX_ERR_ARG for
 *                           n < 1, an index outside 0 .. n - 1, a null pointer;
 *                           PLSX_ERR_STATE without bound regression data.
 *   plsx_simpls_vip_keep / plsx_simpls_vip_ci
 *                           bootstrap standard errors and percentile intervals of
 *                           the VIP scores (variable importance in projection) of
 *                           the c-component model,
 *                           VIP[f] = sqrt(B sum_a ssq_a w[f][a]^2 / |w_a|^2 / sum_a ssq_a),
 *                           ssq_a = |y_loadings[:, a]|^2 (simpls' own), a < c.  A
 *                           square root of a sum of squares over the components:
 *                           no quadratic form of anything, so its spread needs
 *                           every bootstrap's value per feature.
 *                           _keep (after plsx_simpls_set_original): every
 *                           bootstrap that later plsx_simpls_boot_batch calls
 *                           solve is appended in submission order to the caller's
 *                           d_G, `capacity` bootstraps of c S doubles, layout
 *                           [bootstrap][c][S] (bootstrap-major, so that shards of
 *                           several contexts concatenate).  Row a of bootstrap b
 *                           is sqrt(ssq_a / (|w_a|^2 sum_j ssq_j)) a_a, a_a the dual
 *                           weight of component a scattered to subject space
 *                           (kernel k_sd_vip, one wavefront per bootstrap after the
 *                           solver chain; |w_a|^2 = a_a^T K a_a is taken from the
 *                           solver's own K_r wd_a, 2 S flop per component), so that
 *                           VIP_b[f]^2 = B sum_a (sum_s Xc[s][f] G_b[a][s])^2.
 *                           Independent of a coefficient series: both may be open,
 *                           neither moves the other's bits, and everything else a
 *                           batch computes keeps its bits on either route of the
 *                           weights.  A plsx_simpls_boot_batch whose bootstraps no
 *                           longer fit returns PLSX_ERR_ARG before it computes
 *                           anything; _keep returns PLSX_ERR_STATE without bound
 *                           regression data or before plsx_simpls_set_original,
 *                           PLSX_ERR_ARG for c outside 1 .. k, a null buffer or
 *                           capacity < 1.  plsx_set_data, plsx_simpls_set_original
 *                           and a second _keep end the keeping (the buffer stays
 *                           the caller's).
 *                           _ci is stateless: for ANY stack d_G [n][c][S] and the
 *                           bound, centred features it writes, per feature, d_sd
 *                           (B,): the standard deviation with n - 1 in the
 *                           denominator (NaN for n = 1), and d_lo, d_hi (B,): the
 *                           two interpolated order statistics -- virtual indices
 *                           (i, g) as for plsx_percentile_ci -- of
 *                           { VIP_b[f] : b < n }.  Features go in chunks of whole
 *                           128-feature blocks; per chunk kernel k_vip_prod (fp64
 *                           MFMA, M = features, N = bootstraps, K = subjects, the
 *                           block loops over the c components and squares each
 *                           finished contraction into a second register tile)
 *                           writes the series [f][n] contiguous, k_vip_moments
 *                           (two passes: mean, then squared deviations) and the
 *                           selection kernels of plsx_percentile_ci reduce them:
 *                           the (B, n) array never exists whole.  A chunk is at
 *                           most 2 GB and, with the stack, stays inside the
 *                           scratch budget and free device memory.  Every entry
 *                           is one block's work in ascending s and a, every
 *                           reduction has one fixed order: the same bits run to
 *                           run and whatever the chunking.  Limits:
 *                           PLSX_ERR_UNSUPPORTED (context still usable, sizes in
 *                           the message) for n > 16384 or when the stack plus the
 *                           smallest chunk (min(B, 128) features, 8 n bytes each)
 *                           does not fit; PLSX_ERR_ARG for n < 1, c < 1, an index
 *                           outside 0 .. n - 1, a null pointer; PLSX_ERR_STATE
 *                           without bound regression data.
 *   plsx_simpls_coef_perm_test / plsx_simpls_coef_perm_begin / plsx_simpls_coef_perm_end
 *                           permutation test of the coefficients of the c-component
 *                           model: per (feature, behaviour) the number of
 *                           permutations whose coefficient is at least as large in
 *                           magnitude as the observed one, and per (permutation,
 *                           behaviour) the maximum over the features of the
 *                           standardised magnitude (the null of the single-step
 *                           maxT statistic of Westfall & Young).  Counts add over
 *                           permutations and a maximum over features belongs to one
 *                           permutation: no coefficient is ever stored.
 *                           _test is stateless: for ANY stack d_A [n][T][S] and the
 *                           bound, centred features, with
 *                           coef_b[f][t] = sum_s Xc[s][f] A[b][t][s] (contracted in
 *                           ascending s) and s_f = sqrt(sum_s Xc[s][f]^2 / (n_x - 1))
 *                           (n_x the usable rows of X) when `standardise` is set,
 *                           else 1: d_count (B, T) int32 += #{b < n :
 *                           s_f |coef_b[f][t]| >= s_f |d_obs[f][t]|} (>=, so that a
 *                           feature without variance counts every permutation),
 *                           d_max (n, T) = max_f s_f |coef_b[f][t]|.  Kernel
 *                           k_coef_perm_prod has k_coef_prod's tiling (fp64 MFMA,
 *                           M = 128 features, N = 64 permutations of one behaviour,
 *                           K = subjects); a block walks all the tiles of its
 *                           (128 features, t), counts in registers and stores the
 *                           per-tile maxima of its 128 features; k_coef_perm_max
 *                           reduces them over the feature blocks.  The stack goes
 *                           in pieces of at most 16384 permutations, the features
 *                           in chunks of whole 128-feature blocks whose partial
 *                           maxima (8 T n bytes per block) fit 2 GB and, next to
 *                           the stack, the scratch budget (plsx_set_scratch) and
 *                           free device memory.  Integer counts, maxima, one owner
 *                           per (f, t), no atomics: the same bits run to run and
 *                           whatever the chunking.  No bound on n beyond the
 *                           outputs.  PLSX_ERR_ARG for a null pointer or n < 1,
 *                           PLSX_ERR_STATE without bound regression data,
 *                           PLSX_ERR_UNSUPPORTED (context still usable) when not
 *                           even one block of 64 permutations fits.
 *                           _begin (after plsx_simpls_set_original) opens a series
 *                           that rides along plsx_simpls_perm_batch: every solver
 *                           batch runs with the dual weights on (they stay in the
 *                           batch's state; d_out keeps its bits), k_sd_coef writes
 *                           A_p = sum_{j < c} wd_j q_j^T of its permutations into
 *                           scratch (T S doubles each, counted in the batch's share
 *                           of the scratch budget: the batch shrinks, the scratch
 *                           does not grow), the test above runs on that piece
 *                           against d_obs, adds to d_count and appends the maxima
 *                           to d_max (capacity, T) in submission order.  s_f is
 *                           computed once, in _begin.  A batch that would pass
 *                           `capacity` returns PLSX_ERR_ARG before it computes
 *                           anything.  _end, plsx_set_data,
 *                           plsx_simpls_set_original and a second _begin end the
 *                           series (the buffers stay the caller's).  _begin:
 *                           PLSX_ERR_ARG for c outside 1 .. k, a null pointer or
 *                           capacity < 1; PLSX_ERR_STATE without bound regression
 *                           data or before plsx_simpls_set_original.
 *   plsx_simpls_vip_perm_test / plsx_simpls_vip_perm_begin / plsx_simpls_vip_perm_end
 *                           permutation test of the VIP scores of the c-component
 *                           model: per feature the number of permutations whose
 *                           score is at least the observed one (one-sided: VIP is
 *                           non-negative and large means important), and per
 *                           permutation the maximum of its scores over the features
 *                           (the null of the single-step maxT statistic; VIP is
 *                           comparable across features, no scale enters).  No score
 *                           is ever stored.
 *                           _test is stateless: for ANY stack d_G [n][c][S] (the
 *                           layout of plsx_simpls_vip_keep) and the bound, centred
 *                           features, with v_b[f] = sqrt(B sum_a (sum_s Xc[s][f]
 *                           G[b][a][s])^2) -- the bits k_vip_prod writes for the
 *                           same stack row --: d_count (B,) int32 += #{b < n :
 *                           v_b[f] >= d_obs[f]}, d_max (n,) = max_f v_b[f].  A
 *                           permutation whose rows are NaN (a degenerate fit: the
 *                           formula's 0 / 0) counts nowhere and leaves its maximum
 *                           at 0, below every real fit's (sum_f v^2 = B, so
 *                           max_f v >= 1); a NaN in d_obs counts nowhere.  Kernel
 *                           k_vip_perm_prod has k_vip_prod's tiling and loop (fp64
 *                           MFMA, M = 128 features, N = 64 permutations,
 *                           K = subjects, each component's finished contraction
 *                           squared into a second register tile); a block walks a
 *                           run of consecutive tiles of its 128 features -- runs
 *                           sized so that a chunk launches about 8192 blocks: a
 *                           block per whole piece would leave ceil(B / 128) blocks,
 *                           5 at B = 600 --, counts in registers, stores its counts
 *                           per (run, feature) and the per-tile maxima of its 128
 *                           features; k_vip_perm_count adds the runs of a feature,
 *                           k_coef_perm_max (T = 1) reduces the maxima over the
 *                           feature blocks.  The stack goes in pieces of at most 16384
 *                           permutations, the features in chunks of whole
 *                           128-feature blocks whose partial maxima (8 n bytes per
 *                           block) fit 2 GB and, next to the stack, the scratch
 *                           budget and free device memory.  Integer counts, maxima,
 *                           one owner per feature, no atomics: the same bits run to
 *                           run and whatever the chunking.  PLSX_ERR_ARG for a null
 *                           pointer, n < 1 or c outside 1 .. k, PLSX_ERR_STATE
 *                           without bound regression data, PLSX_ERR_UNSUPPORTED
 *                           (context still usable, sizes in the message) when not
 *                           even one block of 64 permutations fits.
 *                           _begin (after plsx_simpls_set_original) opens a series
 *                           that rides along plsx_simpls_perm_batch, next to an
 *                           open coefficient series or without one: every solver
 *                           batch runs with the dual weights on (d_out keeps its
 *                           bits), k_sd_vip writes the scaled dual weights of its
 *                           permutations into scratch (c S doubles each, counted in
 *                           the batch's share of the scratch budget), the test
 *                           above runs on that piece against d_obs, adds to d_count
 *                           and appends the maxima to d_max (capacity,) in
 *                           submission order.  A batch that would pass `capacity`
 *                           returns PLSX_ERR_ARG before it computes anything.
 *                           _end, plsx_set_data, plsx_simpls_set_original and a
 *                           second _begin end the series (the buffers stay the
 *                           caller's).  _begin: PLSX_ERR_ARG for c outside 1 .. k,
 *                           a null pointer or capacity < 1; PLSX_ERR_STATE without
 *                           bound regression data or before
 *                           plsx_simpls_set_original.
 *   plsx_simpls_set_classes / plsx_simpls_cv_class_begin / plsx_simpls_cv_class_end
 *                           PLS discriminant analysis: the bound Y is the indicator
 *                           matrix of G = T classes minus its column means over all
 *                           S rows (the class frequencies n_g / S), and the
 *                           cross-validation also classifies its test rows.
 *                           _set_classes binds one class code 0 .. G - 1 per row of
 *                           the bound regression data, d_class (S,) int32 on the
 *                           device; the context keeps its own copy.  PLSX_ERR_STATE
 *                           without bound regression data, PLSX_ERR_ARG for G != T
 *                           or a code outside 0 .. G - 1 (checked on the host),
 *                           PLSX_ERR_UNSUPPORTED (context still usable) for G > 32,
 *                           the bound of the kernel below.  plsx_set_data clears the
 *                           binding, and so does a null d_class.
 *                           _begin (after _set_classes) opens a series that rides
 *                           along the two cross-validation entries, so that no fit is
 *                           solved twice: while it is open every
 *                           plsx_simpls_crossval_batch of m splits appends m blocks
 *                           [k][G][G] of int32 to d_conf in submission order --
 *                           block[c - 1][g][h] the usable test rows of true class g
 *                           that the first c components predict as class h -- and
 *                           every plsx_simpls_crossval_perm_batch of m permutations
 *                           appends m blocks, each the SUM over that call's n splits
 *                           (the true class of position p is that of row perm[p];
 *                           usability as that entry defines it).  The predicted
 *                           class is the first maximum over g of
 *                           yhat_c[p][g] = n_g / S + ybar_tr[g] + sum_{j <= c} t_j[p] q_j[g],
 *                           the prediction the entries score plus the column mean
 *                           that the centring took away, i.e. the prediction of the
 *                           RAW indicators (lowest index on a tie: numpy's argmax).  Kernel k_sd_cv_class runs after
 *                           k_sd_cv_score on the scores that kernel centred in place:
 *                           one wavefront per fit, lanes over positions; per
 *                           component count the y-loadings q_c come from the sums of
 *                           the scores over the training positions of every class
 *                           (the bound Y being what it is, Y0 = [class] - frequency:
 *                           one pass over the scores, Y0 is not read; registers,
 *                           reduced four at a time in fixed order), the running
 *                           prediction of a position lives in the fit's idle solver
 *                           scratch, the G x G counters of the open c in the wave's
 *                           LDS slice, added to the block with integer atomics.  A
 *                           bound Y that is NOT the indicator matrix of d_class
 *                           minus its column means gives counts that mean nothing.  A block is zeroed when it is appended; counts
 *                           are integers, so the result does not depend on the order
 *                           in which a permutation's splits arrive, on the batch
 *                           size, the scratch budget or the route of the solver.
 *                           d_r, d_r2, d_sse / d_mse of both entries keep their bits
 *                           with the series open.  A call that would pass `capacity`
 *                           (blocks) returns PLSX_ERR_ARG before it computes
 *                           anything.  _end, plsx_set_data, plsx_simpls_set_classes
 *                           and a second _begin end the series (the buffer stays the
 *                           caller's).  _begin: PLSX_ERR_STATE without bound
 *                           regression data or before plsx_simpls_set_classes,
 *                           PLSX_ERR_ARG for a null buffer or capacity < 1.
 *   plsx_simpls_cv_auc_begin / plsx_simpls_cv_auc_end
 *                           The area under the ROC curve of every class against the
 *                           rest, from the same predictions: a second series with
 *                           the rules of plsx_simpls_cv_class_begin, independent of
 *                           it (none, either or both may be open).  While it is open
 *                           every plsx_simpls_crossval_batch of m splits appends m
 *                           blocks [k][G][2] of int64 to d_auc in submission order,
 *                           and every plsx_simpls_crossval_perm_batch of m
 *                           permutations appends m blocks, each the SUM over that
 *                           call's n splits.  With pos the usable test positions of
 *                           a fit whose true class is g (under a permutation that of
 *                           row perm[p]), neg its other usable test positions and
 *                           v[p] = yhat_c[p][g], the prediction of the raw indicator
 *                           that k_sd_cv_class takes the argmax of,
 *                             block[c - 1][g][0] = u2    = sum over i in pos, j in neg of
 *                                                          2 if v[i] > v[j], 1 if v[i] == v[j], else 0
 *                             block[c - 1][g][1] = pairs = |pos| |neg|
 *                           so that AUC = u2 / (2 pairs): Mann-Whitney, ties one
 *                           half.  A comparison with a NaN prediction is false both
 *                           ways: such a pair stays in `pairs` and adds nothing to
 *                           u2.  The counts are 64-bit: a permutation's sum over 100
 *                           splits at S = 20 000 passes 2^31.  Kernel k_sd_cv_auc
 *                           runs after k_sd_cv_score (and after k_sd_cv_class where
 *                           that series is open too): one wavefront per fit; it
 *                           lists the usable test positions class by class once,
 *                           forms q_c and the running prediction of the listed
 *                           positions as k_sd_cv_class does (the fit's idle solver
 *                           scratch), and per class lets the lanes own the positives
 *                           and walk the negatives, staged 64 at a time in the
 *                           wave's LDS slice; per-lane integer counts, a 64-bit wave
 *                           reduction and one 64-bit integer atomic per count.  A
 *                           block is zeroed when it is appended; the counts are
 *                           integers, so the result does not depend on the order in
 *                           which a permutation's splits arrive, on the batch size,
 *                           the scratch budget or the route of the solver.  d_r,
 *                           d_r2, d_sse / d_mse of both entries and the blocks of an
 *                           open confusion series keep their bits with the series
 *                           open.  A call that would pass `capacity` (blocks) of
 *                           either open series returns PLSX_ERR_ARG before it
 *                           computes anything or zeroes a block.  _end,
 *                           plsx_set_data, plsx_simpls_set_classes and a second
 *                           _begin end the series (the buffer stays the caller's).
 *                           _begin: PLSX_ERR_STATE without bound regression data or
 *                           before plsx_simpls_set_classes, PLSX_ERR_ARG for a null
 *                           buffer or capacity < 1.
 *   plsx_simpls_cv_pred_begin / plsx_simpls_cv_pred_end
 *                           The out-of-fold predictions themselves: a third series,
 *                           independent of the two series of counts.  While it is
 *                           open every plsx_simpls_crossval_batch and every
 *                           plsx_simpls_crossval_confound_batch of m splits appends m
 *                           slots [T][S] of doubles to d_pred in submission order,
 *                           and every plsx_simpls_crossval_nested_batch of n outer
 *                           splits n slots, those of its OUTER fits.  slot[t][p] is
 *                           the prediction of behaviour t at row p by the model of
 *                           c components fitted on the split's training rows,
 *                             ybar_tr[t] + sum_{j <= c} t_j[p] q_j[t]
 *                           -- [1, x_p] @ simpls(X_tr, Y_tr, c)['beta'] in the units
 *                           of the bound (globally centred, on the confound route
 *                           fold-residualised) Y -- on the usable test rows of the
 *                           split and NaN on every other row: all S T entries of a
 *                           slot are written.  After plsx_simpls_set_classes the
 *                           slot holds the prediction of the RAW indicators
 *                           (f + sum z_c q_c), the values k_sd_cv_class takes the
 *                           argmax of and k_sd_cv_auc ranks.  c = 1 .. k is the
 *                           count of every slot; c = 0 takes, per outer fit of the
 *                           nested entry, the count its selection has just chosen
 *                           (read on the device; an undefined group, count 0, gets
 *                           an all-NaN slot) -- the other two entries then return
 *                           PLSX_ERR_ARG.  d_ncomp [capacity] int32 or NULL: the
 *                           count used for every slot.  d_true [capacity][T][S] or
 *                           NULL: the rows of the fit's own Y at the same positions
 *                           (on the confound route the fold-residualised Y, which
 *                           exists on the device only), NaN elsewhere.  Kernel
 *                           k_sd_cv_pred runs behind k_sd_cv_score (and behind
 *                           k_sd_cv_class / k_sd_cv_auc / k_sd_cvn_select where they
 *                           run): one wavefront per kept fit, lanes over positions,
 *                           no LDS on either solver route; q_j[t] and the update go
 *                           through the device functions of k_sd_cv_score and
 *                           k_sd_cv_class, so the values are the ones those kernels
 *                           scored and do not depend on the batch size, the scratch
 *                           budget or where a call ends.  The permutation entries
 *                           append nothing, and every output of every entry keeps its
 *                           bits with the series open.  A call that would pass
 *                           `capacity` (slots) returns PLSX_ERR_ARG before it
 *                           computes or writes anything.  _end, plsx_set_data and a
 *                           second _begin end the series (the buffers stay the
 *                           caller's).  _begin: PLSX_ERR_STATE without bound
 *                           regression data, PLSX_ERR_ARG for a null stack,
 *                           capacity < 1 or c outside 0 .. k, PLSX_ERR_UNSUPPORTED
 *                           (context still usable, sizes in the message) for a
 *                           stack -- 8 S T capacity bytes, twice that with d_true --
 *                           beyond the scratch budget.
 *   plsx_simpls_cvn_class_begin / plsx_simpls_cvn_class_end
 *                           PLS discriminant analysis under the nested entries
 *                           (after plsx_simpls_set_classes): the selection runs on
 *                           COUNTS and the selected counts come back.  While the
 *                           series is open every fit of
 *                           plsx_simpls_crossval_nested_batch / _perm_batch is also
 *                           classified by k_sd_cv_class (and, d_auc given, ranked by
 *                           k_sd_cv_auc) into a block of its own in the batch's
 *                           scratch, [k][G][G] int32 and [k][G][2] int64 per fit,
 *                           which count towards the batch size and the
 *                           one-group-must-fit refusal.  Then, per group
 *                           (k_sd_cvn_class_select in place of k_sd_cvn_select, one
 *                           wavefront, no atomics), for c = 1 .. k
 *                             pooled[c] = sum over the ni inner folds, ascending, of
 *                               the fold's block at c (integers);
 *                             PLSX_CVN_SELECT_ACCURACY: crit[c] = trace / total of
 *                               pooled[c], one division;
 *                             PLSX_CVN_SELECT_BALANCED: crit[c] = the recalls
 *                               pooled[g][g] / rowsum_g of the classes with
 *                               rowsum_g > 0, added one by one in ascending g from
 *                               0.0, divided by their number;
 *                             best = 1; for c = 2 .. k: if crit[c] > crit[best]:
 *                               best = c -- the first maximum, a NaN never wins;
 *                             ncomp = best, or 0 where crit[best] is NaN (no counted
 *                               row in the pooled block): the group is undefined,
 *                               its scores NaN and its counts zero;
 *                             PLSX_CVN_SELECT_MSE: k_sd_cvn_select's own rule.
 *                           The observed entry appends, per outer split, the OUTER
 *                           fit's block at c = ncomp to d_conf [capacity][G][G]
 *                           int32 and d_auc [capacity][G][2] int64 (or NULL: no AUC
 *                           counts), and pooled[1 .. k] to d_inner_conf
 *                           [capacity][k][G][G] int32 (or NULL); the permuted entry
 *                           appends one block per permutation, the sum over its
 *                           outer splits (k_sd_cvn_class_reduce, next to
 *                           k_sd_cvn_reduce; integers, so any batch cut gives the
 *                           same result; d_inner_conf is not written).  d_r, d_r2,
 *                           d_mse, d_ncomp(_count) and d_inner_mse of both entries
 *                           are those of THIS selection; an open series of
 *                           predictions with c = 0 takes its count.  A call that
 *                           would pass `capacity` (blocks) returns PLSX_ERR_ARG
 *                           before it computes anything.  _end, plsx_set_data,
 *                           plsx_simpls_set_classes and a second _begin end the
 *                           series.  _begin: PLSX_ERR_STATE without bound regression
 *                           data or before plsx_simpls_set_classes, PLSX_ERR_ARG for
 *                           a null d_conf, capacity < 1 or an unknown rule.
 */
#define PLSX_CVN_SELECT_MSE 0
#define PLSX_CVN_SELECT_ACCURACY 1
#define PLSX_CVN_SELECT_BALANCED 2
int plsx_simpls_decompose(plsx_ctx* ctx, double* d_xwT, double* d_pctvar, double* d_cvec,
                          double* d_yload, void* stream);
int plsx_simpls_set_original(plsx_ctx* ctx, const double* d_w0cT, void* stream);
int plsx_simpls_perm_batch(plsx_ctx* ctx, const int32_t* d_perm_idx, int n, double* d_out, void* stream);
int plsx_simpls_boot_batch(plsx_ctx* ctx, const int32_t* d_boot_idx, const double* d_ystack, int n,
                           double* d_usum, double* d_usq, double* d_yload, void* stream);
int plsx_simpls_set_row_masks(plsx_ctx* ctx, const uint8_t* d_okx, const uint8_t* d_oky, void* stream);
int plsx_simpls_crossval_batch(plsx_ctx* ctx, const uint8_t* d_masks, int m, double* d_r, double* d_r2,
                               double* d_sse, void* stream);
int plsx_simpls_crossval_perm_batch(plsx_ctx* ctx, const uint8_t* d_masks, int n, const int32_t* d_perm_idx, int m,
                                    double* d_r, double* d_r2, double* d_mse, void* stream);
int plsx_simpls_crossval_nested_batch(plsx_ctx* ctx, const uint8_t* d_codes, int n, int ni, double* d_r, double* d_r2,
                                      double* d_mse, int32_t* d_ncomp, double* d_inner_mse, void* stream);
int plsx_simpls_crossval_nested_perm_batch(plsx_ctx* ctx, const uint8_t* d_codes, int n, int ni,
                                           const int32_t* d_perm_idx, int m, double* d_r, double* d_r2, double* d_mse,
                                           int32_t* d_ncomp_count, void* stream);
int plsx_simpls_split_half_batch(plsx_ctx* ctx, const int32_t* d_perm_idx, int np, const uint8_t* d_masks, int ns,
                                 double* d_ucorr, double* d_vcorr, void* stream);
int plsx_simpls_set_confounds(plsx_ctx* ctx, const double* d_Z, int q, double* d_gx, double* d_gy, void* stream);
int plsx_simpls_crossval_confound_batch(plsx_ctx* ctx, const uint8_t* d_masks, int n, double* d_r, double* d_r2,
                                        double* d_sse, void* stream);
int plsx_simpls_crossval_confound_perm_batch(plsx_ctx* ctx, const uint8_t* d_masks, int n, const int32_t* d_perm_idx,
                                             int m, double* d_r, double* d_r2, double* d_mse, void* stream);
int plsx_simpls_coef_begin(plsx_ctx* ctx, int c, void* stream);
int plsx_simpls_coef_finish(plsx_ctx* ctx, double* d_bsum, double* d_bsq, void* stream);
int plsx_simpls_coef_keep(plsx_ctx* ctx, double* d_A, long long capacity);
int plsx_simpls_coef_ci(plsx_ctx* ctx, const double* d_A, long long n, int i_lo, double g_lo, int i_hi, double g_hi,
                        double* d_lo, double* d_hi, void* stream);
int plsx_simpls_coef_perm_test(plsx_ctx* ctx, const double* d_A, long long n, const double* d_obs, int standardise,
                               int32_t* d_count, double* d_max, void* stream);
int plsx_simpls_coef_perm_begin(plsx_ctx* ctx, int c, const double* d_obs, int standardise, int32_t* d_count,
                                double* d_max, long long capacity);
int plsx_simpls_coef_perm_end(plsx_ctx* ctx);
int plsx_simpls_set_classes(plsx_ctx* ctx, const int32_t* d_class, int G, void* stream);
int plsx_simpls_cv_class_begin(plsx_ctx* ctx, int32_t* d_conf, long long capacity);
int plsx_simpls_cv_class_end(plsx_ctx* ctx);
int plsx_simpls_cv_auc_begin(plsx_ctx* ctx, int64_t* d_auc, long long capacity);
int plsx_simpls_cv_auc_end(plsx_ctx* ctx);
int plsx_simpls_cv_pred_begin(plsx_ctx* ctx, int c, int32_t* d_ncomp, double* d_pred, double* d_true, long long capacity);
int plsx_simpls_cv_pred_end(plsx_ctx* ctx);
int plsx_simpls_cvn_class_begin(plsx_ctx* ctx, int rule, int32_t* d_conf, int64_t* d_auc, int32_t* d_inner_conf,
                                long long capacity);
int plsx_simpls_cvn_class_end(plsx_ctx* ctx);

/* The out-of-fold predictions of the behavioural cross-validation.  While a series is
 * open every plsx_crossval_batch, plsx_crossval_lv_batch and
 * plsx_crossval_confound_batch of m splits appends m slots [T][S] of doubles to d_pred
 * in submission order: slot[t][p] = z V_j^T + mean_train_j(Y) over the live latent
 * variables -- the `pred` of k_cv_final / k_cvp_final, which those kernels score -- on
 * the test rows of the split, NaN on its training rows; every entry of a slot is
 * written (kernel k_cv_pred_export, behind k_cv_final / k_cvp_final).  d_true
 * [capacity][T][S] or NULL: the observed rows at the same positions, on the confound
 * route the fold-residualised Y, which exists on the device only.  The permutation
 * entries append nothing; d_r, d_r2 and d_lv keep their bits with the series open.  A
 * call that would pass `capacity` (slots) returns PLSX_ERR_ARG before it computes or
 * writes anything.  _end, plsx_set_data and a second _begin end the series (the
 * buffers stay the caller's).  _begin: PLSX_ERR_STATE without bound behavioural data,
 * PLSX_ERR_ARG for a null stack or capacity < 1, PLSX_ERR_UNSUPPORTED (context still
 * usable, sizes in the message) for a stack -- 8 S T capacity bytes, twice that with
 * d_true -- beyond the scratch budget. */
int plsx_crossval_pred_begin(plsx_ctx* ctx, double* d_pred, double* d_true, long long capacity);
int plsx_crossval_pred_end(plsx_ctx* ctx);
int plsx_simpls_vip_keep(plsx_ctx* ctx, int c, double* d_G, long long capacity);
int plsx_simpls_vip_ci(plsx_ctx* ctx, const double* d_G, long long n, int c, int i_lo, double g_lo, int i_hi, double g_hi,
                       double* d_sd, double* d_lo, double* d_hi, void* stream);
int plsx_simpls_vip_perm_test(plsx_ctx* ctx, const double* d_G, long long n, int c, const double* d_obs,
                              int32_t* d_count, double* d_max, void* stream);
int plsx_simpls_vip_perm_begin(plsx_ctx* ctx, int c, const double* d_obs, int32_t* d_count, double* d_max,
                               long long capacity);
int plsx_simpls_vip_perm_end(plsx_ctx* ctx);

/* Bootstrap ratios -- compute.boot_rel (pyls/compute.py:212-237), elementwise
 * on (B, L) arrays: se = sqrt(|usq - usum^2/n| / (n-1)), bsr = orig / se.
 * add_orig != 0 first adds the original back (usum + orig, usq + orig^2) as
 * behavioral / regression PLS do (pyls/types/behavioral.py:201-203); `n` is
 * then n_boot + 1. */
int plsx_boot_rel(plsx_ctx* ctx, const double* d_orig, const double* d_usum,
                  const double* d_usq, int n, int add_orig, long long count,
                  double* d_bsr, double* d_se, void* stream);

/* Percentile interval of many series -- compute.boot_ci (pyls/compute.py:184-209,
 * numpy.percentile, default 'linear' interpolation).  d_data (nseries, n)
 * contiguous series; the two quantiles are given by their virtual index
 * (i, g) = (floor((n-1) q), fractional part) as numpy computes them.
 * d_lo, d_hi (nseries,) out.  n <= 16384.  Long series whose two ranks lie in the tails (a 95 % interval of 10 000
 * bootstraps) are settled by selection -- pivots from a sorted sample, one counting pass, a sort of the <= 2048
 * values beyond the pivots -- with the full LDS sort as the fallback; both are exact order statistics. */
int plsx_percentile_ci(plsx_ctx* ctx, const double* d_data, long long nseries, int n, int i_lo, double g_lo,
                       int i_hi, double g_hi, double* d_lo, double* d_hi, void* stream);

/* On-box fp64 MFMA issue-rate microbenchmark (v_mfma_f64_16x16x4_f64, 8
 * independent accumulators per wave): measured TFLOP/s -> *tflops. */
int plsx_mfma_f64_peak(plsx_ctx* ctx, double* tflops);

/* Performance counters of the last perm/boot call: fills up to `cap` doubles:
 * [0] kernel ms of the cross-product kernel (HIP events on the launch stream),
 * [1] its launch count, [2] resamples per launch group, [3] M tiles per block,
 * [4] super-batch size, [5] resamples those launches covered, [6] 1 if
 * permutations take the dual (S x S kernel) path and launch no cross-product
 * kernel, [7] compact blocks (one bootstrap per block contracting over the
 * rows it draws): contracted rows / S of the last launch, 0 when the last
 * launch used the dense layouts, [8] flop of the timed dual-space products
 * (k_nt_gemm), [9] bootstrap series closed on the quadratic-form route
 * (plsx_boot_finish) since timing was switched on, [10] / [11] tile rows of a
 * block / blocks per latent variable of the last closing pass.
 * [12..18] say how the last rotation pass (k_urot) and the last Gram pass were
 * launched; they are recorded whether or not timing is on (0 before the first
 * such launch): [12] waves per block of the rotation kernel (4 or 8), [13] its
 * resample splits (grid y; more than 1: partial sums added by k_add_splits),
 * [14] resamples per split, [15] its variant: the compiled-in k-step count
 * 1..16, plus 100 when the last tile of L ran on the 4x4x4 shape (TAIL); 0 the
 * generic variant with the whole operand in LDS, -1 the generic variant staged
 * in pieces -- of the launch of the first chunk of L tiles, [16] column chunks
 * of the last k_gram4 / k_gram / k_gram_lds launch, [17] as [15] for the last
 * chunk of L tiles (equal to [15] unless L is cut into several launches),
 * [18] the Gram kernel: row blocks NB of k_gram4 (1..13), 0 k_gram (16x16x4),
 * -1 k_gram_lds.
 * [19] / [20] say how the last pass of plsx_split_half_batch ran: [19] its
 * cross-product blocks -- 0 both halves as resamples of the plain blocks (no
 * fused epilogue), 1 the dense fused blocks (several splits per block), 5 / 8
 * compact blocks, one split each, with the fused epilogue 5 / the raw first-half
 * sums of epilogue 8; [20] the one-pass reader behind epilogue 8 -- 0 none, else
 * its waves per block (12 or 8), plus 100 with the wave kinds in runs of four.
 * [21] 1 when the compact bootstrap blocks of the last launch formed the first
 * moments of the features in their own padding rows (the moment-only blocks then
 * contract X^2 alone), 0 on every other route.
 * [22] 1 when the last permutation call took the projected route (rotated
 * permutations of a fixed-X binding with L == T' and every original LV live:
 * singular values from the row norms of (V0^T A_p) X, no cross-product scratch,
 * no Gram pass, no small solver; option "no_perm_project"), else 0.
 * [23] column tiles per wave of the compact bootstrap blocks of the last
 * launch: 4 (blocks of 256 feature columns) or 2 (128), 0 when the last
 * launch had no such blocks; options "no_compact_wide", "compact_wide_always".
 * Returns the number written. */
int plsx_last_timing(const plsx_ctx* ctx, double* out, int cap);
/* Scratch budget of the resampling super-batches (default 48 GB; the R block
 * of one bootstrap is 8 T' B bytes).  fixed = 1: every launch uses budget-sized
 * super-batches -- the steady-state setting for a long-lived context (what
 * bench.py measures).  fixed = 0 (default): the super-batch of a call is sized
 * by a cost model that weighs mapping fresh device memory (the driver clears
 * recycled VRAM, 30-70 ms per GB) against the per-launch overhead, so a
 * one-shot run of a few thousand resamples maps a few GB instead of 48.
 * Must precede plsx_set_data.  No reference counterpart
 * (joblib workers size themselves, pyls/base.py:490-507). */
int plsx_set_scratch(plsx_ctx* ctx, double max_gb, int fixed);

/* Enable (1) / disable (0) event timing of the kernel launches (HIP events on
 * the launch stream); enabling clears the records. */
int plsx_set_timing(plsx_ctx* ctx, int enable);

/* Summed duration (ms) and launch count of one kernel class since timing was
 * enabled: 0 k_xprod (cross-product), 1 k_gram / k_gram4 (+ partial reduce),
 * 2 k_small / k_small_ql (eigen-solve + Procrustes), 3 k_urot (+ split add), 4 k_nt_gemm
 * (+ reduce), 5 k_ucorr_partial, 6 k_simpls_dual, 7 reserved, ..., 9 k_sd_cv_score (with the pair expansion and the
 * reduction over the splits of plsx_simpls_crossval_perm_batch, and k_row_sum / k_sd_sh_prep / k_sd_sh_expand /
 * k_sd_sh_score of plsx_simpls_split_half_batch, and k_sd_cv_pred / k_cv_pred_export of an open plsx_simpls_cv_pred_begin / plsx_crossval_pred_begin series), ..., 11 k_coef_prod (the feature pass of
 * plsx_simpls_coef_ci; k_vip_prod and k_vip_moments of plsx_simpls_vip_ci and k_coef_perm_prod / k_coef_perm_max /
 * k_col_sd of plsx_simpls_coef_perm_test and k_vip_perm_prod / k_vip_perm_count / k_coef_perm_max of plsx_simpls_vip_perm_test count
 * here too, and so do k_coef_perm_prod / k_coef_perm_max / k_col_rsd of plsx_perm_weights_test, whose builders
 * k_perm_W_behav / k_perm_VA / k_perm_W_mc count under 7; k_sd_vip under 10 with
 * k_sd_coef), 12 k_percentile (selection / sort of plsx_percentile_ci, plsx_simpls_coef_ci and plsx_simpls_vip_ci),
 * 13 k_contrast (non-rotated PLS: k_contrast_norms + its chunk sum, k_contrast_quad, k_contrast_fill),
 * 14 k_mb_rownorm (multiblock PLS: the row norms of a batch's R slots and their scaling, k_mb_rownorm + k_mb_rowscale),
 * 15 k_sd_cv_class (the confusion counts of an open plsx_simpls_cv_class_begin series),
 * 16 k_sd_cv_auc (the AUC counts of an open plsx_simpls_cv_auc_begin series),
 * 17 k_weights_prod (the feature pass of plsx_boot_weights_ci: one launch per chunk of features; its scale table
 * counts under 8, its operand builders under 7, its selection under 12),
 * 18 k_cvp_moments (the per-split training mean / scale tables of plsx_crossval_perm_batch),
 * 19 k_cvp_gram (its scaled Gram product with the sum of the partial tiles; its operand builder counts under 7, its
 * small solver under 2, its scores under 9), 20 k_cvp_w and 21 k_cvp_g (its products W' = A M^T and G = W' A^T:
 * k_nt_gemm launches, which class 4 counts as well), 22 k_cvp_mean (its mean over the splits),
 * 23 k_cv_final (the predictions and scores of plsx_crossval_batch / plsx_crossval_lv_batch), 24 k_cv_lv and
 * 25 k_cvp_lv (the score correlations of the latent variables of plsx_crossval_lv_batch / plsx_crossval_perm_lv_batch).
 * 26 k_cf_resid (plsx_simpls_set_confounds: k_cf_ztilde and k_cf_chol in one bracket, the two k_cf_resid launches in
 * another; K formed again counts under 4), and of its fold entries 27 k_cf_fold_prep (k_cf_fold_prep and k_cf_fold_F,
 * one bracket each per group of splits; C_s = P_s K_r counts under 4), 28 k_cf_fold_K (one launch per group) and
 * 29 k_cf_fold_Y (the fits' own Y of a solver batch, and the expansion of their masks under permutations); their fits
 * count under 6 and 9, the reduction over the splits under 9.
 * 30 k_cfb_fold_X (the fold copies X_s of plsx_crossval_confound_batch / _perm_batch: one bracket per group of splits;
 * their P_s count under 27, their Y under 29, plsx_residualize / plsx_set_confounds under 26).
 * plsx_kernel_class_name returns the label, NULL past the last class.
 * Measurement only; no reference counterpart. */
int plsx_kernel_timing(const plsx_ctx* ctx, int kernel_class, double* ms, int* launches);
const char* plsx_kernel_class_name(int kernel_class);

/* Route of plsx_perm_batch: dual = 1 (default where available) forms the S x S
 * kernel of the fixed feature matrix once per call and never touches the
 * features again; dual = 0 takes the feature pass R_p = A_p X per permutation,
 * the same pipeline the bootstrap uses (the north-star pipeline; what
 * bench.py reports as value_primal).  Both give the same statistics to
 * rounding.  The S x S kernel is a function of the bound data only: the first
 * dual call after plsx_set_data or after this call forms it, later calls
 * (chunks of one analysis) reuse it; dual < 0 keeps the route and only drops
 * that kernel (bench.py: every timed analysis forms its own).  Returns the
 * route now in effect (0 / 1; 0 whatever was asked when the original spectrum is graded, see
 * plsx_numeric_report) or a negative status.  At bind time: plsx_set_option(ctx, "no_dual_perm", 1). */
int plsx_set_perm_path(plsx_ctx* ctx, int dual);

/*
 * Route / layout switch `key` := value (0 / 1 unless stated).  Every route computes the same statistics to
 * rounding; the switches exist for A/B measurements and so that tests can pin each kernel variant against the
 * others and the oracle.  The library reads NO environment variable: a host that wants PLSX_<KEY>=1 to mean
 * something passes it on itself (bench.py and the tests do, pypyls_amd.engine.options_from_env).
 *   layout-time (before plsx_set_data): "min_batch" (resamples per super-batch aimed for, default 4096),
 *     "inblock_moments", "no_fixed_x", "no_dual_perm"
 *   any time: "no_refine" (graded spectra: skip the refinement on R), "two_pass_boot", "no_compact_boot",
 *     "compact_boot_always", "crosscov_sparse" (plsx_crosscov_batch treats its resamples as bootstraps: the compact
 *     blocks wherever plsx_boot_batch would take them, so that tests can read R of a compact launch),
 *     "sepmom_always", "no_moment_rows" (compact bootstrap blocks: first moments from the moment-only blocks even
 *     where the padding rows of a block could deliver them), "no_compact_wide" (compact bootstrap blocks: two
 *     column tiles per wave, blocks of 128 columns, also where blocks of 256 are the default),
 *     "compact_wide_always" (tests: four column tiles per wave wherever they are compiled, T' <= 64),
 *     "no_perm_project" (rotated permutations on the fixed-X
 *     route: always R, its Gram matrix and the small solver, also where the row norms of the projected product
 *     would do), "no_split_fuse" (split halves: two passes), "split_two_readers"
 *     (fused split blocks read by the Gram and the projection kernel instead of the one-pass reader),
 *     "split_reader8" (bit 0: the one-pass reader as the round-5 8-wave block whose matrix waves build the tiles
 *     themselves, instead of the 12-wave block with dedicated construction waves; bit 1: wave kinds in runs of
 *     four waves instead of interleaved wave by wave),
 *     "split_inblock", "no_gram4", "urot_generic", "urot_no_tail4", "simpls_jacobi" (SIMPLS: full Jacobi instead
 *     of the leading-eigenpair solver), "simpls_global" (SIMPLS: the component-step kernels with their S-long
 *     buffers in device memory, the route S beyond the on-chip bound takes anyway), "quad_sums" (plsx_boot_begin: 1 = the quadratic-form route whenever it
 *     applies, -1 = never), "percentile_sort" (plsx_percentile_ci: always the full sort instead of the tail
 *     selection);
 *     "expect_resamples" = n: the caller is about to ship n resamples in several calls (chunks of one analysis):
 *     size the super-batch scratch for n once instead of per call (0 = per call)
 * plsx_option_name(i) enumerates the keys (NULL past the last).  No reference counterpart.
 */
int plsx_set_option(plsx_ctx* ctx, const char* key, int value);
const char* plsx_option_name(int index);

/*
 * Graded spectra.  The device takes singular values / vectors from the Gram side (G = R R^T), which loses
 * eps (d_max / d_k)^2 where the reference's SVD of R (pyls/compute.py:10-52) loses eps d_max / d_k.  A resample
 * with a live LV below 1e-3 d_max therefore re-solves the subspace of its small LVs on R itself (its Gram matrix
 * in the rotated basis V_s^T R, whose rounding errors are relative to the SMALL scale) wherever R exists: every
 * feature-pass route, at every T' (one-sided Jacobi solver up to T' = 64, Householder + QL above).  A data set
 * whose ORIGINAL spectrum is graded (plsx_decompose / plsx_set_original) is taken off the dual-space routes for
 * that reason.  This call synchronises the device and returns -- and clears -- two counters since the last call:
 * resamples whose small LVs were refined, and resamples with a live LV below 1e-5 d_max that could NOT be -- only a
 * dual-space route on data whose original spectrum was not graded leaves any: their LVs below ~ 6e-6 d_max may
 * miss the 1e-5 relative tolerance; the host warns.
 */
int plsx_numeric_report(plsx_ctx* ctx, long long* refined, long long* unrefined);

/*
 * Host-side index generators -- gen_permsamp / gen_bootsamp / gen_splits
 * (pyls/base.py:10-79, 82-159, 162-229), draw-for-draw compatible with the
 * reference's numpy.random.RandomState so a seed gives the same arrays.  No
 * device and no context involved.  The generator state travels as numpy's
 * `RandomState.get_state()` pair: mt_key (624 words, in/out) and *mt_pos
 * (in/out).  groups (n_groups,) subjects per group; output one resample per
 * ROW: (n, S) int32 indices / (n_split, S) uint8 masks (1 = first half /
 * training row).  Return 0, 1 when the 500-try duplicate limit was hit (the
 * reference warns, base.py:70-74), or a negative status.
 * plsx_gen_splits_seeded draws the masks of n_seeds independent
 * RandomState(seeds[i]) streams (what permutation i uses, base.py:705-708):
 * out (n_seeds, n_split, S).
 */
int plsx_gen_permsamp(const int* groups, int n_groups, int n_cond, int n_perm, uint32_t* mt_key, int* mt_pos,
                      int32_t* out);
int plsx_gen_bootsamp(const int* groups, int n_groups, int n_cond, int n_boot, uint32_t* mt_key, int* mt_pos,
                      int32_t* out);
/* Streaming variants: identical draws and output; *rows_done (may be NULL) is
 * stored with release order after every finished row, so that another host
 * thread can ship rows [0, *rows_done) to the device while later rows are
 * still being drawn -- the duplicate test only ever looks backwards
 * (base.py:67-69, 145-149), finished rows never change. */
int plsx_gen_permsamp_stream(const int* groups, int n_groups, int n_cond, int n_perm, uint32_t* mt_key, int* mt_pos,
                             int32_t* out, int* rows_done);
int plsx_gen_bootsamp_stream(const int* groups, int n_groups, int n_cond, int n_boot, uint32_t* mt_key, int* mt_pos,
                             int32_t* out, int* rows_done);
int plsx_gen_splits(const int* groups, int n_groups, int n_cond, int n_split, double test_size,
                    uint32_t* mt_key, int* mt_pos, uint8_t* out);
int plsx_gen_splits_seeded(const int* groups, int n_groups, int n_cond, int n_split, double test_size,
                           const uint32_t* seeds, int n_seeds, uint8_t* out);

/*
 * The collective of the sharded resampling loops: what the
 * reference does with joblib's gather of the per-resample results
 * (pyls/base.py:490-507, 644-650; pyls/utils.py:252-279) is, with one process
 * per GPU, ONE all-gather of a packed per-rank buffer
 *     [ perm_singval slice | distrib slice | partial sum U | partial sum U^2 ].
 * The communicator is RCCL (xGMI inside a node), reached through dlopen: the
 * library does not link a communication runtime.  plsx_comm_load names the
 * librccl.so to use -- a host that already carries one (PyTorch-ROCm bundles
 * its own) passes that path so the process keeps a single copy; with NULL
 * the copy already loaded in the process is taken, else "librccl.so.1" /
 * "librccl.so" from the loader path, else /opt/rocm/lib/librccl.so.
 *   plsx_comm_unique_id  rank 0 only: 128 bytes to hand to every rank through
 *                        the launcher's own rendezvous (store, file, MPI ...)
 *   plsx_comm_init       collective over the `world` ranks: one rank per GPU,
 *                        binds the communicator to the context's device
 *   plsx_allgather       d_recv[r * bytes_per_rank ...] = rank r's d_send, on
 *                        `stream`, asynchronous like every other entry;
 *                        d_send may alias its own slot of d_recv (in place)
 *   plsx_comm_destroy    also called by plsx_ctx_destroy
 * Without plsx_comm_init a context is a world of one and plsx_allgather is a
 * device-to-device copy.
 *
 * ONE process driving several devices (SURVEY 8(b) "plsx_allgather(ctx[], nranks,
 * ...)", 8(e) "single process driving 8 devices (ncclCommInitAll) is sufficient;
 * no torch.distributed") -- what `n_proc` workers are in the reference
 * (pyls/utils.py:252-279, pyls/base.py:286-292): the host keeps one context per
 * device and one host thread per context, and a single thread issues the
 * collective for all of them:
 *   plsx_comm_init_all   contexts 0 .. n-1 become ranks 0 .. n-1 of one team.
 *                        transport PLSX_TRANSPORT_RCCL: ncclCommInitAll over the
 *                        contexts' devices (they must be distinct);
 *                        PLSX_TRANSPORT_PEER: no communicator, the gather is n
 *                        hipMemcpyPeerAsync pulls per rank (xGMI between devices;
 *                        the only form that accepts the SAME device twice -- two
 *                        contexts sharing one GPU, the single-GPU test of the team
 *                        path); PLSX_TRANSPORT_AUTO: RCCL when the devices are
 *                        distinct, peer copies otherwise.
 *   plsx_allgather_all   d_recv[r][q * bytes ...] = d_send[q] for every rank r,
 *                        enqueued on streams[r] (NULL = the null streams): one
 *                        ncclGroupStart / n x ncclAllGather / ncclGroupEnd, or the
 *                        peer copies ordered behind an event on every sender's
 *                        stream.  Asynchronous; a send buffer may be reused once
 *                        EVERY rank's stream has passed the call.
 *   plsx_comm_destroy    per context, as above.
 *   plsx_comm_transport  0: the context is a world of one, else the
 *                        PLSX_TRANSPORT_* value its communicator runs on.
 */
enum { PLSX_TRANSPORT_AUTO = 0, PLSX_TRANSPORT_RCCL = 1, PLSX_TRANSPORT_PEER = 2 };
int plsx_comm_load(plsx_ctx* ctx, const char* librccl_path);
int plsx_comm_unique_id(plsx_ctx* ctx, void* id128);
int plsx_comm_init(plsx_ctx* ctx, const void* id128, int rank, int world);
int plsx_comm_rank(const plsx_ctx* ctx, int* rank, int* world);
int plsx_allgather(plsx_ctx* ctx, const void* d_send, void* d_recv, long long bytes_per_rank, void* stream);
int plsx_comm_destroy(plsx_ctx* ctx);
int plsx_comm_init_all(plsx_ctx** ctxs, int n, int transport);
int plsx_comm_transport(const plsx_ctx* ctx);
int plsx_allgather_all(plsx_ctx** ctxs, int n, const void* const* d_send, void* const* d_recv,
                       long long bytes_per_rank, void* const* streams);

#ifdef __cplusplus
}
#endif
#endif /* PLSX_H_ */
