// plsx_k_xprod.h -- the cross-product kernels k_xprod (dense blocks, every epilogue) and k_xprod_compact (one resample per block).
// Included through plsx_kernels.h (which documents the operand layouts and lists the kernel headers in order).  gfx950 only.
#pragma once
#include <type_traits>
#include <utility>

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), unrolled at compile time
template <class F, int... I>
__device__ __forceinline__ void xprod_static_for(F&& f, std::integer_sequence<int, I...>)
{
    (f(std::integral_constant<int, I>()), ...);
}
#include "plsx_common.h"
#include "plsx_k_prep.h"

// ---------------------------------------------------------------------------
// K_R: resampled cross-product  R[r] = scale o (A_r . X)
// ---------------------------------------------------------------------------
//
// One block = 128 feature columns x one group of n resamples (all of its
// n*T' (+ moment) rows): 8 waves, wave w owns the 16-column tile w and every
// M tile, so X is streamed from HBM exactly once per group straight into MFMA
// B fragments (no LDS, no reuse to exploit) while the small A operand (shared
// by all 8 waves and by every block of the group) is staged through LDS in
// fragment order -> conflict-free ds_read_b64, one read per MFMA.
// Block id -> (column block, group) with the group as the fast index: block b
// runs on XCD b % 8, so with 8 groups every XCD's L2 keeps one group's A.
//
// Rows of a group: [0, w0*16) data rows (n*T' packed), then first-moment rows
// (weights, B operand x), then second-moment rows (same weights, B operand
// x*x).  The epilogue turns the two moments into 1/std of the resampled
// feature inside the cell (ddof = 1, pyls/compute.py:84) and scales R.
// NW waves per block (block = NW*16 feature columns), KT k-steps per LDS stage.
// Copy one fragment-ordered A stage (STAGE doubles) global -> LDS with the
// LDS-DMA path: each wave instruction moves 64 lanes x 16 B into
// wave-uniform-base + lane*16, i.e. a straight lane-linear memcpy.
// The copy goes through a buffer resource: the per-lane offset (tid * 16) never
// changes and the per-pass offset is an SGPR, so the copy costs no VALU
// instruction at all (VALU issue between fp64 MFMAs costs matrix-pipe slots;
// flat addressing needs 64-bit VALU adds per load).
#define PLSX_RSRC_FLAGS 0x00020000
template <int NT, int PASSES, bool EVEN, int STAGE>
__device__ __forceinline__ void stage_copy_buf(const double* src, double* dst, int tid, int wave)
{
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)src, (short)0, 0x7fffffff,
                                                                   PLSX_RSRC_FLAGS);
    const int voff = tid * 16;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        if (EVEN || p * NT + wave * 64 < STAGE / 2) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rs, (__attribute__((address_space(3))) void*)(dst + (size_t)(p * NT + wave * 64) * 2),
                16, voff, p * NT * 16, 0, 0);
        }
    }
}

__device__ __forceinline__ double load_x_buf(const double* rowbase, int voff)
{
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)rowbase, (short)0, 0x7fffffff,
                                                                   PLSX_RSRC_FLAGS);
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, 0, 0));
}

// NSQ = number of second-moment tiles; they are the LAST NSQ tiles of the block
// (static split: no per-tile operand select in the MFMA loop -- VALU work between
// fp64 MFMAs costs matrix-pipe issue slots on gfx950, measured 8 %).
// EPI selects the epilogue: 0 = store R (scaled by 1/std when the group carries moment rows),
// 1 = fused split-half (both halves from the first half's raw sums, SplitEpi),
// 2 = accumulate: the group's data rows are rows l = 0..L-1 of ITS resamples (out_row[row] = l),
//     nothing is stored per resample; the block adds its resamples' values and squares per
//     (l, column) in LDS and writes one partial (sum, sum of squares) tile per group -- the
//     single-pass bootstrap of the unscaled modes, where the A operand already holds
//     W_r^T = (A_r^T M_r)^T and the product IS the rotated bootstrap weights U_r = X^T W_r.
// 3 = data-only block of the separate-moments layout: R scaled by 1 / std from a table (se.scale),
// 4 = moment-only block (MT = 2 NSQ: weight tiles against X, then against X^2) writing that table.
//     Correlation mode with in-block moments spends 2 of 24 tiles on 7 + 7 moment rows; here the
//     moments of 192 (resample, cell) pairs fill a block and the data blocks carry data only.
#define PLSX_ACC_PITCH 80        // LDS pitch of an l-row (64 columns + 16: rows l, l+1 of one MFMA register land in different banks)
// 6 = moment-only block writing the raw moments m1, m2 (se.scale, se.scale2) -- the first-half feature moments
//     of the compact fused split-half blocks (k_xprod_compact, EPI 5 there).
// 9 = second-moment-only block (NSQ == MT: every tile against X^2) writing the RAW m2 of its 16 MT pairs into the
//     table that holds 1 / std on the other routes (se.scale): the compact bootstrap blocks whose padding rows deliver
//     m1 (k_xprod_compact, EPI 3 with se.nmu > 0) form 1 / std from the two themselves.
// 10 = row norms: nothing of R is stored; the block writes sum_col (A . X)^2 of its 64 columns per row (se.acc_sum:
//     [column block][group][se.accB rows]) -- rotated permutations with a square orthogonal V0 on the fixed-X route,
//     whose A operand is V0^T A_p (k_build_A_proj): the statistic is the norm of each row of V0^T R_p.
//     The tiles are held TRANSPOSED.  For v_mfma_f64_16x16x4 the two operand layouts coincide (A wants A[i][k] at lane
//     16 k + i, B wants B[k][n] at lane 16 k + n), so the same two registers in the other order -- mfma(x, a, acc) for
//     mfma(a, x, acc) -- give D^T: lane & 15 = row inside the tile, (lane >> 4, register r) = column 4 r + (lane >> 4)
//     of the wave's 16.  Every accumulator element receives the same products in the same k order (the same bits), the
//     loop issues the same instructions, and a lane's four registers of a tile are four columns of ONE row: the sum
//     of squares over the columns starts lane-local (4 fp64 operations a tile) and ends with 16 partials per row in LDS.
//     With the rows on lane >> 4 and the registers (every other epilogue) each of a lane's 100 values is another row
//     and has to be added over 16 lanes: 400 additions and 800 DPP moves a lane, 4.2 ms per launch of 504 at the
//     headline shape (74.17 against 69.92 for the same loop, operands NOT exchanged, with this epilogue -- a timing
//     build, its values are wrong).  The exchange itself is not free as the instruction count suggests: the loop with
//     x as the A operand measures 1 - 3 ms per launch slower, by how many LDS reads run ahead (see the main loop).
//     profiles/perm_rownorm_lanes_compare.txt has the figures.
template <int MT, int NW, int KT, int NSQ, int EPI = 0>
__global__ __launch_bounds__(NW * 64, 2)
void k_xprod(const double* __restrict__ Afrag, size_t group_stride,
             const double* __restrict__ X, int ldx, int nks,
             double* __restrict__ R, int ldr, int rows_per_group,
             const int* __restrict__ out_row, const int* __restrict__ mom_idx,
             const double* __restrict__ mom_n, int nmom_pad,
             int n_groups, int ncolblk, double* __restrict__ mom_out, SplitEpi se, int ntab)
{
    // ntab > 1 (sliced layout): group g holds slice g % ntab of resample g / ntab; every
    // slice has its own row tables, all slices of a resample write into its R block.
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int NT = NW * 64;                      // threads
    constexpr int STAGE = KT * MT * 64;              // doubles per stage (global pitch)
    constexpr int STAGE_LDS = ((STAGE + 127) / 128) * 128;   // LDS pitch: whole wave-DMA pieces
    constexpr int PASSES = (STAGE + NT * 2 - 1) / (NT * 2);   // NT threads x double2
    constexpr bool EVEN = (STAGE % (NT * 2)) == 0;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    // block id -> (group, column block): consecutive ids walk 8 groups (one per
    // XCD: block b runs on XCD b % 8, so each XCD's L2 keeps ONE group's A
    // operand at a time) and then the column blocks; groups beyond the first 8
    // follow in further sweeps over the columns.
    // A last, partial sweep (n_groups % 8 = rem groups) would leave 8 - rem XCDs
    // idle: its rem * ncolblk tiles are dealt out as eight contiguous ranges
    // instead, one per XCD (each XCD then touches at most two groups' A).
    const int sweep = blockIdx.x / (8 * ncolblk);
    const int within = blockIdx.x - sweep * (8 * ncolblk);
    int grp = sweep * 8 + (within & 7);
    int colblk = within >> 3;
    if (sweep * 8 + 8 > n_groups) {
        const int rem = n_groups - sweep * 8;
        const int cnt = (rem * ncolblk + 7) >> 3;
        const int id = (within & 7) * cnt + colblk;
        if (colblk >= cnt || id >= rem * ncolblk) return;
        grp = sweep * 8 + id / ncolblk;
        colblk = id - (id / ncolblk) * ncolblk;
    }
    const int col = colblk * (NW * 16) + wave * 16 + (lane & 15);
    const int kq = lane >> 4;

    // EPI 7 (rows s0.. of a SYMMETRIC matrix, quadratic form): the contraction starts at the block's own first row --
    // the packer doubled the entries right of the diagonal (inside the diagonal block too) and dropped those left of it
    static_assert(EPI != 7 || KT == 1 || KT == 2 || KT == 4, "EPI 7: the four k-steps of a tile row are whole stages");
    // groups are numbered row block first (grp = block * se.J + lv, se.J = LVs of the pass): the eight groups of a
    // sweep -- one per XCD, dispatched in lockstep -- then have the same contraction length
    const int qblk = (EPI == 7) ? grp / max(se.J, 1) : 0;
    const int ks0 = (EPI == 7) ? qblk * (MT * 4) : 0;
    if (EPI == 7) { X += (size_t)ks0 * 4 * ldx; nks -= ks0; }
    const double* Ag = Afrag + (size_t)grp * group_stride + (size_t)ks0 * (MT * 64);
    const int swave = __builtin_amdgcn_readfirstlane(wave);
    const int xvoff = (kq * ldx + min(col, ldx - 1)) * 8;   // per-lane byte offset inside a 4-row k-step (a block of
                                                            // 8 waves may hang over the last 64 columns)

    d4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = (d4){0.0, 0.0, 0.0, 0.0};

    const int nkt = nks / KT;
    constexpr bool SPLIT = (EPI == 1);
    if constexpr (SPLIT) {
        // Fused split-half: the epilogue needs this block's (Tpp x 64) tile of the
        // arrangement's full-sample R and the group's row constants.  Fetched here by
        // LDS-DMA (they land during the main loop), the epilogue then has NO global
        // load between its stores: on gfx950 loads and stores share vmcnt, so a load
        // waited for in the store loop drains every store before it (measured: the
        // interleaved form cost 20 % of the kernel).
        if (se.off_pre > 0 && NW == 4) {
            double* sRf = smem + se.off_pre;
            double* sRc = sRf + se.Tpp * (NW * 16);
            __amdgpu_buffer_rsrc_t rsF = __builtin_amdgcn_make_buffer_rsrc(
                (void*)(se.Rfull + (size_t)colblk * (NW * 16)), (short)0, 0x7fffffff, PLSX_RSRC_FLAGS);
            const int vo = ((lane >> 5) * ldr + (lane & 31) * 2) * 8;
            for (int j = swave; j < se.Tpp / 2; j += NW)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rsF, (__attribute__((address_space(3))) void*)(sRf + j * 128), 16, vo, j * 2 * ldr * 8, 0, 0);
            __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc(
                (void*)(se.rowc + (size_t)grp * MT * 16 * 5), (short)0, 0x7fffffff, PLSX_RSRC_FLAGS);
            for (int pc = swave; pc < (MT * 16 * 5 + 127) / 128; pc += NW)     // (whole 1 KB pieces: rowc carries slack)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rsC, (__attribute__((address_space(3))) void*)(sRc + pc * 128), 16, lane * 16, pc * 1024, 0, 0);
        }
    }
    // prologue: stage 0 of A, first X fragments
    stage_copy_buf<NT, PASSES, EVEN, STAGE>(Ag, smem, tid, swave);
    double xb[KT];
#pragma unroll
    for (int s = 0; s < KT; ++s)
        xb[s] = load_x_buf(X + (size_t)(s * 4) * ldx, xvoff);
    // Force the first X fragments to be resident before the loop: a load still
    // pending at the loop header makes hipcc place a near-draining
    // s_waitcnt vmcnt(1) right after the next stage's loads are issued.
#pragma unroll
    for (int s = 0; s < KT; ++s) asm volatile("" : "+v"(xb[s]));
    __syncthreads();

    // one pass of the main loop with the first NA tiles live (NA = MT: all of them).  EPI 7: inside the diagonal block
    // the packer kept the upper triangle (k_pack_afrag) -- the fragment of tile m is zero for every k-step left of the
    // tile's first row (kt < 4 m) and is not issued: the first 4 MT passes run unrolled in chunks of four with
    // m + 1 live tiles, a compile-time count each, so that neither they nor the steady-state loop carry a test (with
    // one test inside the single main loop the whole loop lost its schedule: 26.8 -> 40 ms at c5).
    auto pass = [&](int kt, auto na) {
        constexpr int NA = decltype(na)::value;
        const int cur = kt & 1;
        // next stage (clamped on the last pass: a harmless re-load keeps the
        // loop body branch-free so the waits sit right before the LDS write)
        const int kn = min(kt + 1, nkt - 1);
        double xn[KT];
        // A stage kn: global -> LDS DMA (buffer_load ... lds: no staging VGPRs,
        // no ds_write pass), into the buffer every wave finished reading before
        // the barrier that ended the previous pass.
        stage_copy_buf<NT, PASSES, EVEN, STAGE>(Ag + (size_t)kn * STAGE, smem + (cur ^ 1) * STAGE_LDS, tid, swave);
#pragma unroll
        for (int s = 0; s < KT; ++s)
            xn[s] = load_x_buf(X + (size_t)((kn * KT + s) * 4) * ldx, xvoff);
        const double* sA = smem + cur * STAGE_LDS + lane;
#pragma unroll
        for (int s = 0; s < KT; ++s) {
            const double b = xb[s];
            const double bsq = (NSQ > 0) ? b * b : 0.0;
#pragma unroll
            for (int m = 0; m < NA; ++m) {
                // EPI 10: the same two registers in the other order -- the transposed tile (see the epilogue list above)
                if constexpr (EPI == 10) acc[m] = mfma_f64(b, sA[(s * MT + m) * 64], acc[m]);
                else acc[m] = mfma_f64(sA[(s * MT + m) * 64], (m < MT - NSQ) ? b : bsq, acc[m]);
            }
        }
        if constexpr (EPI == 10) {
            // With the operands exchanged hipcc keeps only three LDS reads of A (two fragments each) ahead of the MFMAs
            // -- the other instantiations get five -- and the loop ran slower for it.  The order is pinned instead:
            // seven reads up front, then one read per two MFMAs.  Per launch of 504 at the headline shape: 73.4 ms as
            // hipcc orders it, 72.1 with five reads ahead, 71.3 with seven (248 registers), 72.9 with eight, 71.2
            // with nine (256 registers: nothing left); profiles/perm_rownorm_lanes_compare.txt.
            __builtin_amdgcn_sched_group_barrier(0x100, 7, 0);
#pragma unroll
            for (int i = 0; i < (KT * MT) / 2; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
        }
#pragma unroll
        for (int s = 0; s < KT; ++s) xb[s] = xn[s];
        __syncthreads();             // (drains the DMA issued one pass ago, then barrier)
    };
    int kt_first = 0;
    if constexpr (EPI == 7) {
        xprod_static_for([&](auto mm) {
#pragma unroll
            for (int j = 0; j < 4 / KT; ++j) {
                const int kt = (4 / KT) * decltype(mm)::value + j;
                if (kt < nkt) pass(kt, std::integral_constant<int, decltype(mm)::value + 1>());
            }
        }, std::make_integer_sequence<int, MT>());
        kt_first = min(nkt, 4 * MT / KT);
    }
    for (int kt = kt_first; kt < nkt; ++kt) pass(kt, std::integral_constant<int, MT>());

    // ---- epilogue -----------------------------------------------------------
    // Tile roles are static: data tiles [0, W0), first-moment (weight) tiles
    // [W0, SQ0), second-moment tiles [SQ0, MT).  Lane (kq, c) reg i of weight
    // tile W0+j holds m1 of moment row j*16 + kq + 4*i and the same lane / reg
    // of tile SQ0+j holds m2 of that row.  The A stages are dead: reuse LDS.
    constexpr int W0 = (EPI == 9) ? 0 : MT - 2 * NSQ, SQ0 = MT - NSQ, NMOM = NSQ * 16;
    if constexpr (EPI == 10) {
        // row norms (projected permutations): the block's share of sum_col acc^2 per row, in a FIXED order.  The tiles are
        // transposed (operands exchanged in the main loop): lane (kq, i) holds row m * 16 + i of tile m at the wave's
        // columns kq, 4 + kq, 8 + kq, 12 + kq in registers 0 .. 3, so its share of the row's norm is lane-local:
        //   q = ((a0^2 + a1^2) + a2^2) + a3^2     (fma chain, register order)
        // -- no cross-lane move.  A row then has 16 partials, one per (wave, kq), i.e. per column class
        // c % 4 = kq of the wave's 16 columns: they meet in LDS (the A stages are dead), partial p = wave * 4 + kq in
        // sP[p][MT * 16], and one thread per row adds them as ((p0 + p1) + (p2 + p3)) per wave, then
        // ((w0 + w1) + (w2 + w3)) over the waves.  No atomics; one value per row leaves the block:
        // se.acc_sum[colblk][grp][row] for the se.accB rows of a group that carry resamples.  Columns >= B of X are
        // zero and add zero.
        static_assert(NSQ == 0 && NW == 4, "EPI 10 is the fixed-X block");
        constexpr int PP = MT * 16;                          // pitch of a partial: the rows of a block
        double* sP = smem;                                   // [NW * 4][PP]
        double* sq = sP + (wave * 4 + kq) * PP + (lane & 15);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            double q = acc[m][0] * acc[m][0];
            q = __builtin_fma(acc[m][1], acc[m][1], q);
            q = __builtin_fma(acc[m][2], acc[m][2], q);
            q = __builtin_fma(acc[m][3], acc[m][3], q);
            sq[m * 16] = q;
        }
        __syncthreads();
        const int rows = se.accB;
        double* pp = se.acc_sum + ((size_t)colblk * n_groups + grp) * rows;
        for (int row = tid; row < rows; row += NT) {
            double w[NW];
#pragma unroll
            for (int v = 0; v < NW; ++v) {
                const double* p = sP + v * 4 * PP + row;
                w[v] = (p[0] + p[PP]) + (p[2 * PP] + p[3 * PP]);
            }
            pp[row] = (w[0] + w[1]) + (w[2] + w[3]);
        }
        return;
    }
    if constexpr (EPI == 9) {
        // second-moment-only block: tile j holds the raw m2 of pairs j * 16 .. + 15
        static_assert(MT == NSQ, "EPI 9 runs every tile against X^2");
#pragma unroll
        for (int j = 0; j < MT; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int pair = grp * (MT * 16) + j * 16 + kq + 4 * i;
                if (pair >= se.npairs || col >= ldr) continue;
                se.scale[(size_t)pair * ldr + col] = acc[j][i];
            }
        return;
    }
    if constexpr (EPI == 6) {
        // moment-only block writing the RAW first / second moments of its pairs (compact split-half)
        static_assert(MT == 2 * NSQ, "EPI 6 is a moment-only instantiation");
#pragma unroll
        for (int j = 0; j < NSQ; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int pair = grp * (NSQ * 16) + j * 16 + kq + 4 * i;
                if (pair >= se.npairs || col >= ldr) continue;
                se.scale[(size_t)pair * ldr + col] = acc[j][i];
                se.scale2[(size_t)pair * ldr + col] = acc[NSQ + j][i];
            }
        return;
    }
    if constexpr (EPI == 4) {
        // moment-only block (W0 = 0): tile j holds the first moments of pairs j * 16 .. + 15, tile
        // NSQ + j their second moments; 1 / std (ddof 1) of the resampled feature inside the cell
        // straight from the accumulators to the scale table
        static_assert(MT == 2 * NSQ, "EPI 4 is the moment-only instantiation");
#pragma unroll
        for (int j = 0; j < NSQ; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int pair = grp * (NSQ * 16) + j * 16 + kq + 4 * i;
                if (pair >= se.npairs || col >= ldr) continue;
                const double m1 = acc[j][i], m2 = acc[NSQ + j][i];
                const double nn = mom_n[pair];
                const double ss = m2 - m1 * m1 / nn;
                const double var = ss / (nn - 1.0);
                se.scale[(size_t)pair * ldr + col] = raw_ss_live(ss, nn, m2) ? sd_rsqrt(var) : 0.0;
            }
        return;
    }
    if constexpr (EPI == 3) {
        // data-only block: the scales of the group's (resample, cell) pairs for this block's 64 columns
        // come from the table, all loads up front (a load waited for between the stores below would
        // drain them: loads and stores share vmcnt on gfx950)
        const int nmu = se.npairs;
        double* sS3 = smem;                               // [nmu][64]
        int* s_out = reinterpret_cast<int*>(smem + (size_t)nmu * (NW * 16));
        int* s_mom = s_out + MT * 16;
        const double* sc0 = se.scale + (size_t)grp * nmu * ldr + colblk * (NW * 16);
        for (int idx = tid; idx < nmu * (NW * 16); idx += NT) {
            const int mi = idx / (NW * 16), c = idx - mi * (NW * 16);
            sS3[idx] = sc0[(size_t)mi * ldr + c];
        }
        for (int i = tid; i < MT * 16; i += NT) { s_out[i] = out_row[i]; s_mom[i] = mom_idx[i]; }
        __syncthreads();
        double* Rg = R + (size_t)grp * rows_per_group * ldr + col;
        const int cw = wave * 16 + (lane & 15);
        // the last group may hold fewer resamples than its block has room for: their rows (zero A
        // rows, no scale) are not stored -- the R scratch is sized for the resamples of the launch
        const int rows_valid = min(rows_per_group, se.accB - grp * rows_per_group);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            int orow[4];
            double sc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = m * 16 + kq + 4 * i;
                orow[i] = s_out[row];
                const int mi = s_mom[row];
                sc[i] = mi >= 0 ? sS3[mi * (NW * 16) + cw] : 1.0;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (orow[i] >= 0 && orow[i] < rows_valid) Rg[(size_t)orow[i] * ldr] = acc[m][i] * sc[i];
        }
        return;
    }
    if constexpr (EPI == 7) {
        // quadratic form (k_quad_*): the group's rows are rows s0 .. s0 + MT * 16 - 1 of ONE symmetric S x S matrix
        // C_l (group g: l = g % nl, s0 = (g / nl) * MT * 16; nl = se.J, S = se.accB), acc = (C_l X)[s][col];
        // the block adds X[s][col] * acc over its rows -- its share of x_col^T C_l x_col -- and writes ONE value per
        // column: se.acc_sum[grp][ldr].  The X rows are the ones the main loop just streamed (L2).
        if (NW > 4 && col >= ldr) return;
        const int s0 = qblk * (MT * 16);
        const int Srows = se.accB;
        const double* Xc = X + col - (size_t)(ks0 * 4) * ldx;   // (X was advanced to the block's first contraction row)
        double part = 0.0;
        // one tile at a time, addresses clamped and the value selected (no control flow around the loads), each
        // tile's four loads consumed before the next are issued: with the loop unrolled freely hipcc hoisted all
        // 4 MT loads above the first multiply and spilled them next to the accumulators (173 VGPRs at MT = 21,
        // VERDICT r4 weak #7)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            double xv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int sr = s0 + m * 16 + kq + 4 * i;
                const double x = Xc[(size_t)min(sr, Srows - 1) * ldx];
                xv[i] = sr < Srows ? x : 0.0;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) part = __builtin_fma(xv[i], acc[m][i], part);
            asm volatile("" : "+v"(part));          // (keeps tile m + 1's loads behind this tile's use)
        }
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (kq == 0) se.acc_sum[(size_t)grp * ldr + col] = part;
        return;
    }
    if constexpr (EPI == 2) {
        // accumulate over the resamples of the group, in a FIXED order (round 5; LDS atomics before: the order in which
        // concurrent adds land is not defined).  The block's (MT * 16 x NW * 16) tile goes through LDS two M tiles at a
        // time; thread (l, column) -- the only writer of its cell -- adds the rows that carry its LV in increasing row
        // order.  LDS: [2][L][ACCP] sums, [32][ACCP] staging, the row -> l map (the A stages are dead).
        constexpr int ACCP = NW * 16 + 16;      // LDS pitch of an l-row (PLSX_ACC_PITCH for 4 waves)
        constexpr int BCW = NW * 16;
        const int L = se.accL;
        double* sU = smem;
        double* sV = smem + (size_t)L * ACCP;
        double* sT = sV + (size_t)L * ACCP;                  // [32][ACCP]
        int* s_l = reinterpret_cast<int*>(sT + 32 * ACCP);
        for (int i = tid; i < 2 * L * ACCP; i += NT) smem[i] = 0.0;
        for (int i = tid; i < MT * 16; i += NT) s_l[i] = out_row[i];
        const int cw = wave * 16 + (lane & 15);
#pragma unroll
        for (int m0 = 0; m0 < MT; m0 += 2) {
            __syncthreads();
#pragma unroll
            for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (m0 + mm < MT) sT[(mm * 16 + kq + 4 * i) * ACCP + cw] = acc[m0 + mm][i];
            __syncthreads();
            for (int idx = tid; idx < L * BCW; idx += NT) {
                const int l = idx / BCW, c = idx - l * BCW;
                double u = sU[l * ACCP + c], v2 = sV[l * ACCP + c];
                for (int rl = 0; rl < 32 && m0 * 16 + rl < MT * 16; ++rl)
                    if (s_l[m0 * 16 + rl] == l) { const double v = sT[rl * ACCP + c]; u += v; v2 += v * v; }
                sU[l * ACCP + c] = u; sV[l * ACCP + c] = v2;
            }
        }
        __syncthreads();
        const int b0 = colblk * (NW * 16);
        double* ps = se.acc_sum + (size_t)grp * se.accB * L;
        double* pq = se.acc_sq + (size_t)grp * se.accB * L;
        for (int idx = tid; idx < NW * 16 * L; idx += NT) {
            const int c = idx / L, l = idx - c * L;
            if (b0 + c < se.accB) {
                ps[(size_t)(b0 + c) * L + l] = sU[l * ACCP + c];
                pq[(size_t)(b0 + c) * L + l] = sV[l * ACCP + c];
            }
        }
        return;
    }
    if constexpr (SPLIT && NSQ > 0) {
        // fused split-half: both halves from the first half's raw sums (see SplitEpi)
        const int nmu = se.nmu;
        const bool pre = se.off_pre > 0 && NW == 4;
        double* w5 = smem + wave * (5 * nmu * 16);           // u1, v1, u2, v2, sF : [5][nmu][16] per wave
        int* s_out = reinterpret_cast<int*>(smem + NW * 5 * nmu * 16);
        int* s_mom = s_out + MT * 16;
        const double* sRf = smem + se.off_pre;               // [Tpp][64] tile of Rfull (pre)
        double* s_rc = pre ? smem + se.off_pre + se.Tpp * (NW * 16)
                           : reinterpret_cast<double*>(s_mom + MT * 16);   // [MT*16][5]
        // row maps (ntab == 1); the R row inside the arrangement (orow mod 2 Tpp) rides in the
        // upper half of the word so the store loop does no integer division
        const int pitch2 = 2 * se.Tpp;
        for (int i = tid; i < MT * 16; i += NT) {
            const int orw = out_row[i];
            s_out[i] = orw < 0 ? -1 : (orw | ((orw % pitch2) << 20));
            s_mom[i] = mom_idx[i];
        }
        if (!pre)
            for (int i = tid; i < MT * 16 * 5; i += NT) s_rc[i] = se.rowc[(size_t)grp * MT * 16 * 5 + i];
        // moments of the first half sit in the accumulators of tiles W0+j / SQ0+j
#pragma unroll
        for (int j = 0; j < NSQ; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int mr = j * 16 + kq + 4 * i;
                if (mr >= nmu) continue;
                const int o = mr * 16 + (lane & 15);
                const double n1 = mom_n[(size_t)grp * nmom_pad + mr];
                const double m1 = acc[W0 + j][i], m2 = acc[SQ0 + j][i];
                const int jc = mr % se.J;
                const double nF = (double)se.cell_len[jc];
                const double SF = se.cellS1[(size_t)jc * ldr + col], SFF = se.cellS2[(size_t)jc * ldr + col];
                const double n2 = nF - n1;
                const bool ok = n1 > 1.5 && n2 > 1.5;
                // (the second half's moments are differences of the full sample's: their rounding bound is the full
                // sample's, twice -- one share for each of the two sums subtracted)
                const double ss1 = m2 - m1 * m1 / n1;
                const double var1 = ok ? ss1 / (n1 - 1.0) : 0.0;
                const double s2x = SF - m1, s2xx = SFF - m2;
                const double ss2 = s2xx - s2x * s2x / n2;
                const double var2 = ok ? ss2 / (n2 - 1.0) : 0.0;
                const double ssF = SFF - SF * SF / nF;
                const double varF = ssF / (nF - 1.0);
                w5[0 * nmu * 16 + o] = ok ? m1 / n1 : 0.0;
                w5[1 * nmu * 16 + o] = (ok && raw_ss_live(ss1, n1, m2)) ? 1.0 / sqrt(var1) : 0.0;
                w5[2 * nmu * 16 + o] = ok ? s2x / n2 : 0.0;
                w5[3 * nmu * 16 + o] = (ok && raw_ss_live(ss2, 2.0 * nF + 1.0, SFF)) ? 1.0 / sqrt(var2) : 0.0;
                w5[4 * nmu * 16 + o] = raw_ss_live(ssF, nF, SFF) ? sqrt(varF) : 0.0;
            }
        __syncthreads();
        double* Rg = R + (size_t)grp * rows_per_group * ldr + col;
#pragma unroll
        for (int m = 0; m < W0; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = m * 16 + kq + 4 * i;
                const int packed = s_out[row];
                if (packed < 0) continue;
                const int orow = packed & 0xfffff, t = packed >> 20;
                const int o = s_mom[row] * 16 + (lane & 15);
                const double* rc = s_rc + row * 5;
                const double c1 = acc[m][i];
                const double rf = pre ? sRf[t * (NW * 16) + wave * 16 + (lane & 15)]
                                      : se.Rfull[(size_t)t * ldr + col];
                const double cf = rf * rc[4] * w5[4 * nmu * 16 + o];
                const double r1 = (c1 - rc[0] * w5[o]) * rc[1] * w5[1 * nmu * 16 + o];
                const double r2 = ((cf - c1) - rc[2] * w5[2 * nmu * 16 + o]) * rc[3] * w5[3 * nmu * 16 + o];
                // non-temporal: the 2 x 83 MB per split are read back from HBM by later kernels
                __builtin_nontemporal_store(r1, &Rg[(size_t)orow * ldr]);
                __builtin_nontemporal_store(r2, &Rg[(size_t)(orow + se.Tpp) * ldr]);
            }
        return;
    }
    double* sS = smem + wave * (2 * NMOM * 16);      // m1 -> 1/std : [NMOM][16] per wave
    double* sQ = sS + NMOM * 16;                     // m2
    int* s_out = reinterpret_cast<int*>(smem + NW * 2 * NMOM * 16);   // row maps, shared
    int* s_mom = s_out + MT * 16;
    const int tab = (ntab > 1) ? (grp % ntab) * (MT * 16) : 0;
    for (int i = tid; i < MT * 16; i += NT) { s_out[i] = out_row[tab + i]; s_mom[i] = mom_idx[tab + i]; }
    if (NSQ > 0) {
#pragma unroll
        for (int j = 0; j < NSQ; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sS[j * 256 + (kq + 4 * i) * 16 + (lane & 15)] = acc[W0 + j][i];
                sQ[j * 256 + (kq + 4 * i) * 16 + (lane & 15)] = acc[SQ0 + j][i];
            }
    }
    __syncthreads();
    if (NSQ > 0) {
        for (int mr = kq; mr < NMOM; mr += 4) {
            const int o = mr * 16 + (lane & 15);
            const double m1 = sS[o], m2 = sQ[o];
            const double nn = mom_n[(size_t)grp * nmom_pad + mr];
            const double ss = m2 - m1 * m1 / nn;
            const double var = ss / (nn - 1.0);
            const double sc = raw_ss_live(ss, nn, m2) ? 1.0 / sqrt(var) : 0.0;
            sS[o] = sc;
            if (mom_out) {       // training mean / inverse std of the features (cross-validation)
                double* mo = mom_out + ((size_t)grp * nmom_pad + mr) * 2 * ldr + col;
                mo[0] = m1 / nn;
                mo[ldr] = sc;
            }
        }
        __syncthreads();
    }
    if (NW > 4 && col >= ldr) return;                 // (a block of 8 waves may hang over the last 64 columns)
    double* Rg = R + (size_t)(ntab > 1 ? grp / ntab : grp) * rows_per_group * ldr + col;
#pragma unroll
    for (int m = 0; m < W0; ++m) {
        int orow[4];
        double sc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = m * 16 + kq + 4 * i;
            orow[i] = s_out[row];
            const int mi = s_mom[row];
            sc[i] = (NSQ > 0 && mi >= 0) ? sS[mi * 16 + (lane & 15)] : 1.0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (orow[i] >= 0) Rg[(size_t)orow[i] * ldr] = acc[m][i] * sc[i];
    }
}

// ---------------------------------------------------------------------------
// K_RC: compact cross-product blocks -- ONE resample per block, contraction over the rows IT uses
// ---------------------------------------------------------------------------
// A bootstrap draws ~63 % of the rows of X (the rest have weight zero), the first half of a split holds
// S / 2: the dense layout of k_xprod packs ~7 resamples into a 24-tile block and contracts the block over
// all S rows -- the union of what seven resamples use -- i.e. multiplies 37 - 50 % zeros.  Here a block is
// one resample (group) x 128 feature columns and contracts over the resample's own rows: the X row behind
// contraction index k comes from a row table (k_split_rank: rank of the row among the used rows; the A
// operand is built at the rank, multiplicities folded in), padded with row 0 against zero A columns.
// What a block of ceil(T'/16) tiles loses against 24 tiles -- X fragments, A fragments and stores per MFMA
// all go up 6 x -- is halved again by giving every wave TWO 16-column tiles that interleave (lane c holds
// columns 2c, 2c+1 of the wave's 32): one 16-byte X load and one LDS read of A feed two MFMAs, and the
// epilogue stores 16 bytes per lane.
// Block id -> (group, column block): the 8 groups of a sweep go to ONE XCD per column block (slots s, s+1,
// .. of XCD x: groups 0..7 of column block (s / 8) * 8 + x); their sorted row lists advance together, so
// each row of the column block comes from HBM about once per sweep and from L2 for the other groups
// (measured: 11.9 GB fetched per 100 splits against 40 GB of row segments requested).
// The feature moments come from moment-only blocks of k_xprod (EPI 4 / 6) over all (resample, cell) pairs.
// EPI 3: R = (A . X) scaled by the 1 / std table (bootstraps; se.scale, se.npairs = cells, se.accB); MT up to 13
//        tiles (T' <= 208) at 3 or 2 waves per SIMD.  With se.nmu = T' (moment rows, compact_moment_rows) the block's
//        padding rows T' + j carry the cells' multiplicities: the first moments come out of its own accumulators, the
//        table holds the raw second moments (k_xprod EPI 9) and 1 / std is formed after the loop.
// EPI 5: fused split-half (both halves from the first half's raw sums and the arrangement's full-sample R:
//        se.Rfull, se.rowc, se.scale / scale2 = raw first-half moments, se.cellS1 / S2, se.cell_len).
// EPI 8: the raw first-half sums of one split per block (the one-pass reader k_split_fused rebuilds both halves).
// A block is short (~80 k-steps at the headline shape, 788 k blocks per launch), so what it does outside its loop is
// kept to ONE barrier and two dependent round trips in front of the loop and to stores behind it (epilogues 3, 8):
// the kernel body says how.
// TAIL: the last tile holds <= 4 live rows and runs on the 4x4x4 shape (16 instead of 64 pipe cycles;
//       A = the tile's rows 0..3 for every block, B = the X fragment as it is, the result lands where
//       register 0 of the 16x16 tile would).
__device__ __forceinline__ d2 load_x2_buf(const double* base, int voff)
{
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, 0x7fffffff, PLSX_RSRC_FLAGS);
    return __builtin_bit_cast(d2, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0));
}

// LDS of a block, in doubles from smem: the row maps (2 x MT * 16 ints, filled once in the prologue and read by the
// epilogue: an area of their own, nothing is staged after the loop), the two A stages, the row table (byte offsets
// of the block's X rows), and for epilogue 3 with more cells than a lane keeps in registers the 1 / std table.
// plsx_compact.hip sizes the launch with the same three functions.
__host__ __device__ constexpr int compact_stage_lds(int MT, int KT) { return ((KT * MT * 64 + 127) / 128) * 128; }
// cells whose 1 / std (16 bytes per lane and cell) a lane of epilogue 3 holds in registers: they arrive in the
// registers that hold the next stage's X fragments in every pass but the last, so as many as a stage has k-steps;
// four at the most (the store loop selects among them with compares)
// (NC column tiles per wave: 16 NC bytes per lane and cell, in the 16 NC bytes per k-step of the X fragments -- the
// same count at either width)
__host__ __device__ constexpr int compact_scale_regs(int KT, int NC = 2) { return KT < 4 ? KT : 4; }
__host__ __device__ constexpr size_t compact_lds_bytes(int MT, int KT, int EPI, int nks, int J, int NC = 2)
{
    const size_t loop = (size_t)MT * 16 * 8 + (size_t)2 * compact_stage_lds(MT, KT) * 8 + (size_t)nks * 4 * 4;
    if (EPI == 3) return loop + (J > compact_scale_regs(KT, NC) ? (size_t)J * (64 * NC) * 8 : 0);
    // epilogue 5: u1, v1, u2, v2, sF : [5][J][128] and the row constants [MT * 16][5] over the stages and the table
    const size_t epi5 = (size_t)MT * 16 * 8 + (size_t)5 * J * 128 * 8 + (size_t)MT * 16 * 5 * 8;
    return EPI == 5 && epi5 > loop ? epi5 : loop;
}

// waves per SIMD the register allocation is held to: what each variant runs at (epilogue 3: 7 / 6 at two tiles with /
// without the tail, 5 at four tiles with the tail -- the headline --, 4 otherwise up to six tiles, 3 up to nine and at
// ten with the tail, 2 beyond)
__host__ __device__ constexpr int compact_waves(int MT, int EPI, bool TAIL, int NC = 2)
{
    // four column tiles per wave (epilogue 3, up to four tiles of rows): twice the accumulators and X fragments -- 4 waves
    // at one tile, 3 beyond (the headline, four tiles with the tail: 160 registers), 2 at four tiles without the tail
    if (NC == 4) return MT == 1 ? 4 : (MT == 4 && !TAIL) ? 2 : 3;
    if (EPI == 3 && MT == 2) return TAIL ? 7 : 6;            // (72 / 80 registers: where they stood before they had moment rows to read)
    if (EPI == 3) return MT > 10 ? 2 : MT == 10 ? (TAIL ? 3 : 2) : MT > 6 ? 3 : MT > 4 ? 4 : (MT == 4 && TAIL) ? 5 : 4;
    return (EPI == 5 && MT == 4 && !TAIL) ? 3 : 4;
}

// NC = 4: FOUR interleaved column tiles per wave (epilogue 3, up to four tiles of rows).  Lane c holds columns 4c .. 4c+3
// of the wave's 64, a block is 4 waves x 64 = 256 columns: one LDS read of an A tile feeds four MFMAs, a lane loads 32
// contiguous bytes of an X row (512 per row and wave) and stores 32 per row, and a launch has half the blocks -- half
// the A re-staging, table fills, prologue round trips, barriers and dispatches per column.  The A stages, the row
// table, the row maps, the single prologue barrier and the two-passes-per-trip loop are those of the two-tile body
// below; every element of R receives the same products in the same k order, and 1 / std the same operations: the
// same bits.  The comments of the two-tile body are not repeated here.
template <int MT, int KT, bool TAIL>
__device__ __forceinline__ void compact_wide_block(double* smem, const double* __restrict__ Afrag, size_t group_stride,
                                                   const double* __restrict__ X, int ldx, int nks,
                                                   double* __restrict__ R, int ldr, int rows_per_group,
                                                   const int* __restrict__ out_row, const int* __restrict__ mom_idx,
                                                   const double* __restrict__ mom_n, int n_groups, int ncolblk,
                                                   const SplitEpi& se)
{
    constexpr int NC = 4, NW = 4, NT = NW * 64, BC = NW * 16 * NC;
    constexpr int STAGE = KT * MT * 64;
    constexpr int STAGE_LDS = compact_stage_lds(MT, KT);
    constexpr int PASSES = (STAGE + NT * 2 - 1) / (NT * 2);
    constexpr bool EVEN = (STAGE % (NT * 2)) == 0;
    constexpr int MF = TAIL ? MT - 1 : MT;
    constexpr int NSCR = compact_scale_regs(KT, NC);
    static_assert(MT * 16 <= NT, "the row maps are staged by one thread per row");
    const int ncb = (ncolblk + 7) & ~7;
    const int sweep = blockIdx.x / (8 * ncb);
    const int within = blockIdx.x - sweep * (8 * ncb);
    const int slot = within >> 3;
    const int grp = sweep * 8 + (slot & 7);
    const int colblk = (slot >> 3) * 8 + (within & 7);
    if (grp >= n_groups || colblk >= ncolblk) return;
    const double* Ag = Afrag + (size_t)grp * group_stride;
    const int swave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);

    d4 acc[NC][MF > 0 ? MF : 1];
    double tl[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        tl[c] = 0.0;
#pragma unroll
        for (int m = 0; m < MF; ++m) acc[c][m] = (d4){0.0, 0.0, 0.0, 0.0};
    }

    int* s_out = reinterpret_cast<int*>(smem);
    double* sStage = smem + MT * 16;
    int* s_tab = reinterpret_cast<int*>(sStage + 2 * STAGE_LDS);
    const int J3 = se.npairs;
    double* sW = reinterpret_cast<double*>(s_tab + nks * 4) + swave * (J3 * 64);   // [J3][64]: 1 / std, this wave's columns
    d2 scr[NSCR][2];                                          // ... or per cell in registers (columns 0, 1 | 2, 3 of the lane)
    const int mrow0 = se.nmu;
    int cnt_lo[NSCR], cnt_hi[NSCR];
    {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kq = lane >> 4;
    const int cw = wave * 64 + 4 * (lane & 15);              // this lane's first column inside the block
    const int col = colblk * BC + cw;
    const bool live = col < ldr;                             // (ldr is a multiple of 64: whole waves)
    const int lcol8 = (live ? col : 0) * 8;
    const int toff = (lane & 48) + (lane & 3) - lane;

    const int* tabg = se.row_tab + (size_t)grp * nks * 4;
    const int ldx8 = ldx * 8;
    int row0[KT];
#pragma unroll
    for (int s = 0; s < KT; ++s) row0[s] = tabg[s * 4 + kq];
    stage_copy_buf<NT, PASSES, EVEN, STAGE>(Ag, sStage, tid, swave);
    int orw = -1, mix = -1;
    if (tid < MT * 16) {
        orw = out_row[tid];
        mix = mom_idx[tid];
    }
    const int ksteps = max(1, (se.row_cnt[grp] + 3) >> 2);
    const int nkt = (ksteps + KT - 1) / KT;
    const int ntab = nkt * KT * 4;
    auto tab_load = [&](int i0, int (&v)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = tabg[min(i0 + u * NT + tid, ntab - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) asm volatile("" : "+v"(v[u]));
    };
    auto tab_store = [&](int i0, const int (&v)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u * NT + tid < ntab) s_tab[i0 + u * NT + tid] = v[u] * ldx8;
    };
    int tv[4];
    tab_load(0, tv);
    d2 xa[KT][2], xb[KT][2];
#pragma unroll
    for (int s = 0; s < KT; ++s) {
        xa[s][0] = load_x2_buf(X, row0[s] * ldx8 + lcol8);
        xa[s][1] = load_x2_buf(X, row0[s] * ldx8 + lcol8 + 16);
    }
    tab_store(0, tv);
    for (int i0 = 4 * NT; i0 < ntab; i0 += 4 * NT) { tab_load(i0, tv); tab_store(i0, tv); }
    if (tid < MT * 16) {
        const int rows_valid = min(rows_per_group, se.accB - grp * rows_per_group);
        s_out[tid] = (orw < 0 || orw >= rows_valid) ? -1 : (orw | ((mix + 1) << 16));
    }
#pragma unroll
    for (int s = 0; s < KT; ++s) { asm volatile("" : "+v"(xa[s][0])); asm volatile("" : "+v"(xa[s][1])); }
    __syncthreads();

    const double* sA0 = sStage + lane;
    const double* sT0 = sA0 + toff;
    auto contract = [&](auto curc, const d2 (&xc)[KT][2], auto full, int nlive) {
        const int cur = curc;
        const double* sA = sA0 + cur * STAGE_LDS;
        const double* sT = sT0 + cur * STAGE_LDS;
#pragma unroll
        for (int s = 0; s < KT; ++s) {
            if (!decltype(full)::value && s >= nlive) continue;
            const double b[NC] = {xc[s][0].x, xc[s][0].y, xc[s][1].x, xc[s][1].y};
#pragma unroll
            for (int m = 0; m < MF; ++m) {
                const double a = sA[(s * MT + m) * 64];
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[c][m] = mfma_f64(a, b[c], acc[c][m]);
            }
            if constexpr (TAIL) {
                const double a = sT[(s * MT + MT - 1) * 64];
#pragma unroll
                for (int c = 0; c < NC; ++c) tl[c] = mfma_f64_4x4(a, b[c], tl[c]);
            }
        }
    };
    const int* tp = s_tab + KT * 4 + kq;
    const double* An = Ag + STAGE;
    auto pass = [&](auto curc, const d2 (&xc)[KT][2], d2 (&xn)[KT][2]) {
        constexpr int CUR = decltype(curc)::value;
        stage_copy_buf<NT, PASSES, EVEN, STAGE>(An, sStage + (CUR ^ 1) * STAGE_LDS, tid, swave);
#pragma unroll
        for (int s = 0; s < KT; ++s) {
            xn[s][0] = load_x2_buf(X, tp[s * 4] + lcol8);
            xn[s][1] = load_x2_buf(X, tp[s * 4] + lcol8 + 16);
        }
        An += STAGE;
        tp += KT * 4;
        contract(curc, xc, std::true_type(), KT);
        __syncthreads();
    };
    // the last pass: the block's 1 / std (or raw m2) per cell, 32 bytes per lane and cell into registers, or each wave's
    // own 64 columns of the table by LDS-DMA (two pieces of 4 bytes per lane and cell) into its part of the LDS area
    auto last = [&](int cur, const d2 (&xc)[KT][2]) {
#pragma unroll
        for (int j = 0; j < NSCR; ++j) { scr[j][0] = scr[j][1] = (d2){1.0, 1.0}; cnt_lo[j] = 0; cnt_hi[j] = 0; }
        if (J3 <= NSCR) {
            if (mrow0 > 0) {
#pragma unroll
                for (int j = 0; j < NSCR; ++j)
                    if (j < J3) {
                        const double v = mom_n[(size_t)grp * J3 + j];
                        cnt_lo[j] = __builtin_amdgcn_readfirstlane(__double2loint(v));
                        cnt_hi[j] = __builtin_amdgcn_readfirstlane(__double2hiint(v));
                    }
            }
#pragma unroll
            for (int j = 0; j < NSCR; ++j)
                if (j < J3) {
                    const char* p = reinterpret_cast<const char*>(se.scale + ((size_t)grp * J3 + j) * ldr) + lcol8;
                    scr[j][0] = *reinterpret_cast<const d2*>(p);
                    scr[j][1] = *reinterpret_cast<const d2*>(p + 16);
                }
        } else if (live) {
            __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                (void*)(se.scale + (size_t)grp * J3 * ldr + colblk * BC + swave * 64), (short)0, 0x7fffffff, PLSX_RSRC_FLAGS);
            const int ln4 = __lane_id() * 4;
            for (int j = 0; j < J3; ++j) {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rs, (__attribute__((address_space(3))) void*)(sW + j * 64), 4, ln4, j * ldr * 8, 0, 0);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rs, (__attribute__((address_space(3))) void*)(sW + j * 64 + 32), 4, ln4, j * ldr * 8 + 256, 0, 0);
            }
        }
        contract(cur, xc, std::false_type(), ksteps - (nkt - 1) * KT);
    };
    {
        std::integral_constant<int, 0> c0;
        std::integral_constant<int, 1> c1;
        int kt = 0, cur = 0;
        for (; kt + 2 < nkt; kt += 2) { pass(c0, xa, xb); pass(c1, xb, xa); }
        if (kt + 1 < nkt) {
            pass(c0, xa, xb);
#pragma unroll
            for (int s = 0; s < KT; ++s) { xa[s][0] = xb[s][0]; xa[s][1] = xb[s][1]; }
            cur = 1;
        }
        last(cur, xa);
    }
    }

    // ---- moment rows: 1 / std from the block's own first moments --------------------------------------------------
    // scr[j] holds m2 of the lane's four columns, m1 sits in row r = T' + j of the last tile (lane 16 (r % 4) + column,
    // register (r % 16) / 4).  The four lanes that share the four columns would all form the same four values: the
    // 16-lane row q = lane >> 4 forms column q's, ONE chain of two divisions and a square root per lane and cell as in
    // the two-tile body, and the rows exchange.
    if (mrow0 > 0 && J3 <= NSCR) {
        const int ln = __lane_id();
        const int q = ln >> 4;
#pragma unroll
        for (int j = 0; j < NSCR; ++j) {
            if (j >= J3) continue;
            const int r = mrow0 + j;
            const int src = ((r & 3) << 4) | (ln & 15);
            double m1 = 0.0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                double a;
                if constexpr (TAIL) a = tl[c];
                else {
                    const int ri = (r & 15) >> 2;
                    a = acc[c][MT - 1][0];
#pragma unroll
                    for (int i = 1; i < 4; ++i)
                        if (ri == i) a = acc[c][MT - 1][i];
                }
                const double v = __shfl(a, src);
                if (q == c) m1 = v;
            }
            const double nn = __hiloint2double(cnt_hi[j], cnt_lo[j]);
            const double m2 = q == 0 ? scr[j][0].x : q == 1 ? scr[j][0].y : q == 2 ? scr[j][1].x : scr[j][1].y;
            const double ss = m2 - m1 * m1 / nn;
            const double var = ss / (nn - 1.0);
            double sc = raw_ss_live(ss, nn, m2) ? sd_rsqrt(var) : 0.0;
            asm volatile("" : "+v"(sc));
            const int c15 = ln & 15;
            scr[j][0] = (d2){__shfl(sc, c15), __shfl(sc, c15 | 16)};
            scr[j][1] = (d2){__shfl(sc, c15 | 32), __shfl(sc, c15 | 48)};
        }
    }

    // ---- epilogue: stores (the lane's constants derived again, opaque to the compiler) ------------------------------
    int tid16 = threadIdx.x * 16;
    asm volatile("" : "+v"(tid16));
    const int tid = tid16 >> 4, lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
    const int cw = wave * 64 + 4 * (lane & 15), col = colblk * BC + cw;
    if (col >= ldr) return;
    if (J3 > NSCR) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (this wave's own copy of its scales)
    double* Rg = R + (size_t)grp * rows_per_group * ldr + col;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (TAIL && m == MT - 1 && i > 0) break;
            const int packed = s_out[m * 16 + kq + 4 * i];
            if (packed < 0) continue;
            const int orow = packed & 0xffff, mi = (packed >> 16) - 1;
            d2 s0 = (d2){1.0, 1.0}, s1 = (d2){1.0, 1.0};
            if (J3 > NSCR) {
                if (mi >= 0) {
                    s0 = *reinterpret_cast<const d2*>(&sW[mi * 64 + 4 * (lane & 15)]);
                    s1 = *reinterpret_cast<const d2*>(&sW[mi * 64 + 4 * (lane & 15) + 2]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < NSCR; ++j)
                    if (mi == j) { s0 = scr[j][0]; s1 = scr[j][1]; }
            }
            double v[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) v[c] = (TAIL && m == MT - 1) ? tl[c] : acc[c][m < MF ? m : 0][i];
            d2* dst = reinterpret_cast<d2*>(&Rg[(size_t)orow * ldr]);
            // (ordinary stores: nontemporal ones, as epilogue 8 has, measured within the launch-to-launch spread at either
            // width, profiles/compact_wide_compare.txt)
            dst[0] = (d2){v[0] * s0.x, v[1] * s0.y};
            dst[1] = (d2){v[2] * s1.x, v[3] * s1.y};
        }
}

template <int MT, int KT, int EPI, bool TAIL, int NC = 2>
__global__ __launch_bounds__(256, compact_waves(MT, EPI, TAIL, NC))
void k_xprod_compact(const double* __restrict__ Afrag, size_t group_stride,
                     const double* __restrict__ X, int ldx, int nks,
                     double* __restrict__ R, int ldr, int rows_per_group,
                     const int* __restrict__ out_row, const int* __restrict__ mom_idx,
                     const double* __restrict__ mom_n, int n_groups, int ncolblk, SplitEpi se)
{
    static_assert(EPI == 3 || EPI == 5 || EPI == 8, "compact blocks: bootstrap (3), fused split-half (5) or raw first-half sums (8)");
    static_assert(NC == 2 || (NC == 4 && EPI == 3 && MT <= 4), "four column tiles per wave: bootstraps of up to four tiles");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    if constexpr (NC == 4) {
        compact_wide_block<MT, KT, TAIL>(smem, Afrag, group_stride, X, ldx, nks, R, ldr, rows_per_group, out_row, mom_idx,
                                         mom_n, n_groups, ncolblk, se);
        return;
    }
    constexpr int NW = 4, NT = NW * 64, BC = NW * 32;       // threads, columns of a block
    constexpr int STAGE = KT * MT * 64;
    constexpr int STAGE_LDS = compact_stage_lds(MT, KT);
    constexpr int PASSES = (STAGE + NT * 2 - 1) / (NT * 2);
    constexpr bool EVEN = (STAGE % (NT * 2)) == 0;
    constexpr int MF = TAIL ? MT - 1 : MT;                   // tiles on the 16x16x4 shape
    constexpr int NSCR = compact_scale_regs(KT);
    static_assert(MT * 16 <= NT, "the row maps are staged by one thread per row");
    const int ncb = (ncolblk + 7) & ~7;
    const int sweep = blockIdx.x / (8 * ncb);
    const int within = blockIdx.x - sweep * (8 * ncb);
    const int slot = within >> 3;
    const int grp = sweep * 8 + (slot & 7);
    const int colblk = (slot >> 3) * 8 + (within & 7);
    if (grp >= n_groups || colblk >= ncolblk) return;         // (the whole block: before its only barrier outside the loop)
    const double* Ag = Afrag + (size_t)grp * group_stride;
    const int swave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);

    d4 acc0[MF > 0 ? MF : 1], acc1[MF > 0 ? MF : 1];
#pragma unroll
    for (int m = 0; m < MF; ++m) { acc0[m] = (d4){0.0, 0.0, 0.0, 0.0}; acc1[m] = (d4){0.0, 0.0, 0.0, 0.0}; }
    double tl0 = 0.0, tl1 = 0.0;

    int* s_out = reinterpret_cast<int*>(smem);
    int* s_mom = s_out + MT * 16;
    double* sStage = smem + MT * 16;
    int* s_tab = reinterpret_cast<int*>(sStage + 2 * STAGE_LDS);
    const int J3 = se.npairs;                                 // (epilogue 3: cells)
    double* sW = reinterpret_cast<double*>(s_tab + nks * 4) + swave * (J3 * 32);   // [J3][32]: 1 / std, this wave's columns
    d2 scr[NSCR];                                             // ... or per cell in registers
    // Epilogue 3 with se.nmu = T' > 0 (moment rows): row T' + j of the block -- a padding row of its last tile -- holds the
    // multiplicities of cell j's drawn rows, so the accumulators of that row are m1 = sum w x of the block's columns;
    // the table holds the raw m2 (k_xprod EPI 9) and the epilogue forms 1 / std from the two and the cell's count.
    const int mrow0 = (EPI == 3) ? se.nmu : 0;
    int cnt_lo[NSCR], cnt_hi[NSCR];                           // draws inside cell j, a double in two scalar registers
    {   // ---- prologue and main loop (a scope of their own: the epilogue declares its lane constants again) ------
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kq = lane >> 4;
    const int cw = wave * 32 + 2 * (lane & 15);              // this lane's (even) column inside the block
    const int col = colblk * BC + cw;
    const bool live = col < ldr;                             // (ldr is a multiple of 64: whole waves)
    const int lcol8 = (live ? col : 0) * 8;                  // byte offset of the lane's columns in a row of X (0: beyond ldr)
    const int toff = (lane & 48) + (lane & 3) - lane;        // TAIL: lane 16 k + 4 blk + i -> fragment position 16 k + i

    // ---- prologue: everything the block needs besides its A stages and X rows, behind ONE barrier ----------------
    // Every lane fetches the table entries of stage 0 for itself, so its first X loads wait for one round trip, not
    // for the table's way through LDS; the A stage-0 copy, the row maps and the table are in flight meanwhile.
    // The table holds rows; its LDS copy holds their byte offsets in X (row * ldx * 8, the 32-bit range x_off always
    // had), multiplied here once per entry instead of once per lane, k-step and pass.
    // Padding entries (the table is zero beyond the block's rows: row 0 against zero A columns) come along as they are.
    const int* tabg = se.row_tab + (size_t)grp * nks * 4;
    const int ldx8 = ldx * 8;
    int row0[KT];
#pragma unroll
    for (int s = 0; s < KT; ++s) row0[s] = tabg[s * 4 + kq];
    stage_copy_buf<NT, PASSES, EVEN, STAGE>(Ag, sStage, tid, swave);
    int orw = -1, mix = -1;
    if (tid < MT * 16) {
        orw = out_row[tid];
        if (EPI != 8) mix = mom_idx[tid];
    }
    // any mask / index list is legal: the tables are sized for S rows, the block contracts over its own count
    const int ksteps = max(1, (se.row_cnt[grp] + 3) >> 2);
    const int nkt = (ksteps + KT - 1) / KT;
    const int ntab = nkt * KT * 4;                            // live entries, whole stages (<= nks * 4)
    // four entries per thread and trip, all four loads issued before the first is waited for
    auto tab_load = [&](int i0, int (&v)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = tabg[min(i0 + u * NT + tid, ntab - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) asm volatile("" : "+v"(v[u]));    // (or hipcc sinks a load into its guarded store)
    };
    auto tab_store = [&](int i0, const int (&v)[4]) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u * NT + tid < ntab) s_tab[i0 + u * NT + tid] = v[u] * ldx8;
    };
    int tv[4];
    tab_load(0, tv);
    d2 xa[KT], xb[KT];
#pragma unroll
    for (int s = 0; s < KT; ++s) xa[s] = load_x2_buf(X, row0[s] * ldx8 + lcol8);
    tab_store(0, tv);
    for (int i0 = 4 * NT; i0 < ntab; i0 += 4 * NT) { tab_load(i0, tv); tab_store(i0, tv); }
    if (tid < MT * 16) {
        if constexpr (EPI == 3) {
            // one word per row: the R row and the row's cell + 1; rows of resamples beyond the launch's last one (the
            // last group may hold fewer than its block has room for: zero A rows, no scale) are not stored
            const int rows_valid = min(rows_per_group, se.accB - grp * rows_per_group);
            s_out[tid] = (orw < 0 || orw >= rows_valid) ? -1 : (orw | ((mix + 1) << 16));
        } else if constexpr (EPI == 5) {
            // the R row inside the arrangement (orow mod 2 Tpp) rides in the upper half of the word so the store
            // loop does no integer division
            s_out[tid] = orw < 0 ? -1 : (orw | ((orw % (2 * se.Tpp)) << 20));
            s_mom[tid] = mix;
        } else {
            s_out[tid] = orw;
        }
    }
    // (first X fragments resident before the loop: a load still pending at the loop header makes hipcc place a
    // near-draining s_waitcnt right after the next stage's loads are issued)
#pragma unroll
    for (int s = 0; s < KT; ++s) asm volatile("" : "+v"(xa[s]));
    __syncthreads();

    // ---- main loop --------------------------------------------------------------------------------------------------
    // the MFMAs of one stage: buffer CUR, X fragments xc; the first `nlive` k-steps when the stage may be partial
    const double* sA0 = sStage + lane;                       // this lane's word of a fragment, buffer 0
    const double* sT0 = sA0 + toff;                          // ... of the tail tile's fragment
    auto contract = [&](auto curc, const d2 (&xc)[KT], auto full, int nlive) {
        const int cur = curc;
        const double* sA = sA0 + cur * STAGE_LDS;
        const double* sT = sT0 + cur * STAGE_LDS;
#pragma unroll
        for (int s = 0; s < KT; ++s) {
            if (!decltype(full)::value && s >= nlive) continue;    // (no break: the loop must unroll, xc[s] is a register)
            const double b0 = xc[s].x, b1 = xc[s].y;
#pragma unroll
            for (int m = 0; m < MF; ++m) {
                const double a = sA[(s * MT + m) * 64];
                acc0[m] = mfma_f64(a, b0, acc0[m]);
                acc1[m] = mfma_f64(a, b1, acc1[m]);
            }
            if constexpr (TAIL) {
                const double a = sT[(s * MT + MT - 1) * 64];
                tl0 = mfma_f64_4x4(a, b0, tl0);
                tl1 = mfma_f64_4x4(a, b1, tl1);
            }
        }
    };
    // One pass before the last: stage kt + 1 of A by LDS-DMA into the other buffer and its X fragments into the OTHER
    // register set, then the MFMAs of stage kt.  The loop runs two passes per trip, so the buffer is a constant and the
    // register sets swap by name (no moves); the table's LDS address and the A source step by one stage per pass, and
    // the X offset of a k-step is its table entry plus the lane's column bytes: one add.
    const int* tp = s_tab + KT * 4 + kq;
    const double* An = Ag + STAGE;
    auto pass = [&](auto curc, const d2 (&xc)[KT], d2 (&xn)[KT]) {
        constexpr int CUR = decltype(curc)::value;
        stage_copy_buf<NT, PASSES, EVEN, STAGE>(An, sStage + (CUR ^ 1) * STAGE_LDS, tid, swave);
#pragma unroll
        for (int s = 0; s < KT; ++s) xn[s] = load_x2_buf(X, tp[s * 4] + lcol8);
        An += STAGE;
        tp += KT * 4;
        contract(curc, xc, std::true_type(), KT);
        __syncthreads();             // (drains the DMA issued in this pass, then barrier)
    };
    // The last pass fetches no further stage.  Epilogue 3 issues its only loads here instead, so that they land
    // under the last MFMAs and the epilogue is stores only: the block's 1 / std per cell, 16 bytes per lane and cell
    // into registers (up to NSCR cells), or each wave's own 32 columns of the table by LDS-DMA into its part of an
    // LDS area of its own -- read back by that wave alone, so its wait for the copy is all the ordering it needs.
    auto last = [&](int cur, const d2 (&xc)[KT]) {
#pragma unroll
        for (int j = 0; j < NSCR; ++j) { scr[j] = (d2){1.0, 1.0}; cnt_lo[j] = 0; cnt_hi[j] = 0; }
        if constexpr (EPI == 3) {
            if (J3 <= NSCR) {
                if (mrow0 > 0) {
#pragma unroll
                    for (int j = 0; j < NSCR; ++j)
                        if (j < J3) {
                            const double v = mom_n[(size_t)grp * J3 + j];
                            cnt_lo[j] = __builtin_amdgcn_readfirstlane(__double2loint(v));
                            cnt_hi[j] = __builtin_amdgcn_readfirstlane(__double2hiint(v));
                        }
                }
#pragma unroll
                for (int j = 0; j < NSCR; ++j)
                    if (j < J3)                                // (lcol8: the loop's own register, not lcol kept beside it)
                        scr[j] = *reinterpret_cast<const d2*>(
                            reinterpret_cast<const char*>(se.scale + ((size_t)grp * J3 + j) * ldr) + lcol8);
            } else if (live) {
                // one piece per cell: the wave's 256 bytes of the cell's table row, 4 bytes per lane (whole pieces of
                // 16 bytes per lane would hold four cells: with lanes beyond the last cell clamped onto it the copies came
                // out wrong whenever the cells were no multiple of four)
                __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                    (void*)(se.scale + (size_t)grp * J3 * ldr + colblk * BC + swave * 32), (short)0, 0x7fffffff, PLSX_RSRC_FLAGS);
                const int ln4 = __lane_id() * 4;              // (not `lane`: that would be one more register across the loop)
                for (int j = 0; j < J3; ++j)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(
                        rs, (__attribute__((address_space(3))) void*)(sW + j * 32), 4, ln4, j * ldr * 8, 0, 0);
            }
        }
        contract(cur, xc, std::false_type(), ksteps - (nkt - 1) * KT);
        if constexpr (EPI == 5) __syncthreads();   // (its epilogue builds tables over the stages)
    };
    {
        std::integral_constant<int, 0> c0;
        std::integral_constant<int, 1> c1;
        int kt = 0, cur = 0;
        for (; kt + 2 < nkt; kt += 2) { pass(c0, xa, xb); pass(c1, xb, xa); }
        if (kt + 1 < nkt) {
            pass(c0, xa, xb);
#pragma unroll
            for (int s = 0; s < KT; ++s) xa[s] = xb[s];      // (once per block)
            cur = 1;
        }
        last(cur, xa);
    }
    }

    // ---- moment rows (epilogue 3): 1 / std from the block's own first moments ------------------------------------
    // scr[j] holds m2 of the lane's two columns; m1 sits in the last tile's accumulators of row r = T' + j: register
    // (r % 16) / 4 of lane 16 (r % 4) + column (the tail tile has register 0 only).  var and 1 / std as epilogue 4 of
    // k_xprod forms them.  The four lanes that share a column pair would all form the same two values: the lanes of
    // the even 16-lane rows form the first column's, those of the odd rows the second's, and neighbouring rows swap --
    // ONE chain of two divisions and a square root per cell instead of two (vector fp64 work takes issue slots from
    // the other waves' MFMAs), and few enough temporaries next to the accumulators: with both chains in flight
    // <10,1,3,true> spilled.  The step stands before the epilogue's lane constants exist, for the same reason; every
    // wave runs it, live columns or not.
    if constexpr (EPI == 3) {
        if (mrow0 > 0 && J3 <= NSCR) {
            const int ln = __lane_id();
            const bool second = (ln & 16) != 0;
#pragma unroll
            for (int j = 0; j < NSCR; ++j) {
                if (j >= J3) continue;
                const int r = mrow0 + j;
                double a0, a1;
                if constexpr (TAIL) { a0 = tl0; a1 = tl1; }
                else {
                    const int ri = (r & 15) >> 2;
                    a0 = acc0[MT - 1][0]; a1 = acc1[MT - 1][0];
#pragma unroll
                    for (int q = 1; q < 4; ++q)
                        if (ri == q) { a0 = acc0[MT - 1][q]; a1 = acc1[MT - 1][q]; }
                }
                const int src = ((r & 3) << 4) | (ln & 15);
                const double nn = __hiloint2double(cnt_hi[j], cnt_lo[j]);
                const double m1x = __shfl(a0, src), m1y = __shfl(a1, src);
                const double m1 = second ? m1y : m1x, m2 = second ? scr[j].y : scr[j].x;
                const double ss = m2 - m1 * m1 / nn;
                const double var = ss / (nn - 1.0);
                double sc = raw_ss_live(ss, nn, m2) ? sd_rsqrt(var) : 0.0;
                asm volatile("" : "+v"(sc));
                const double other = __shfl_xor(sc, 16);
                scr[j] = second ? (d2){other, sc} : (d2){sc, other};
            }
        }
    }

    // ---- epilogue: stores -----------------------------------------------------------------------------------------
    // The lane's constants are derived again from the thread id, opaque to the compiler: carried across the loop they
    // took <4,3,3,true> past 96 VGPRs (5 -> 4 waves per SIMD).
    int tid16 = threadIdx.x * 16;                             // (the value the loop's LDS-DMA offset already holds)
    if constexpr (EPI != 5) asm volatile("" : "+v"(tid16));   // (epilogue 5 spills two registers more with it than without)
    const int tid = tid16 >> 4, lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
    const int cw = wave * 32 + 2 * (lane & 15), col = colblk * BC + cw;
    const bool live = col < ldr;
    // value of (tile m, register i), column 0 / 1 of the lane; the tail tile has register 0 only
    auto val0 = [&](int m, int i) -> double { return (TAIL && m == MT - 1) ? tl0 : acc0[m < MF ? m : 0][i]; };
    auto val1 = [&](int m, int i) -> double { return (TAIL && m == MT - 1) ? tl1 : acc1[m < MF ? m : 0][i]; };

    if constexpr (EPI == 8) {
        // raw first-half sums C_1 = A_1 . X of ONE split per block, stored once (slot = split): the fused reader
        // (k_split_fused) rebuilds both z-scored halves from them and the arrangement's full-sample cross-product,
        // so this leg writes half the bytes of epilogue 5 and spends no arithmetic on them
        if (!live) return;
        double* Rg = R + (size_t)grp * rows_per_group * ldr + col;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (TAIL && m == MT - 1 && i > 0) break;
                const int orow = s_out[m * 16 + kq + 4 * i];
                if (orow < 0) continue;
                __builtin_nontemporal_store((d2){val0(m, i), val1(m, i)}, reinterpret_cast<d2*>(&Rg[(size_t)orow * ldr]));
            }
        return;
    } else if constexpr (EPI == 3) {
        if (!live) return;
        if (J3 > NSCR) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (this wave's own copy of its scales)
        double* Rg = R + (size_t)grp * rows_per_group * ldr + col;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (TAIL && m == MT - 1 && i > 0) break;
                const int packed = s_out[m * 16 + kq + 4 * i];
                if (packed < 0) continue;
                const int orow = packed & 0xffff, mi = (packed >> 16) - 1;
                d2 sc = (d2){1.0, 1.0};
                if (J3 > NSCR) {
                    if (mi >= 0) sc = *reinterpret_cast<const d2*>(&sW[mi * 32 + 2 * (lane & 15)]);
                } else {
#pragma unroll
                    for (int j = 0; j < NSCR; ++j)
                        if (mi == j) sc = scr[j];
                }
                *reinterpret_cast<d2*>(&Rg[(size_t)orow * ldr]) = (d2){val0(m, i) * sc.x, val1(m, i) * sc.y};
            }
        return;
    } else {
        const int J = se.J;
        double* w5 = sStage;                                 // u1, v1, u2, v2, sF : [5][J][BC] (the stages and the table are dead)
        double* s_rc = w5 + (size_t)5 * J * BC;
        for (int i = tid; i < MT * 16 * 5; i += NT) s_rc[i] = se.rowc[(size_t)grp * MT * 16 * 5 + i];
        const int cb0 = colblk * BC;
        for (int idx = tid; idx < J * BC; idx += NT) {
            const int jc = idx / BC, c = idx - jc * BC;
            double u1 = 0, v1 = 0, u2 = 0, v2 = 0, sF = 0;
            if (cb0 + c < ldr) {
                const size_t pair = (size_t)grp * J + jc;
                const double n1 = mom_n[pair];
                const double m1 = se.scale[pair * ldr + cb0 + c], m2 = se.scale2[pair * ldr + cb0 + c];
                const double nF = (double)se.cell_len[jc];
                const double SF = se.cellS1[(size_t)jc * ldr + cb0 + c], SFF = se.cellS2[(size_t)jc * ldr + cb0 + c];
                const double n2 = nF - n1;
                const bool ok = n1 > 1.5 && n2 > 1.5;
                const double ss1 = m2 - m1 * m1 / n1;                // (bounds as in the split epilogue of k_xprod)
                const double var1 = ok ? ss1 / (n1 - 1.0) : 0.0;
                const double s2x = SF - m1, s2xx = SFF - m2;
                const double ss2 = s2xx - s2x * s2x / n2;
                const double var2 = ok ? ss2 / (n2 - 1.0) : 0.0;
                const double ssF = SFF - SF * SF / nF;
                const double varF = ssF / (nF - 1.0);
                u1 = ok ? m1 / n1 : 0.0;
                v1 = (ok && raw_ss_live(ss1, n1, m2)) ? 1.0 / sqrt(var1) : 0.0;
                u2 = ok ? s2x / n2 : 0.0;
                v2 = (ok && raw_ss_live(ss2, 2.0 * nF + 1.0, SFF)) ? 1.0 / sqrt(var2) : 0.0;
                sF = raw_ss_live(ssF, nF, SFF) ? sqrt(varF) : 0.0;
            }
            const int o = jc * BC + c;
            w5[0 * J * BC + o] = u1; w5[1 * J * BC + o] = v1; w5[2 * J * BC + o] = u2;
            w5[3 * J * BC + o] = v2; w5[4 * J * BC + o] = sF;
        }
        __syncthreads();
        if (!live) return;
        double* Rg = R + (size_t)grp * rows_per_group * ldr + col;
        const int JW = J * BC;
        // Phase A: the first halves -- they need no Rfull -- go out first, 13 stores with nothing to wait for.
        // Phase B: the second halves in batches of two tiles; a batch's eight Rfull loads (L2) are issued
        // together and waited for once (loads and stores share vmcnt, so that wait also drains the stores before
        // it: one round trip per batch, covered by the other waves of the SIMD).  Holding the whole Rfull tile
        // in registers next to the accumulators (one wait per block) cost 168 VGPRs = 3 waves per SIMD.
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (TAIL && m == MT - 1 && i > 0) break;
                const int row = m * 16 + kq + 4 * i;
                const int packed = s_out[row];
                if (packed < 0) continue;
                const int o = s_mom[row] * BC + cw;
                const double rc0 = s_rc[row * 5], rc1 = s_rc[row * 5 + 1];
                const d2 u1 = *reinterpret_cast<const d2*>(&w5[o]), v1 = *reinterpret_cast<const d2*>(&w5[JW + o]);
                const d2 r1 = (d2){(val0(m, i) - rc0 * u1.x) * rc1 * v1.x, (val1(m, i) - rc0 * u1.y) * rc1 * v1.y};
                __builtin_nontemporal_store(r1, reinterpret_cast<d2*>(&Rg[(size_t)(packed & 0xfffff) * ldr]));
            }
#pragma unroll
        for (int m0 = 0; m0 < MT; m0 += 2) {
            asm volatile("" ::: "memory");          // (keeps hipcc from hoisting this batch's loads over the stores above:
            d2 rfv[2][4];                           //  that is the all-in-registers form again)
#pragma unroll
            for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = m0 + mm;
                    if (m >= MT || (TAIL && m == MT - 1 && i > 0)) break;
                    const int packed = s_out[m * 16 + kq + 4 * i];
                    rfv[mm][i] = packed < 0 ? (d2){0.0, 0.0}
                                            : *reinterpret_cast<const d2*>(&se.Rfull[(size_t)(packed >> 20) * ldr + col]);
                }
#pragma unroll
            for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int m = m0 + mm;
                    if (m >= MT || (TAIL && m == MT - 1 && i > 0)) break;
                    const int row = m * 16 + kq + 4 * i;
                    const int packed = s_out[row];
                    if (packed < 0) continue;
                    const int o = s_mom[row] * BC + cw;
                    const double rc2 = s_rc[row * 5 + 2], rc3 = s_rc[row * 5 + 3], rc4 = s_rc[row * 5 + 4];
                    const d2 u2 = *reinterpret_cast<const d2*>(&w5[2 * JW + o]), v2 = *reinterpret_cast<const d2*>(&w5[3 * JW + o]);
                    const d2 sF = *reinterpret_cast<const d2*>(&w5[4 * JW + o]);
                    const double c10 = val0(m, i), c11 = val1(m, i);
                    const double cf0 = rfv[mm][i].x * rc4 * sF.x, cf1 = rfv[mm][i].y * rc4 * sF.y;
                    const d2 r2 = (d2){((cf0 - c10) - rc2 * u2.x) * rc3 * v2.x, ((cf1 - c11) - rc2 * u2.y) * rc3 * v2.y};
                    __builtin_nontemporal_store(r2, reinterpret_cast<d2*>(&Rg[(size_t)((packed & 0xfffff) + se.Tpp) * ldr]));
                }
        }
    }
}
