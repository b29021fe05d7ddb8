// plsx_k_contrast.h -- non-rotated PLS (plsx_set_contrasts): the kernels that stand where the Gram pass and the small
// solver stand while contrasts are set.
// Included through plsx_kernels.h (which documents the operand layouts and lists the kernel headers in order).  gfx950 only.
#pragma once
#include "plsx_common.h"
#include "plsx_k_small.h"

// ---------------------------------------------------------------------------
// With the caller's contrasts V (T' x L, unit columns, zero columns past Lc) nothing is decomposed: a resample's
// statistic is s_l = || R_r^T v_l ||, and its weights are U_r = R_r^T V -- the rotation kernel's product with the
// SAME operand for every resample.  V is kept once per binding in the fragment order k_small writes M in
// ([chunk of PLSX_LT_CHUNK tiles][k-step][tile][lane], mfrag_decode), so that k_urot, k_build_W and k_build_Vd
// consume it unchanged.
// ---------------------------------------------------------------------------

// Doubles before the fragments of tile `lt` at k-step 0, and the tiles of its chunk (the k-step pitch is 64 x that).
__device__ __forceinline__ size_t cfrag_tile_base(int lt, int nks_t, int LT, int& ltc)
{
    const int chunk = lt / PLSX_LT_CHUNK;
    ltc = min(PLSX_LT_CHUNK, LT - chunk * PLSX_LT_CHUNK);
    return mfrag_chunk_base(chunk, nks_t) + (size_t)(lt - chunk * PLSX_LT_CHUNK) * 64;
}

// C (T' x Lc row-major, unit columns) -> dense (T' x L, zero padded) and the fragment-ordered operand.
static __global__ void k_contrast_pack(const double* __restrict__ C, int n, int Lc, int L, int nks_t, int LT,
                                       double* __restrict__ dense, double* __restrict__ frag)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n * L) {
        const int t = idx / L, l = idx - t * L;
        dense[idx] = l < Lc ? C[(size_t)t * Lc + l] : 0.0;
    }
    if (idx < nks_t * LT * 64) {
        int lane, lt, ks;
        mfrag_decode(idx, nks_t, LT, ks, lt, lane);
        const int t = ks * 4 + (lane >> 4), l = lt * 16 + (lane & 15);
        frag[idx] = (t < n && l < Lc) ? C[(size_t)t * Lc + l] : 0.0;
    }
}

// The operand of every resample of a batch: Mfrag[r] = V (stands where k_small writes M_r).
static __global__ void k_contrast_fill(const double* __restrict__ frag, int tot, double* __restrict__ Mfrag)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < tot) Mfrag[(size_t)blockIdx.y * tot + idx] = frag[idx];
}

// s_l^2 of one chunk of feature columns: partial[r][chunk][l] = sum over the chunk's columns b < B of (R_r^T V)[b][l]^2
// for the LTC tiles of L from lt0 on.  grid (nchunk, nres), 4 waves; wave w takes the chunk's 16-column tiles
// w, w + 4, ..: per tile the (16 x 16 LTC) product accumulates over the T'pp / 4 k-steps on v_mfma_f64_16x16x4_f64
// (A = the R fragment, one 8-byte load per lane and k-step, rows contiguous over the lanes; B = the V fragment from LDS),
// is squared and added to LTC running sums per lane.  The four row groups of a wave (shuffles), then the four
// waves (LDS, wave order) are added in one fixed order: the chunking is a function of B alone, so a resample's bits do
// not depend on the batch it came in.  Columns [B, B + L) of R hold the score columns of gen_distrib and do not count.
// VLDS = false: V too large for LDS (T' L beyond 8192 doubles per LTC tiles), fragments from L2.
template <int LTC, bool VLDS>
__global__ __launch_bounds__(256)
void k_contrast_norms(const double* __restrict__ R, long long strideR, int ldr, int nks_t,
                      const double* __restrict__ frag, int LT, int lt0, int B, int tiles_per_chunk, int L,
                      double* __restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) double sm_c[];
    __shared__ double red[4][LTC][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = blockIdx.x, r = blockIdx.y, nchunk = gridDim.x;
    size_t vbase[LTC];
    int vpitch[LTC];
#pragma unroll
    for (int j = 0; j < LTC; ++j) {
        int ltc;
        vbase[j] = cfrag_tile_base(lt0 + j, nks_t, LT, ltc);
        vpitch[j] = ltc * 64;
    }
    if (VLDS) {
        // [k-step][tile of this launch][lane]
        for (int i = threadIdx.x; i < nks_t * LTC * 64; i += blockDim.x) {
            const int ks = i / (LTC * 64), rem = i - ks * LTC * 64, j = rem >> 6;
            sm_c[i] = frag[vbase[j] + (size_t)ks * vpitch[j] + (rem & 63)];
        }
        __syncthreads();
    }
    auto vfrag = [&](int ks, int j) -> double {
        return VLDS ? sm_c[(ks * LTC + j) * 64 + lane] : frag[vbase[j] + (size_t)ks * vpitch[j] + lane];
    };
    const int ntiles = (B + 15) / 16;
    const int t_end = min(ntiles, (chunk + 1) * tiles_per_chunk);
    const double* Rr = R + (size_t)r * strideR + (size_t)(lane >> 4) * ldr + (lane & 15);
    const size_t kstep = (size_t)4 * ldr;
    double s[LTC];
#pragma unroll
    for (int j = 0; j < LTC; ++j) s[j] = 0.0;
    for (int tile = chunk * tiles_per_chunk + wave; tile < t_end; tile += 4) {
        const int b0 = tile * 16;
        const double* Rp = Rr + b0;
        d4 acc[LTC];
#pragma unroll
        for (int j = 0; j < LTC; ++j) acc[j] = (d4){0, 0, 0, 0};
        int ks = 0;
        for (; ks + 4 <= nks_t; ks += 4) {
            double a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = Rp[(size_t)(ks + u) * kstep];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < LTC; ++j) acc[j] = mfma_f64(a[u], vfrag(ks + u, j), acc[j]);
        }
        for (; ks < nks_t; ++ks) {
            const double a = Rp[(size_t)ks * kstep];
#pragma unroll
            for (int j = 0; j < LTC; ++j) acc[j] = mfma_f64(a, vfrag(ks, j), acc[j]);
        }
        // D: lane, register i = feature b0 + (lane >> 4) + 4 i, column 16 (lt0 + j) + (lane & 15)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = b0 + (lane >> 4) + 4 * i < B;
#pragma unroll
            for (int j = 0; j < LTC; ++j) {
                const double v = in ? acc[j][i] : 0.0;
                s[j] += v * v;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < LTC; ++j) {
        double v = s[j];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (lane < 16) red[wave][j][lane] = v;
    }
    __syncthreads();
    if (threadIdx.x < LTC * 16) {
        const int j = threadIdx.x >> 4, c = threadIdx.x & 15, l = (lt0 + j) * 16 + c;
        if (l < L)
            partial[((size_t)r * nchunk + chunk) * L + l] = ((red[0][j][c] + red[1][j][c]) + red[2][j][c]) + red[3][j][c];
    }
}

// out[r][l] = sqrt(sum of the chunks in ascending order) for l < Lc, 0 for the padding columns.
static __global__ void k_contrast_finish(const double* __restrict__ partial, int nchunk, int nres, int L, int Lc,
                                         double* __restrict__ out)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)nres * L) return;
    const int r = (int)(idx / L), l = (int)(idx - (long long)r * L);
    double s = 0.0;
    if (l < Lc)
        for (int c = 0; c < nchunk; ++c) s += partial[((size_t)r * nchunk + c) * L + l];
    out[idx] = sqrt(s);
}

// Projected permutations: out[r][l] = sqrt(sum over the column blocks, ascending, of the row-norm partials the fixed-X
// blocks left (k_xprod EPI 10: part[column block][group][rows], resample r = group * n + rr in rows rr * T' ..)).  The
// column blocks follow B alone and every partial is the work of one block: the bits of a resample do not depend on the
// batch, on its place in it or on the scratch budget.
static __global__ void k_rownorm_finish(const double* __restrict__ part, int ncolblk, int groups, int rows, int n, int Tp,
                                        int nres, double* __restrict__ out)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)nres * Tp) return;
    const int r = (int)(idx / Tp), l = (int)(idx - (long long)r * Tp);
    const double* p = part + (size_t)(r / n) * rows + (r % n) * Tp + l;
    const size_t step = (size_t)groups * rows;
    double s = 0.0;
    int c = 0;
    for (; c + 8 <= ncolblk; c += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(c + u) * step];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; c < ncolblk; ++c) s += p[(size_t)c * step];
    out[idx] = sqrt(s);
}

// Dual-space permutations: s_l^2 = v_l^T G_p v_l (clamped at 0) from the Gram matrix perm_dual forms.  One block per
// permutation; thread l walks the rows of G (the same address over the block: one broadcast fetch) against column l
// of the dense V (consecutive over the threads).
static __global__ void k_contrast_quad(const double* __restrict__ G, int n, const double* __restrict__ V, int L, int Lc,
                                       double* __restrict__ out)
{
    const double* Gr = G + (size_t)blockIdx.x * n * n;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        double q = 0.0;
        if (l < Lc)
            for (int i = 0; i < n; ++i) {
                double t = 0.0;
                for (int j = 0; j < n; ++j) t += Gr[(size_t)i * n + j] * V[(size_t)j * L + l];
                q += V[(size_t)i * L + l] * t;
            }
        out[(size_t)blockIdx.x * L + l] = sqrt(fmax(q, 0.0));
    }
}

// x_weights = Z / s per column (0 where the norm is 0), in place on Z (B x L).
static __global__ void k_contrast_scale(double* __restrict__ Z, long long count, int L, const double* __restrict__ sv)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= count) return;
    const double s = sv[idx % L];
    Z[idx] = s > 0.0 ? Z[idx] / s : 0.0;
}
