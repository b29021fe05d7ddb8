// plsx_k_multiblock.h -- multiblock PLS (PLSX_MULTIBLOCK): the per-row normalisation that makes the task block and the
// behaviour block of one stacked cross-covariance matrix commensurable.
// Included through plsx_kernels.h (which documents the operand layouts and lists the kernel headers in order).  gfx950 only.
#pragma once
#include "plsx_common.h"

// ---------------------------------------------------------------------------
// R_mb = [ rownorm(cell means - reference mean) ; rownorm(per-cell xcorr) ]: the cross-product kernel leaves both blocks
// of a resample in its R slot (rows [0, J) unscaled, rows [J, T') scaled by 1 / std where the mode asks for it), and
// every row t < T' is then divided by its L2 norm over the B features.  Columns [B, B + L) of a slot hold the score
// columns of gen_distrib: they are neither counted nor scaled.  Rows >= T' are never touched (they stay zero).
// Two launches per batch: the chunk partials of every row's sum of squares, then the scaling, which first adds the
// partials of its row in ascending chunk order.  The chunking is a function of B alone (mb_chunk_cols) and every sum has
// one fixed order -- a lane's columns in ascending order, the lanes by a butterfly of shuffles, the four waves through
// LDS in wave order, the chunks in ascending order -- so a resample's bits do not depend on the batch it came in, on the
// scratch budget or on the team.  No floating-point atomics.
// ---------------------------------------------------------------------------

// Feature columns per chunk: at least 4096 (32 KB of a row), at most 64 chunks, whole passes of a block (512 columns).
__host__ __device__ inline int mb_chunk_cols(int B)
{
    const int per = ((B + 63) / 64 + 511) / 512 * 512;
    return per > 4096 ? per : 4096;
}

// part[(r * Tp + t) * nchunk + chunk] = sum over the chunk's columns b < B of R_r[t][b]^2.  grid (nchunk, T', resamples
// of the launch), 4 waves; a row is contiguous (pitch ldr, a multiple of 128 doubles, so every 16-byte load is aligned):
// wave w takes the chunk's 128-column segments w, w + 4, .. -- one 16-byte load per lane, 1 KB per wave and instruction.
static __global__ __launch_bounds__(256)
void k_mb_rownorm(const double* __restrict__ R, long long strideR, int ldr, int Tp, int B, int chunk_cols,
                  double* __restrict__ part)
{
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = blockIdx.x, t = blockIdx.y, r = blockIdx.z, nchunk = gridDim.x;
    const double* row = R + (size_t)r * strideR + (size_t)t * ldr;
    const int c0 = chunk * chunk_cols, c1 = min(B, c0 + chunk_cols);
    double s = 0.0;
    // (b is even and ldr >= B + 1 is even: the pair (b, b + 1) lies inside the row even where b + 1 == B)
    for (int b = c0 + wave * 128 + lane * 2; b < c1; b += 512) {
        const d2 v = *reinterpret_cast<const d2*>(row + b);
        s += v.x * v.x;
        if (b + 1 < c1) s += v.y * v.y;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        part[((size_t)r * Tp + t) * nchunk + chunk] = ((red[0] + red[1]) + red[2]) + red[3];
}

// R_r[t][b] *= 1 / || R_r[t][:B] || for b < B; a row of norm 0 (or a non-finite one) is left as it is.  grid
// (ceil(B / 2048), T', resamples of the launch), 256 threads x four 16-byte loads and stores.
static __global__ __launch_bounds__(256)
void k_mb_rowscale(double* __restrict__ R, long long strideR, int ldr, int Tp, int B, int nchunk,
                   const double* __restrict__ part)
{
    __shared__ double s_inv;
    const int t = blockIdx.y, r = blockIdx.z;
    if (threadIdx.x == 0) {
        const double* p = part + ((size_t)r * Tp + t) * nchunk;
        double s = 0.0;
        for (int c = 0; c < nchunk; ++c) s += p[c];
        s_inv = (s > 0.0 && s < HUGE_VAL) ? 1.0 / sqrt(s) : 0.0;
    }
    __syncthreads();
    const double inv = s_inv;
    if (inv == 0.0) return;
    double* row = R + (size_t)r * strideR + (size_t)t * ldr;
    const int b0 = blockIdx.x * 2048 + threadIdx.x * 2;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int b = b0 + u * 512;
        if (b >= B) break;
        d2* q = reinterpret_cast<d2*>(row + b);
        d2 v = *q;
        v.x *= inv;
        if (b + 1 < B) v.y *= inv;
        *q = v;
    }
}
