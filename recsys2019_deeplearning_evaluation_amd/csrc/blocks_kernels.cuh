// blocks_kernels.cuh -- the kernels under both block-pair handles (PureSVD, NMF), kernels only; launched by blocks.hip  [DESIGN.md section 11].
//
//   svd_spmm_kernel     Y[row] = sum_j val[j] * X[idx[j]]: a row is cut into PIECES of at most SPLIT nonzeros, one piece per group of
//                       16 / 32 / 64 lanes (chosen from r, so that short blocks pack 4 or 2 pieces into a wavefront); a lane owns up to
//                       CPL columns lp apart per pass over the piece and sums them in nonzero order.  One-piece rows write Y
//                       directly, pieces of longer rows write a partial row that svd_long_rows_kernel adds in piece order: no
//                       atomics, a product is bitwise repeatable.  All-ones URMs skip the value stream.
//   svd_gram_kernel     G = X^T X in float64 FMAs: 64 x 64 tiles of the upper triangle, a slab of rows per workgroup, the slabs'
//                       partial tiles added in slab order by svd_gram_reduce_kernel (which mirrors the lower triangle).
//   svd_iota_kernel     out[i] = i: the identity row gather of score.hip's GEMM.
// The constants the host shares with them (SPLIT, SPMM_THREADS, GT, GR) and every grid are in blocks_plan.h.
#pragma once

#include <hip/hip_runtime.h>

#include "blocks_plan.h"

namespace {

using namespace mi355rec::blocks;

constexpr int CPL = 4;            // columns a lane owns per pass over its piece

template <bool ONES>
__global__ __launch_bounds__(SPMM_THREADS) void svd_spmm_kernel(const int *__restrict__ p_row, const int *__restrict__ p_begin,
                                                                const int *__restrict__ p_end, const int *__restrict__ p_slot,
                                                                int n_pieces, const int *__restrict__ idx,
                                                                const float *__restrict__ val, const float *__restrict__ X, int r,
                                                                int lp_shift, float *__restrict__ Y, float *__restrict__ partial) {
    const int lp = 1 << lp_shift;
    const int gtid = blockIdx.x * SPMM_THREADS + threadIdx.x;
    const int piece = gtid >> lp_shift, sub = gtid & (lp - 1);
    if (piece >= n_pieces) return;
    const int b = p_begin[piece], e = p_end[piece], slot = p_slot[piece];
    float *out = slot < 0 ? Y + (size_t)p_row[piece] * r : partial + (size_t)slot * r;
    for (int c0 = sub; c0 < r; c0 += lp * CPL) {
        int nq = 0;                                   // columns of this lane in this pass: c0 + q * lp < r
#pragma unroll
        for (int q = 0; q < CPL; ++q) nq += (c0 + q * lp < r) ? 1 : 0;
        float acc[CPL];
#pragma unroll
        for (int q = 0; q < CPL; ++q) acc[q] = 0.f;
        int j = b;
        // (loading the indices of the next four nonzeros ahead of the rows of the current four was measured and is slower: 1.22 against
        // 1.05 ms per pass at the ML-20M shape, r = 60)
        for (; j + 4 <= e; j += 4) {
            const float *x0 = X + (size_t)idx[j] * r + c0, *x1 = X + (size_t)idx[j + 1] * r + c0;
            const float *x2 = X + (size_t)idx[j + 2] * r + c0, *x3 = X + (size_t)idx[j + 3] * r + c0;
            float v0 = 1.f, v1 = 1.f, v2 = 1.f, v3 = 1.f;
            if (!ONES) { v0 = val[j]; v1 = val[j + 1]; v2 = val[j + 2]; v3 = val[j + 3]; }
            float g[4][CPL];
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const bool in = q < nq;
                g[0][q] = in ? x0[q * lp] : 0.f;
                g[1][q] = in ? x1[q * lp] : 0.f;
                g[2][q] = in ? x2[q * lp] : 0.f;
                g[3][q] = in ? x3[q * lp] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                if (ONES) {
                    acc[q] = (((acc[q] + g[0][q]) + g[1][q]) + g[2][q]) + g[3][q];
                } else {
                    acc[q] = fmaf(v0, g[0][q], acc[q]);
                    acc[q] = fmaf(v1, g[1][q], acc[q]);
                    acc[q] = fmaf(v2, g[2][q], acc[q]);
                    acc[q] = fmaf(v3, g[3][q], acc[q]);
                }
            }
        }
        for (; j < e; ++j) {
            const float *x0 = X + (size_t)idx[j] * r + c0;
            const float v0 = ONES ? 1.f : val[j];
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const float g = q < nq ? x0[q * lp] : 0.f;
                acc[q] = ONES ? acc[q] + g : fmaf(v0, g, acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < CPL; ++q)
            if (q < nq) out[c0 + q * lp] = acc[q];
    }
}

// Y[row] = partial[first] + partial[first + 1] + ... (the pieces of a long row, in piece order)
__global__ __launch_bounds__(256) void svd_long_rows_kernel(const int *__restrict__ l_row, const int *__restrict__ l_first,
                                                            const int *__restrict__ l_count, const float *__restrict__ partial, int r,
                                                            float *__restrict__ Y) {
    const int row = l_row[blockIdx.x], first = l_first[blockIdx.x], count = l_count[blockIdx.x];
    for (int c = threadIdx.x; c < r; c += 256) {
        float s = partial[(size_t)first * r + c];
        for (int k = 1; k < count; ++k) s += partial[(size_t)(first + k) * r + c];
        Y[(size_t)row * r + c] = s;
    }
}

// part[slab][i][j] = sum over the slab's rows of X[row][i] * X[row][j] for the tiles (ti <= tj) of the upper triangle
__global__ __launch_bounds__(256) void svd_gram_kernel(const float *__restrict__ X, int n, int r, int rows_per_slab,
                                                       double *__restrict__ part) {
    const int ti = blockIdx.x, tj = blockIdx.y, slab = blockIdx.z;
    if (tj < ti) return;
    __shared__ float As[GR][GT], Bs[GR][GT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    const int r0 = slab * rows_per_slab, r1 = min(n, r0 + rows_per_slab);
    for (int base = r0; base < r1; base += GR) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < GR * GT / 256; ++i) {
            const int e = tid + 256 * i, k = e >> 6, c = e & 63, row = base + k;
            const float *x = X + (size_t)row * r;
            As[k][c] = (row < r1 && ti * GT + c < r) ? x[ti * GT + c] : 0.f;
            Bs[k][c] = (row < r1 && tj * GT + c < r) ? x[tj * GT + c] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < GR; ++k) {
            const float4 a4 = *reinterpret_cast<const float4 *>(&As[k][ty * 4]);
            const float4 b4 = *reinterpret_cast<const float4 *>(&Bs[k][tx * 4]);
            const double a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fma(a[p], b[q], acc[p][q]);
        }
    }
    double *out = part + (size_t)slab * r * r;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = ti * GT + ty * 4 + p, j = tj * GT + tx * 4 + q;
            if (i < r && j < r) out[(size_t)i * r + j] = acc[p][q];
        }
}

__global__ __launch_bounds__(256) void svd_gram_reduce_kernel(const double *__restrict__ part, int n_slabs, int r, double *__restrict__ G) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= r * r) return;
    const int i = e / r, j = e % r;
    // tiles below the diagonal were not computed: (i, j) is read from the tile of (min, max)
    const int lo = (i / GT <= j / GT) ? i : j, hi = (i / GT <= j / GT) ? j : i;
    double s = 0.0;
    for (int k = 0; k < n_slabs; ++k) s += part[(size_t)k * r * r + (size_t)lo * r + hi];
    G[e] = s;
}

__global__ __launch_bounds__(256) void svd_iota_kernel(int *out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = i;
}

}  // namespace
