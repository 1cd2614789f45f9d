// ease_kernels.cuh -- the device code of ease.hip: the four kernels of a step of the unpivoted float32 elimination (diag, panel,
// update, write-back), the pad / diagonal / weights kernels and the column-wise top-K.  What each step does and why no kernel forms
// an address outside the padded buffer: the head of ease.hip.  The constants shared with the host (EASE_TILE, TK, PANEL_W): ease_plan.h.
// Included by ease.hip only.
#pragma once

#include "common.h"
#include "ease_plan.h"
#include "topk.cuh"

using namespace mi355rec;
using namespace mi355rec::ease;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int TILE = EASE_TILE;     // cells of a side of the update kernel's tile
constexpr int LDT = TILE + 4;       // leading dimension of its [k][row] operand tiles: rows stay 16-byte aligned

// D = A[k0 .. k0 + NB, k0 .. k0 + NB]^-1 in float64, by Gauss-Jordan without pivoting.  The block lives in registers, a P x P patch
// per thread (32 x 32 threads); sweep j needs the old column j and row j of the block, which their owners publish in LDS -- two
// buffers taken in turn, so one barrier per sweep is enough (nobody can write a buffer for sweep j + 2 before everybody has passed
// the barrier of sweep j + 1, i.e. has finished reading it for sweep j).
template <int NB>
__global__ __launch_bounds__(1024) void ease_diag_kernel(const float *A, int64_t ld, int k0, int step, int *status, float *D) {
    constexpr int P = NB / 32;
    __shared__ double col[2][NB], row[2][NB];
    if (*status >= 0) return;
    const int tid = threadIdx.x, i0 = (tid >> 5) * P, c0 = (tid & 31) * P;
    double a[P][P];
#pragma unroll
    for (int x = 0; x < P; ++x)
#pragma unroll
        for (int y = 0; y < P; ++y) a[x][y] = (double)A[(int64_t)(k0 + i0 + x) * ld + k0 + c0 + y];
    for (int j = 0; j < NB; ++j) {
        double *cj = col[j & 1], *rj = row[j & 1];
#pragma unroll
        for (int x = 0; x < P; ++x)
#pragma unroll
            for (int y = 0; y < P; ++y) {
                if (c0 + y == j) cj[i0 + x] = a[x][y];
                if (i0 + x == j) rj[c0 + y] = a[x][y];
            }
        __syncthreads();
        const double p = rj[j];
        if (!(p > 0.0)) {            // not positive definite (or NaN): the same value in every thread
            if (tid == 0) *status = step;
            return;
        }
        const double inv = 1.0 / p;
        double cv[P], rv[P];
#pragma unroll
        for (int x = 0; x < P; ++x) cv[x] = cj[i0 + x];
#pragma unroll
        for (int y = 0; y < P; ++y) rv[y] = rj[c0 + y] * inv;
#pragma unroll
        for (int x = 0; x < P; ++x)
#pragma unroll
            for (int y = 0; y < P; ++y) {
                const bool in_row = i0 + x == j, in_col = c0 + y == j;
                a[x][y] = in_row ? (in_col ? inv : rv[y]) : (in_col ? -cv[x] * inv : a[x][y] - cv[x] * rv[y]);
            }
    }
#pragma unroll
    for (int x = 0; x < P; ++x)
#pragma unroll
        for (int y = 0; y < P; ++y) D[(i0 + x) * NB + c0 + y] = (float)a[x][y];
}

// The panels of step k for the 64 columns (and the 64 rows) t0 .. t0 + 63:
//   R[m][t0 + c]  = sum_q D[m][q] A[k0 + q][t0 + c]         the scaled row panel        [NB][ld]
//   Ct[m][t0 + r] = A[t0 + r][k0 + m]                        the column panel, k-major   [NB][ld]
//   ND[t0 + r][m] = -sum_q A[t0 + r][k0 + q] D[q][m]         what the column panel becomes [ld][NB]
template <int NB>
__global__ __launch_bounds__(256) void ease_panel_kernel(const float *A, int64_t ld, int k0, const int *status, const float *D, float *R, float *Ct,
                                                         float *ND) {
    extern __shared__ __attribute__((aligned(16))) float lds32[];
    constexpr int SD = NB + 4;
    float *Ds = lds32, *Xs = Ds + NB * SD, *Ys = Xs + NB * PANEL_W;       // Ds[NB][SD], Xs[NB][64], Ys[64][SD]
    if (*status >= 0) return;
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * PANEL_W;
    for (int e = tid; e < NB * NB; e += 256) Ds[(e / NB) * SD + e % NB] = D[e];
    for (int e = tid; e < NB * PANEL_W; e += 256) {
        const int m = e / PANEL_W, c = e % PANEL_W;
        Xs[e] = A[(int64_t)(k0 + m) * ld + t0 + c];
    }
    for (int e = tid; e < PANEL_W * NB; e += 256) {
        const int r = e / NB, m = e % NB;
        Ys[r * SD + m] = A[(t0 + r) * ld + k0 + m];
    }
    __syncthreads();
    constexpr int PER = NB / 4;     // outputs of a thread in each product
    {   // R: a wavefront shares the rows of D (LDS broadcasts), its lanes run along the columns
        const int c = tid & 63, m0 = (tid >> 6) * PER;
        float acc[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) acc[u] = 0.f;
        for (int q = 0; q < NB; q += 4) {
            const float x0 = Xs[q * PANEL_W + c], x1 = Xs[(q + 1) * PANEL_W + c], x2 = Xs[(q + 2) * PANEL_W + c], x3 = Xs[(q + 3) * PANEL_W + c];
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const float4 d = *reinterpret_cast<const float4 *>(&Ds[(m0 + u) * SD + q]);
                acc[u] = fmaf(d.w, x3, fmaf(d.z, x2, fmaf(d.y, x1, fmaf(d.x, x0, acc[u]))));
            }
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) R[(int64_t)(m0 + u) * ld + t0 + c] = acc[u];
    }
    {   // ND: a wavefront shares the rows of the column panel, its lanes run along the columns of D
        constexpr int GROUPS = 256 / NB;
        const int m = tid % NB, r0 = (tid / NB) * (PANEL_W / GROUPS);
        static_assert(PANEL_W / GROUPS == PER, "rows per thread");
        float acc[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) acc[u] = 0.f;
        for (int q = 0; q < NB; q += 4) {
            const float d0 = Ds[q * SD + m], d1 = Ds[(q + 1) * SD + m], d2 = Ds[(q + 2) * SD + m], d3 = Ds[(q + 3) * SD + m];
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const float4 y = *reinterpret_cast<const float4 *>(&Ys[(r0 + u) * SD + q]);
                acc[u] = fmaf(y.w, d3, fmaf(y.z, d2, fmaf(y.y, d1, fmaf(y.x, d0, acc[u]))));
            }
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) ND[(t0 + r0 + u) * NB + m] = -acc[u];
    }
    for (int e = tid; e < NB * PANEL_W; e += 256) {
        const int m = e / PANEL_W, r = e % PANEL_W;
        Ct[(int64_t)m * ld + t0 + r] = Ys[r * SD + m];
    }
}

// A[r][c] -= sum_m Ct[m][r] R[m][c] on one 128 x 128 tile: 2 x 2 wavefronts, four 32 x 32 accumulators each, the next K chunk's
// 16-byte loads in flight during the MFMAs of the current one.  Every tile is treated alike: what lands in block row k and block
// column k is replaced by ease_writeback_kernel.
template <int NB>
__global__ __launch_bounds__(256) void ease_update_kernel(float *A, int64_t ld, const int *status, const float *R, const float *Ct) {
    __shared__ __attribute__((aligned(16))) float As[TK][LDT];         // [m][row of the tile]
    __shared__ __attribute__((aligned(16))) float Bs[TK][LDT];         // [m][column of the tile]
    if (*status >= 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t row0 = (int64_t)blockIdx.y * TILE, col0 = (int64_t)blockIdx.x * TILE;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    // staging: thread t moves quads e = t + 256 i (i < 4) of both operands: m = e / 32, cells 4 (e % 32) .. + 3
    const float *ap = Ct + row0 + (tid & 31) * 4, *bp = R + col0 + (tid & 31) * 4;
    const int mq = tid >> 5;
    f32x4 ra[4], rb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ra[i] = *reinterpret_cast<const f32x4 *>(ap + (int64_t)(mq + 8 * i) * ld);
        rb[i] = *reinterpret_cast<const f32x4 *>(bp + (int64_t)(mq + 8 * i) * ld);
    }
    for (int m0 = 0; m0 < NB; m0 += TK) {
        __syncthreads();                   // everybody has finished multiplying the previous chunk
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<f32x4 *>(&As[mq + 8 * i][(tid & 31) * 4]) = ra[i];
            *reinterpret_cast<f32x4 *>(&Bs[mq + 8 * i][(tid & 31) * 4]) = rb[i];
        }
        __syncthreads();
        if (m0 + TK < NB) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ra[i] = *reinterpret_cast<const f32x4 *>(ap + (int64_t)(m0 + TK + mq + 8 * i) * ld);
                rb[i] = *reinterpret_cast<const f32x4 *>(bp + (int64_t)(m0 + TK + mq + 8 * i) * ld);
            }
        }
        // A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]   (32x32x2 f32 operand maps)
        const float *a_col = &As[lane >> 5][wm * 64 + (lane & 31)];
        const float *b_col = &Bs[lane >> 5][wn * 64 + (lane & 31)];
#pragma unroll 4
        for (int s = 0; s < TK; s += 2) {
            const float a0 = a_col[s * LDT], a1 = a_col[s * LDT + 32];
            const float b0 = b_col[s * LDT], b1 = b_col[s * LDT + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // C/D map: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); the row and column offsets below are the same in every lane
    float *cell = A + (row0 + wm * 64 + 4 * (lane >> 5)) * ld + col0 + wn * 64 + (lane & 31);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            float *at = cell + (int64_t)(a * 32 + (reg & 3) + 8 * (reg >> 2)) * ld;
            at[0] -= acc[a][0][reg];
            at[32] -= acc[a][1][reg];
        }
    }
}

// What step k leaves in its own block row and block column (whatever the update has written there is replaced):
// A[k,:] = R, A[:,k] = ND, A[k,k] = D, for the 64 columns (rows) t0 .. t0 + 63.
template <int NB>
__global__ __launch_bounds__(256) void ease_writeback_kernel(float *A, int64_t ld, int k0, const int *status, const float *D, const float *R,
                                                             const float *ND) {
    if (*status >= 0) return;
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * PANEL_W;
    for (int e = tid; e < NB * PANEL_W; e += 256) {
        const int m = e / PANEL_W;
        const int64_t c = t0 + e % PANEL_W;
        const bool in_k = c >= k0 && c < k0 + NB;
        A[(int64_t)(k0 + m) * ld + c] = in_k ? D[m * NB + (c - k0)] : R[(int64_t)m * ld + c];
    }
    for (int e = tid; e < PANEL_W * NB; e += 256) {
        const int64_t r = t0 + e / NB;
        const int m = e % NB;
        if (!(r >= k0 && r < k0 + NB)) A[r * ld + k0 + m] = ND[r * NB + m];
    }
}

// the identity tail of the padded matrix (cells [n, npad) of the diagonal; the rest of the padding is zero)
__global__ void ease_pad_kernel(float *A, int64_t ld, int n, int npad) {
    const int i = n + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npad) A[(int64_t)i * ld + i] = 1.f;
}

__global__ void ease_set_diagonal_kernel(float *A, int64_t ld, int n, const float *diag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) A[(int64_t)i * ld + i] = diag[i];
}

__global__ void ease_get_diagonal_kernel(const float *A, int64_t ld, int n, float *diag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) diag[i] = A[(int64_t)i * ld + i];
}

// W[i][j] = P[i][j] / -P[j][j], 0 on the diagonal, in place: column j of W is column j of P
__global__ __launch_bounds__(256) void ease_weights_kernel(float *A, int64_t ld, int n, const float *diag) {
    for (int i = blockIdx.y; i < n; i += gridDim.y)
        for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
            float *cell = A + (int64_t)i * ld + j;
            *cell = i == j ? 0.f : *cell / -diag[j];
        }
}

// similarityMatrixTopK on a dense array (Base/Recommender_utils.py:55): per column the topK largest non-zero cells by value
template <int THREADS>
__global__ __launch_bounds__(THREADS) void ease_topk_kernel(const float *W, int64_t ld, int n, int n_pad, int topK, int *out_idx, float *out_val) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *acc = smem;
    uint32_t *aux = reinterpret_cast<uint32_t *>(smem + n_pad);
    __shared__ SelectScratch sc;
    __shared__ uint32_t s_npos, s_nneg, s_ncand;
    const int tid = threadIdx.x, lane = tid & 63;
    const int j = blockIdx.x;
    if (tid == 0) { s_npos = 0; s_nneg = 0; s_ncand = 0; }
    __syncthreads();
    uint32_t npos = 0, nneg = 0;
    for (int i = tid; i < n_pad; i += THREADS) {
        const float v = i < n ? W[(int64_t)i * ld + j] : 0.f;
        acc[i] = v;
        npos += v > 0.f;
        nneg += v < 0.f;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        npos += __shfl_down(npos, off);
        nneg += __shfl_down(nneg, off);
    }
    if (lane == 0) {
        if (npos) atomicAdd(&s_npos, npos);
        if (nneg) atomicAdd(&s_nneg, nneg);
    }
    __syncthreads();
    block_topk_emit<THREADS>(acc, n, topK, s_npos, s_nneg, TOPK_NONZERO, aux, sc, &s_ncand, out_idx + (int64_t)j * topK,
                             out_val + (int64_t)j * topK);
}

}  // namespace
