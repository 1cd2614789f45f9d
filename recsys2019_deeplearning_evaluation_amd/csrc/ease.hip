// ease.hip -- the closed form of EASE_R on MI355X (gfx950): P = G^-1 in place in HBM, the weights W = P / (-diag P) and their
// column-wise top-K  [EASE_R/EASE_R_Recommender.py:40-82; DESIGN.md section 13].
//
// The inverse is a blocked Gauss-Jordan elimination WITHOUT pivoting, valid for symmetric positive-definite input only (every
// diagonal block met on the way is a Schur complement of an SPD matrix, hence SPD).  One step per block column k of NB cells:
//   ease_diag_kernel    one workgroup: D = A[k,k]^-1 by an unpivoted Gauss-Jordan sweep in float64; its pivots are the squares
//                       of the Cholesky factor's diagonal.  A pivot that is <= 0 or NaN writes the step into the status word
//   ease_panel_kernel   the panels the update overwrites go to the workspace: Ct = A[:,k]^T, R = D A[k,:], ND = -A[:,k] D
//   ease_update_kernel  the hot kernel: A[i,j] -= A[i,k] D A[k,j] = Ct^T R, an n x n x NB read-modify-write GEMM on
//                       v_mfma_f32_32x32x2_f32 (128 x 128 tiles, operands staged in LDS as score_gemm_kernel does)
//   ease_writeback_kernel  block row k <- R, block column k <- ND, the block itself <- D (replacing what the update left there)
// Every dependency is a kernel boundary on the handle's stream; a set status word turns every later kernel into an empty launch.
// Matrices that are not positive definite: ease_pivot.hip inverts them on the same handle (ease_handle.h) with pivoting, in float64.
//
// Edges: the matrix lives in an npad x npad buffer, npad = n rounded up to 128, whose tail carries an identity block.  The padded
// matrix is block diagonal, so the leading n x n cells of its inverse are G^-1 exactly and no kernel forms an address outside the
// buffer: every tile and every panel is whole.
#include "common.h"
#include "ease_handle.h"
#include "score.h"
#include "topk.cuh"

#include <algorithm>
#include <chrono>

using namespace mi355rec;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int TILE = EASE_TILE;     // cells of a side of the update kernel's tile; the matrix is padded to a multiple of it
constexpr int TK = 32;              // K chunk of the update kernel staged in LDS
constexpr int LDT = TILE + 4;       // leading dimension of its [k][row] operand tiles: rows stay 16-byte aligned
constexpr int PANEL_W = 64;         // columns (rows) of the panels one workgroup of ease_panel_kernel handles

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

namespace {        // (the handle struct: ease_handle.h)

size_t ease_bytes(int64_t n, int64_t npad, int block) {
    // the matrix, the three panels and the diagonal block, and -- where n is not a multiple of the tile -- the slab in which
    // mi355rec_sim_compute_dense_device builds its unpadded columns before it copies them to the pitch of the matrix
    return (size_t)(npad * npad + 3 * npad * block + (int64_t)block * block + (npad != n ? n * n : 0)) * sizeof(float);
}

void clear_and_pad(mi355rec_ease *h) {
    hipStream_t s = h->stream;
    if (h->npad != h->n) {
        MI_HIP(hipMemsetAsync(h->A.ptr, 0, (size_t)h->npad * h->npad * sizeof(float), s));
        hipLaunchKernelGGL(ease_pad_kernel, dim3(1), dim3(TILE), 0, s, h->A.ptr, (int64_t)h->npad, h->n, h->npad);
        MI_HIP(hipGetLastError());
    }
    h->failed_step = -1;
    h->pivot.valid = false;
}

template <int NB>
void enqueue_elimination(mi355rec_ease *h) {
    hipStream_t s = h->stream;
    const int64_t ld = h->npad;
    const size_t lds_panel = (size_t)(NB * (NB + 4) + NB * PANEL_W + PANEL_W * (NB + 4)) * sizeof(float);
    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ease_panel_kernel<NB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_panel));
    const int tiles = h->npad / TILE;
    for (int step = 0; step < h->steps; ++step) {
        const int k0 = step * NB;
        hipLaunchKernelGGL(ease_diag_kernel<NB>, dim3(1), dim3(1024), 0, s, h->A.ptr, ld, k0, step, h->status.ptr, h->D.ptr);
        hipLaunchKernelGGL(ease_panel_kernel<NB>, dim3(h->npad / PANEL_W), dim3(256), lds_panel, s, h->A.ptr, ld, k0, h->status.ptr, h->D.ptr,
                           h->R.ptr, h->Ct.ptr, h->ND.ptr);
        hipLaunchKernelGGL(ease_update_kernel<NB>, dim3(tiles, tiles), dim3(256), 0, s, h->A.ptr, ld, h->status.ptr, h->R.ptr, h->Ct.ptr);
        hipLaunchKernelGGL(ease_writeback_kernel<NB>, dim3(h->npad / PANEL_W), dim3(256), 0, s, h->A.ptr, ld, k0, h->status.ptr, h->D.ptr,
                           h->R.ptr, h->ND.ptr);
    }
    MI_HIP(hipGetLastError());
    h->launches += 4 * (int64_t)h->steps;
}

// W in place of P, once; true when this call did it
bool ensure_weights(mi355rec_ease *h) {
    MI_REQUIRE(h->state == ST_INVERTED || h->state == ST_WEIGHTS, "the weights need a successful mi355rec_ease_invert first");
    if (h->state == ST_WEIGHTS) return false;
    hipStream_t s = h->stream;
    hipLaunchKernelGGL(ease_get_diagonal_kernel, dim3(div_up(h->n, 256)), dim3(256), 0, s, h->A.ptr, (int64_t)h->npad, h->n, h->diag.ptr);
    hipLaunchKernelGGL(ease_weights_kernel, dim3(std::min(div_up(h->n, 256), 64), std::min(h->n, 65535)), dim3(256), 0, s, h->A.ptr, (int64_t)h->npad, h->n,
                       h->diag.ptr);
    MI_HIP(hipGetLastError());
    h->launches += 2;
    h->state = ST_WEIGHTS;
    return true;
}

}  // namespace

extern "C" int mi355rec_ease_create(mi355rec_ease_t *out, int32_t n_items) {
    return guarded([&] {
        MI_REQUIRE(out, "NULL argument");
        MI_REQUIRE(n_items > 0, "empty matrix (%d items)", n_items);
        *out = nullptr;
        int block = TILE;
        if (const char *v = getenv("MI355REC_EASE_BLOCK")) block = atoi(v);
        MI_REQUIRE(block == 64 || block == 128, "MI355REC_EASE_BLOCK must be 64 or 128, got %d", block);
        const int64_t npad = ((int64_t)n_items + TILE - 1) / TILE * TILE;
        MI_REQUIRE(npad <= INT32_MAX, "%d items: too many", n_items);
        ensure_device();
        size_t free_b = 0, total_b = 0;
        MI_HIP(hipMemGetInfo(&free_b, &total_b));
        const size_t need = ease_bytes(n_items, npad, block) + ((size_t)256 << 20);        // + 256 MiB for outputs and the runtime
        MI_REQUIRE(need <= free_b, "the matrix of %d items and its workspace (%.2f GB) do not fit the device's free memory (%.2f GB)", n_items,
                   need / 1e9, free_b / 1e9);
        auto h = open_handle<mi355rec_ease>(2);
        h->n = n_items; h->npad = (int)npad; h->block = block; h->steps = (int)(npad / block);
        h->A.alloc((size_t)npad * npad);
        h->D.alloc((size_t)block * block);
        h->R.alloc((size_t)block * npad);
        h->Ct.alloc((size_t)block * npad);
        h->ND.alloc((size_t)block * npad);
        h->diag.alloc((size_t)n_items);
        h->status.alloc(1);
        *out = h.release();
    });
}

extern "C" int mi355rec_ease_set_gram_from_sim(mi355rec_ease_t h, mi355rec_sim_t sim) {
    return guarded([&] {
        MI_REQUIRE(h && sim, "NULL argument");
        int n_cols = 0, topK = 0;
        sim_shape(sim, &n_cols, &topK);
        MI_REQUIRE(topK == 0, "the similarity handle must be a dense one (topK == 0), its topK is %d", topK);
        MI_REQUIRE(n_cols == h->n, "the similarity handle has %d columns, the matrix %d items", n_cols, h->n);
        ensure_device();
        ReleaseScope scope(h->stream);
        hipStream_t s = h->stream;
        const auto t0 = std::chrono::steady_clock::now();
        h->state = ST_EMPTY;
        clear_and_pad(h);
        MI_HIP(hipStreamSynchronize(s));
        // the Gram matrix is symmetric: column c of the build, contiguous, is row c of the matrix (pitch npad)
        const int rc = mi355rec_sim_compute_dense_device(sim, 0, h->n, h->A.ptr, h->npad);
        if (rc != MI355REC_OK) throw Error(rc, mi355rec_last_error());
        h->gram_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        h->state = ST_MATRIX;
    });
}

extern "C" int mi355rec_ease_set_matrix(mi355rec_ease_t h, const float *G, int64_t ld) {
    return guarded([&] {
        MI_REQUIRE(h && G, "NULL argument");
        MI_REQUIRE(ld >= h->n, "ld (%lld) < number of items (%d)", (long long)ld, h->n);
        ensure_device();
        hipStream_t s = h->stream;
        h->state = ST_EMPTY;
        clear_and_pad(h);
        MI_HIP(hipMemcpy2DAsync(h->A.ptr, (size_t)h->npad * sizeof(float), G, (size_t)ld * sizeof(float), (size_t)h->n * sizeof(float), (size_t)h->n,
                                hipMemcpyHostToDevice, s));
        MI_HIP(hipStreamSynchronize(s));
        h->state = ST_MATRIX;
    });
}

extern "C" int mi355rec_ease_get_matrix(mi355rec_ease_t h, float *G, int64_t ld) {
    return guarded([&] {
        MI_REQUIRE(h && G, "NULL argument");
        MI_REQUIRE(ld >= h->n, "ld (%lld) < number of items (%d)", (long long)ld, h->n);
        MI_REQUIRE(h->state != ST_EMPTY, "no matrix has been set");
        ensure_device();
        MI_HIP(hipMemcpy2DAsync(G, (size_t)ld * sizeof(float), h->A.ptr, (size_t)h->npad * sizeof(float), (size_t)h->n * sizeof(float), (size_t)h->n,
                                hipMemcpyDeviceToHost, h->stream));
        MI_HIP(hipStreamSynchronize(h->stream));
    });
}

extern "C" int mi355rec_ease_set_diagonal(mi355rec_ease_t h, const float *diag) {
    return guarded([&] {
        MI_REQUIRE(h && diag, "NULL argument");
        MI_REQUIRE(h->state == ST_MATRIX, "set_diagonal needs a matrix that has been set and not yet inverted");
        ensure_device();
        hipStream_t s = h->stream;
        MI_HIP(hipMemcpyAsync(h->diag.ptr, diag, (size_t)h->n * sizeof(float), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(ease_set_diagonal_kernel, dim3(div_up(h->n, 256)), dim3(256), 0, s, h->A.ptr, (int64_t)h->npad, h->n, h->diag.ptr);
        MI_HIP(hipGetLastError());
        MI_HIP(hipStreamSynchronize(s));
    });
}

extern "C" int mi355rec_ease_invert(mi355rec_ease_t h) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL argument");
        MI_REQUIRE(h->state == ST_MATRIX, "invert needs a matrix that has been set and not yet inverted");
        ensure_device();
        hipStream_t s = h->stream;
        h->state = ST_FAILED;                                   // until the status word says otherwise
        MI_HIP(hipMemsetAsync(h->status.ptr, 0xFF, sizeof(int), s));      // -1: no step has failed
        h->launches = 0;
        h->timer.start(s);
        if (h->block == 64) enqueue_elimination<64>(h);
        else enqueue_elimination<128>(h);
        h->timer.stop(s);
        int failed = -1;
        MI_HIP(hipMemcpyAsync(&failed, h->status.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
        h->invert_ms = h->timer.elapsed_ms();
        h->failed_step = failed;
        h->stats = mi355rec_stats{};
        h->stats.kernel_ms = h->stats.call_ms = h->invert_ms;
        h->stats.n_launches = h->launches;
        h->stats.n_timed = 1;
        h->stats.n_units = h->steps;
        h->stats.algorithmic_flops = 2.0 * (double)h->n * h->n * h->n;
        h->stats.algorithmic_bytes = 8.0 * (double)h->n * h->n * h->steps;      // every step reads and writes the matrix once
        if (failed >= 0)
            fail(MI355REC_E_NUMERIC, "the matrix is not positive definite: a pivot <= 0 (or NaN) in elimination step %d of %d (block size %d)",
                 failed, h->steps, h->block);
        h->state = ST_INVERTED;
    });
}

extern "C" int mi355rec_ease_get_dense(mi355rec_ease_t h, float *W, int64_t ld) {
    return guarded([&] {
        MI_REQUIRE(h && W, "NULL argument");
        MI_REQUIRE(ld >= h->n, "ld (%lld) < number of items (%d)", (long long)ld, h->n);
        ensure_device();
        hipStream_t s = h->stream;
        h->call_timer.start(s);
        const bool scaled = ensure_weights(h);
        h->call_timer.stop(s);
        MI_HIP(hipMemcpy2DAsync(W, (size_t)ld * sizeof(float), h->A.ptr, (size_t)h->npad * sizeof(float), (size_t)h->n * sizeof(float), (size_t)h->n,
                                hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
        if (scaled) h->topk_ms = h->call_timer.elapsed_ms();
    });
}

// what the dense scorer (densescore.hip) copies its weights from, device to device: the cells mi355rec_ease_get_dense downloads
void mi355rec::ease_weights_device(mi355rec_ease *h, const float **W, int64_t *ld, int *n) {
    hipStream_t s = h->stream;
    h->call_timer.start(s);
    const bool scaled = ensure_weights(h);
    h->call_timer.stop(s);
    MI_HIP(hipStreamSynchronize(s));
    if (scaled) h->topk_ms = h->call_timer.elapsed_ms();
    *W = h->A.ptr;
    *ld = h->npad;
    *n = h->n;
}

extern "C" int mi355rec_ease_get_topk(mi355rec_ease_t h, int32_t topK, int32_t *idx, float *val) {
    return guarded([&] {
        MI_REQUIRE(h && idx && val, "NULL argument");
        MI_REQUIRE(topK >= 1, "topK must be at least 1, got %d", topK);
        MI_REQUIRE(h->state == ST_INVERTED || h->state == ST_WEIGHTS, "the weights need a successful mi355rec_ease_invert first");
        if (topK > MAX_TOPK || !score_row_fits_lds(h->n, topK))
            fail(MI355REC_E_UNSUPPORTED, "top-%d of columns of %d cells is beyond the in-LDS selection (at most %d of about 30 000 cells)", topK, h->n,
                 MAX_TOPK);
        ensure_device();
        ReleaseScope scope(h->stream);
        hipStream_t s = h->stream;
        const size_t cells = (size_t)h->n * topK;
        if (h->out_idx.count < cells) {
            h->out_idx.alloc(cells);
            h->out_val.alloc(cells);
        }
        h->call_timer.start(s);
        ensure_weights(h);
        const int n_pad = (h->n + 3) & ~3;
        const size_t lds = (size_t)n_pad * 4 + (size_t)AUX_WORDS * 4;
        auto k = ease_topk_kernel<1024>;
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, dim3(h->n), dim3(1024), lds, s, h->A.ptr, (int64_t)h->npad, h->n, n_pad, topK, h->out_idx.ptr, h->out_val.ptr);
        MI_HIP(hipGetLastError());
        h->launches += 1;
        h->call_timer.stop(s);
        h->out_idx.download(idx, cells, s);
        h->out_val.download(val, cells, s);
        MI_HIP(hipStreamSynchronize(s));
        h->topk_ms = h->call_timer.elapsed_ms();
    });
}

extern "C" int mi355rec_ease_fit_info(mi355rec_ease_t h, int32_t *block, int32_t *steps, int32_t *failed_step, double *invert_ms, double *gram_ms,
                                      double *topk_ms, int64_t *launches) {
    return guarded([&] {
        MI_REQUIRE(h && block && steps && failed_step && invert_ms && gram_ms && topk_ms && launches, "NULL argument");
        *block = h->block;
        *steps = h->steps;
        *failed_step = h->failed_step;
        *invert_ms = h->invert_ms;
        *gram_ms = h->gram_ms;
        *topk_ms = h->topk_ms;
        *launches = h->launches;
    });
}

extern "C" int mi355rec_ease_get_stats(mi355rec_ease_t h, mi355rec_stats *stats) { return handle_get_stats(h, stats); }

extern "C" void mi355rec_ease_destroy(mi355rec_ease_t h) { handle_destroy(h); }
