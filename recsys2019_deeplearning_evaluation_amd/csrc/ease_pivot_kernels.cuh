// ease_pivot_kernels.cuh -- the device code of ease_pivot.hip: the pivot search on a scratch copy of the panel (load, pick, elim),
// the row swaps, the block step in float64 (diag, transpose, the GEMM kernel in its three modes, write-back) and the kernels that widen
// the matrix on the way in and gather it on the way out.  What a step does: the head of ease_pivot.hip.  The constants shared with
// the host (CHUNK, GK, PANEL_W): ease_plan.h.  Included by ease_pivot.hip only.
#pragma once

#include "common.h"
#include "ease_plan.h"

#include <climits>
#include <cmath>

using namespace mi355rec;
using namespace mi355rec::ease;

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// ---- pivot search ------------------------------------------------------------------------------------------------------------
// candidate (v, pos): v = |value|, -1 for "none".  A NaN beats everything, an infinity included (the pivot is then refused at this
// column, as the restatement in tests/ease_pivoted_cases.py refuses it); otherwise the larger v wins; ties go to the lower row.
__device__ __forceinline__ bool cand_beats(double va, int pa, double vb, int pb) {
    const bool na = va != va, nb = vb != vb;
    if (na != nb) return na;
    if (na) return pa < pb;
    return va > vb || (va == vb && pa < pb);
}

__device__ __forceinline__ void wave_best(double &v, int &pos) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(v, off);
        const int op = __shfl_down(pos, off);
        if (cand_beats(ov, op, v, pos)) { v = ov; pos = op; }
    }
}

// the first wavefront of a workgroup: the best of rows max(row0, lo) .. min(row0 + 63, n - 1) in column `col` of the scratch panel
template <int NB>
__device__ __forceinline__ void chunk_candidate(const double *P, int row0, int lo, int n, int col, int chunk, double *part_val, int *part_pos) {
    const int row = row0 + (int)threadIdx.x;
    double v = -1.0;
    int pos = INT_MAX;
    if (row >= lo && row < n) {
        v = fabs(P[(int64_t)row * NB + col]);
        pos = row;
    }
    wave_best(v, pos);
    if (threadIdx.x == 0) { part_val[chunk] = v; part_pos[chunk] = pos; }
}

// P[row][c] = A[row][k0 + c] for rows k0 .. n - 1 (P is indexed by the absolute row), and the candidates of column 0
template <int NB>
__global__ __launch_bounds__(256) void ease_pivot_load_kernel(const double *A, int64_t ld, int k0, int n, const int *status, double *P, double *part_val,
                                                              int *part_pos) {
    if (*status >= 0) return;
    const int tid = threadIdx.x, chunk = k0 / CHUNK + blockIdx.x, row0 = chunk * CHUNK;
    for (int e = tid; e < CHUNK * NB; e += 256) {
        const int row = row0 + e / NB, c = e % NB;
        if (row >= k0 && row < n) P[(int64_t)row * NB + c] = A[(int64_t)row * ld + k0 + c];
    }
    __syncthreads();
    if (tid < 64) chunk_candidate<NB>(P, row0, k0, n, 0, chunk, part_val, part_pos);
}

// One workgroup: the pivot row of column j (row g = k0 + j of the matrix) from the chunks' candidates, refused when it is 0 or NaN;
// rows g and pivot swap inside the scratch panel; piv[g] and the two figures of mi355rec_ease_pivot_info.
template <int NB>
__global__ __launch_bounds__(256) void ease_pivot_pick_kernel(double *P, int k0, int j, int n, int step, int *status, const double *part_val,
                                                              const int *part_pos, int *piv, double *info) {
    __shared__ double sv[4];
    __shared__ int sp[4];
    if (*status >= 0) return;
    const int tid = threadIdx.x, g = k0 + j;
    double v = -1.0;
    int pos = INT_MAX;
    for (int c = g / CHUNK + tid; c <= (n - 1) / CHUNK; c += 256) {
        const double cv = part_val[c];
        const int cp = part_pos[c];
        if (cand_beats(cv, cp, v, pos)) { v = cv; pos = cp; }
    }
    wave_best(v, pos);
    if ((tid & 63) == 0) { sv[tid >> 6] = v; sp[tid >> 6] = pos; }
    __syncthreads();
    v = sv[0]; pos = sp[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (cand_beats(sv[w], sp[w], v, pos)) { v = sv[w]; pos = sp[w]; }
    if (pos < g || pos >= n) pos = g;       // (cannot happen: row g itself is always a candidate; keeps every address inside the panel)
    const double pivot = P[(int64_t)pos * NB + j];
    if (!(fabs(pivot) > 0.0)) {             // singular (or NaN): the same value in every thread
        if (tid == 0) *status = step;
        return;
    }
    __syncthreads();                        // everybody has read the pivot before its row moves
    if (pos != g && tid < NB) {
        const double a = P[(int64_t)g * NB + tid], b = P[(int64_t)pos * NB + tid];
        P[(int64_t)g * NB + tid] = b;
        P[(int64_t)pos * NB + tid] = a;
    }
    if (tid == 0) {
        piv[g] = pos;
        info[0] = fmin(info[0], fabs(pivot));
        if (pos != g) info[1] += 1.0;
    }
}

// Column j of the scratch panel is eliminated from rows g + 1 .. n - 1 (columns j + 1 .. NB - 1 change), 64 rows per workgroup, and
// the candidates of column j + 1 are left for the next pick.
template <int NB>
__global__ __launch_bounds__(256) void ease_pivot_elim_kernel(double *P, int k0, int j, int n, const int *status, double *part_val, int *part_pos) {
    if (*status >= 0) return;
    const int tid = threadIdx.x, g = k0 + j, chunk = (g + 1) / CHUNK + blockIdx.x, row0 = chunk * CHUNK;
    const int c = tid % NB;
    const double *prow = P + (int64_t)g * NB;
    const double pivot = prow[j], u = prow[c];
    if (c > j) {
        for (int r = tid / NB; r < CHUNK; r += 256 / NB) {
            const int row = row0 + r;
            if (row > g && row < n) {
                double *cell = P + (int64_t)row * NB;
                cell[c] -= cell[j] / pivot * u;
            }
        }
    }
    __syncthreads();
    if (tid < 64) chunk_candidate<NB>(P, row0, g + 1, n, j + 1, chunk, part_val, part_pos);
}

// the swaps (k0 + j, piv[k0 + j]), j = 0 .. count - 1, in order, on whole rows: one thread per column
__global__ __launch_bounds__(128) void ease_pivot_swap_kernel(double *A, int64_t ld, int k0, int count, const int *piv, const int *status) {
    if (*status >= 0) return;
    double *col = A + (int64_t)blockIdx.x * 128 + threadIdx.x;
    for (int j = 0; j < count; ++j) {
        const int g = k0 + j, p = piv[g];
        if (p != g) {
            const double a = col[(int64_t)g * ld], b = col[(int64_t)p * ld];
            col[(int64_t)g * ld] = b;
            col[(int64_t)p * ld] = a;
        }
    }
}

// ---- the block step in float64 -----------------------------------------------------------------------------------------------
// D = A[k0 .. k0 + NB, k0 .. k0 + NB]^-1 by Gauss-Jordan without pivoting: ease_diag_kernel (ease.hip) reading doubles, refusing only a
// pivot that is 0 or NaN, writing D and its transpose (the A operand of R = D A[k,:]).
template <int NB>
__global__ __launch_bounds__(1024) void ease_diag64_kernel(const double *A, int64_t ld, int k0, int step, int *status, double *D, double *Dt) {
    constexpr int P = NB / 32;
    __shared__ double col[2][NB], row[2][NB];
    if (*status >= 0) return;
    const int tid = threadIdx.x, i0 = (tid >> 5) * P, c0 = (tid & 31) * P;
    double a[P][P];
#pragma unroll
    for (int x = 0; x < P; ++x)
#pragma unroll
        for (int y = 0; y < P; ++y) a[x][y] = A[(int64_t)(k0 + i0 + x) * ld + k0 + c0 + y];
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
        if (!(fabs(p) > 0.0)) {            // singular (or NaN): the same value in every thread
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
        for (int y = 0; y < P; ++y) {
            D[(i0 + x) * NB + c0 + y] = a[x][y];
            Dt[(c0 + y) * NB + i0 + x] = a[x][y];
        }
}

// Ct[m][t0 + r] = A[t0 + r][k0 + m] for the 32 rows t0 .. t0 + 31: the column panel, k-major
template <int NB>
__global__ __launch_bounds__(256) void ease_transpose64_kernel(const double *A, int64_t ld, int k0, const int *status, double *Ct) {
    __shared__ double t[32][NB + 1];
    if (*status >= 0) return;
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * 32;
    for (int e = tid; e < 32 * NB; e += 256) {
        const int r = e / NB, m = e % NB;
        t[r][m] = A[(t0 + r) * ld + k0 + m];
    }
    __syncthreads();
    for (int e = tid; e < 32 * NB; e += 256) {
        const int m = e / 32, r = e % 32;
        Ct[(int64_t)m * ld + t0 + r] = t[r][m];
    }
}

// One T x T tile (T = 32 TS) of  X[r][c] = sum_m Aop[m][r] Bop[m][c], m < K:   MODE 0: C = X,  1: C = -X,  2: C -= X.
// 2 x 2 wavefronts, TS x TS accumulators of v_mfma_f64_16x16x4_f64 each (lane (g = lane / 16, c = lane % 16) supplies A[c][g] and
// B[g][c] of a K quad and holds D[4 i + g][c], i < 4), both operands k-major in LDS, the next K chunk's 16-byte loads in flight during
// the MFMAs of the current one.  Every extent is a multiple of its tile: no edge code.  <4, 2> is the elimination's update: its 128
// accumulator registers and the rest fit the 256 of two wavefronts per SIMD (asked for below), so two workgroups share a CU and one
// multiplies while the other waits at its barriers.
template <int TS, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void ease_gemm64_kernel(double *C, int64_t ldc, const double *Aop, int64_t lda, const double *Bop, int64_t ldb, int K,
                                                          const int *status) {
    constexpr int T = 32 * TS, LDT = T + 2, HALF = T / 2;
    __shared__ __attribute__((aligned(16))) double As[GK][LDT];        // [m][row of the tile]
    __shared__ __attribute__((aligned(16))) double Bs[GK][LDT];        // [m][column of the tile]
    if (*status >= 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, g = lane >> 4, c = lane & 15;
    const int64_t row0 = (int64_t)blockIdx.y * T, col0 = (int64_t)blockIdx.x * T;
    f64x4 acc[TS][TS];
#pragma unroll
    for (int a = 0; a < TS; ++a)
#pragma unroll
        for (int b = 0; b < TS; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[a][b][r] = 0.0;
    // staging: thread t moves pairs e = t + 256 i (i < TS) of both operands: m = e / HALF, cells 2 (e % HALF), + 1
    const int sm = tid / HALF, sp = (tid % HALF) * 2;
    constexpr int SM_STEP = 256 / HALF;
    const double *ap = Aop + (int64_t)sm * lda + row0 + sp, *bp = Bop + (int64_t)sm * ldb + col0 + sp;
    f64x2 ra[TS], rb[TS];
#pragma unroll
    for (int i = 0; i < TS; ++i) {
        ra[i] = *reinterpret_cast<const f64x2 *>(ap + (int64_t)(SM_STEP * i) * lda);
        rb[i] = *reinterpret_cast<const f64x2 *>(bp + (int64_t)(SM_STEP * i) * ldb);
    }
    for (int m0 = 0; m0 < K; m0 += GK) {
        __syncthreads();                   // everybody has finished multiplying the previous chunk
#pragma unroll
        for (int i = 0; i < TS; ++i) {
            *reinterpret_cast<f64x2 *>(&As[sm + SM_STEP * i][sp]) = ra[i];
            *reinterpret_cast<f64x2 *>(&Bs[sm + SM_STEP * i][sp]) = rb[i];
        }
        __syncthreads();
        if (m0 + GK < K) {
#pragma unroll
            for (int i = 0; i < TS; ++i) {
                ra[i] = *reinterpret_cast<const f64x2 *>(ap + (int64_t)(m0 + GK + SM_STEP * i) * lda);
                rb[i] = *reinterpret_cast<const f64x2 *>(bp + (int64_t)(m0 + GK + SM_STEP * i) * ldb);
            }
        }
        const double *a_col = &As[g][wm * HALF + c];
        const double *b_col = &Bs[g][wn * HALF + c];
#pragma unroll
        for (int s = 0; s < GK; s += 4) {
            double av[TS], bv[TS];
#pragma unroll
            for (int t = 0; t < TS; ++t) {
                av[t] = a_col[s * LDT + 16 * t];
                bv[t] = b_col[s * LDT + 16 * t];
            }
#pragma unroll
            for (int a = 0; a < TS; ++a)
#pragma unroll
                for (int b = 0; b < TS; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
    }
    double *cell = C + (row0 + wm * HALF + g) * ldc + col0 + wn * HALF + c;
#pragma unroll
    for (int a = 0; a < TS; ++a)
#pragma unroll
        for (int b = 0; b < TS; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double *at = cell + (int64_t)(16 * a + 4 * i) * ldc + 16 * b;
                if (MODE == 0) *at = acc[a][b][i];
                else if (MODE == 1) *at = -acc[a][b][i];
                else *at -= acc[a][b][i];
            }
}

// A[k,:] = R, A[:,k] = ND, A[k,k] = D for the 64 columns (rows) t0 .. t0 + 63 (whatever the update has written there is replaced)
template <int NB>
__global__ __launch_bounds__(256) void ease_writeback64_kernel(double *A, int64_t ld, int k0, const int *status, const double *D, const double *R,
                                                               const double *ND) {
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

// ---- in and out ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ease_widen64_kernel(const float *A32, double *A64, int64_t cells) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < cells; e += (int64_t)gridDim.x * 256) A64[e] = (double)A32[e];
}

__global__ void ease_pivot_init_kernel(int *piv, int npad, double *info) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < npad) piv[i] = i;
    if (i == 0) { info[0] = INFINITY; info[1] = 0.0; }
}

// A32[i][j] = A64[i][inv_perm[j]]: the row swaps undone on the columns while the result is rounded to float32
__global__ __launch_bounds__(256) void ease_gather32_kernel(const double *A64, float *A32, int64_t ld, int npad, const int *inv_perm) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= npad) return;
    const int src = inv_perm[j];
    for (int i = blockIdx.y; i < npad; i += gridDim.y) A32[(int64_t)i * ld + j] = (float)A64[(int64_t)i * ld + src];
}

}  // namespace
