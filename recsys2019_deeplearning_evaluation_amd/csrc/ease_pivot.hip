// ease_pivot.hip -- the inverse of EASE_R for matrices that are NOT positive definite (explicit ratings: counts, not sums of squares,
// on the diagonal make the matrix symmetric indefinite) on MI355X (gfx950): blocked Gauss-Jordan elimination with partial (row)
// pivoting, float64 throughout  [DESIGN.md section 13].  ease.hip keeps the unpivoted float32 route; this unit shares its handle
// (ease_handle.h) and leaves the result where that route leaves it -- the handle's float32 matrix, state ST_INVERTED -- so weights,
// top-K and the dense scorer's hand-off follow unchanged.
//
// The working matrix is a float64 npad x npad copy of the handle's matrix (same identity tail).  One step per block column k of NB cells:
//   pivot search   LU elimination with partial pivoting on a scratch copy of the panel A[k0 .. n, k0 .. k0 + NB]: ease_pivot_load_kernel
//                  copies it; per column ease_pivot_pick_kernel (one workgroup) reduces the per-chunk candidates to the pivot row
//                  -- the largest |value|, ties to the lowest row, a NaN counts as the largest -- and swaps it up inside the scratch,
//                  ease_pivot_elim_kernel eliminates the column below it and leaves the next column's candidates.  Rows >= n (the
//                  identity tail) are never candidates; a pivot that is 0 or NaN writes the step into the status word
//   ease_pivot_swap_kernel   the NB swaps, in order, on whole rows of the working matrix (converted block columns included)
//   ease_diag64_kernel       D = A[k,k]^-1 by the unpivoted sweep of ease_diag_kernel on doubles (the swaps made the block factorable)
//   ease_transpose64_kernel  Ct = A[:,k]^T
//   ease_gemm64_kernel       R = D A[k,:], ND = -A[:,k] D, and the hot one: A -= Ct^T R, an npad x npad x NB read-modify-write GEMM on
//                            v_mfma_f64_16x16x4_f64 (128 x 128 tiles, operands staged in LDS as ease_update_kernel does)
//   ease_writeback64_kernel  block row k <- R, block column k <- ND, the block itself <- D
// After the last step the row swaps are undone on the COLUMNS, last swap first: the swap list is composed into one permutation on the
// host and ease_gather32_kernel gathers the float32 result from the permuted column while it converts.
// Every dependency is a kernel boundary on the handle's stream; a set status word turns every later kernel into an empty launch; no
// atomics, fixed reduction orders: two runs give the same bits.
#include "common.h"
#include "ease_handle.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <limits>

using namespace mi355rec;

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
constexpr int CHUNK = 64;           // rows of the panel one workgroup of the pivot search handles
constexpr int GK = 16;              // K chunk of the GEMM kernel staged in LDS
constexpr int PANEL_W = 64;         // columns (rows) one workgroup of the write-back handles

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

size_t pivot_bytes(int64_t npad, int block) {
    return (size_t)(npad * npad + 4 * npad * block + 2 * (int64_t)block * block) * sizeof(double);
}

// The workspace, once per handle.  No memory is not an abort: MI355REC_E_UNSUPPORTED with the handle's matrix untouched.  It is decided
// before anything is allocated, from the device's free memory (after the cache of released blocks has gone back to the driver) and from
// MI355REC_EASE_PIVOT_MAX_BYTES, the cap a process that shares the device puts on the workspace (read at every first allocation).
// A hipMalloc that fails all the same is turned into the same code, and the error it leaves in the runtime is taken out, so that the
// next launch check of the handle does not report it.
void ensure_work(mi355rec_ease *h) {
    EasePivotWork &w = h->pivot;
    while ((int)w.events.size() < 4 * h->steps) {           // (a failure here is an ordinary MI355REC_E_HIP)
        hipEvent_t e;
        MI_HIP(hipEventCreate(&e));
        w.events.push_back(e);
    }
    if (w.A.ptr) return;
    const int64_t npad = h->npad;
    const int block = h->block;
    const size_t need = pivot_bytes(npad, block);
    if (const char *v = getenv("MI355REC_EASE_PIVOT_MAX_BYTES")) {
        const unsigned long long cap = strtoull(v, nullptr, 10);
        if (need > cap)
            fail(MI355REC_E_UNSUPPORTED, "no device memory for the float64 working matrix of the pivoted inverse (%.2f GB for %d items): "
                 "MI355REC_EASE_PIVOT_MAX_BYTES allows %llu bytes", need / 1e9, h->n, cap);
    }
    const size_t reserve = (size_t)64 << 20;                // for the small buffers' rounding and the runtime
    size_t free_b = 0, total_b = 0;
    MI_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need + reserve > free_b) {
        uint64_t freed = 0;
        (void)mi355rec_device_trim(&freed);
        MI_HIP(hipMemGetInfo(&free_b, &total_b));
    }
    if (need + reserve > free_b)
        fail(MI355REC_E_UNSUPPORTED, "no device memory for the float64 working matrix of the pivoted inverse (%.2f GB for %d items): %.2f GB are free",
             need / 1e9, h->n, free_b / 1e9);
    try {
        w.A.alloc((size_t)npad * npad);
        w.panel.alloc((size_t)npad * block);
        w.D.alloc((size_t)block * block);
        w.Dt.alloc((size_t)block * block);
        w.R.alloc((size_t)block * npad);
        w.Ct.alloc((size_t)block * npad);
        w.ND.alloc((size_t)block * npad);
        w.part_val.alloc((size_t)npad / CHUNK);
        w.part_pos.alloc((size_t)npad / CHUNK);
        w.piv.alloc((size_t)npad);
        w.inv_perm.alloc((size_t)npad);
        w.info.alloc(2);
    } catch (const Error &e) {
        const std::string why = e.what();
        (void)hipGetLastError();
        ReleaseScope scope(h->stream);
        for (DeviceBuffer<double> *b : {&w.A, &w.panel, &w.D, &w.Dt, &w.R, &w.Ct, &w.ND, &w.part_val, &w.info}) b->release();
        for (DeviceBuffer<int> *b : {&w.part_pos, &w.piv, &w.inv_perm}) b->release();
        fail(MI355REC_E_UNSUPPORTED, "no device memory for the float64 working matrix of the pivoted inverse (%.2f GB for %d items): %s", need / 1e9, h->n,
             why.c_str());
    }
}

template <int NB>
void enqueue_pivoted_elimination(mi355rec_ease *h) {
    EasePivotWork &w = h->pivot;
    hipStream_t s = h->stream;
    const int64_t ld = h->npad;
    const int n = h->n, npad = h->npad;
    int *status = h->status.ptr;
    const int tiles = npad / 128, last_chunk = (n - 1) / CHUNK;
    for (int step = 0; step < h->steps; ++step) {
        const int k0 = step * NB, cols = std::min(NB, n - k0);      // cols <= 0: the block lies in the identity tail, nothing to search
        MI_HIP(hipEventRecord(w.events[4 * step], s));
        if (cols > 0) {
            hipLaunchKernelGGL(ease_pivot_load_kernel<NB>, dim3(last_chunk - k0 / CHUNK + 1), dim3(256), 0, s, w.A.ptr, ld, k0, n, status, w.panel.ptr,
                               w.part_val.ptr, w.part_pos.ptr);
            h->launches += 1;
            for (int j = 0; j < cols; ++j) {
                const int g = k0 + j;
                hipLaunchKernelGGL(ease_pivot_pick_kernel<NB>, dim3(1), dim3(256), 0, s, w.panel.ptr, k0, j, n, step, status, w.part_val.ptr, w.part_pos.ptr,
                                   w.piv.ptr, w.info.ptr);
                h->launches += 1;
                if (j + 1 < NB && g + 1 < n) {      // (the last column of a panel has nothing to its right, the last row nothing below)
                    hipLaunchKernelGGL(ease_pivot_elim_kernel<NB>, dim3(last_chunk - (g + 1) / CHUNK + 1), dim3(256), 0, s, w.panel.ptr, k0, j, n, status,
                                       w.part_val.ptr, w.part_pos.ptr);
                    h->launches += 1;
                }
            }
            hipLaunchKernelGGL(ease_pivot_swap_kernel, dim3(npad / 128), dim3(128), 0, s, w.A.ptr, ld, k0, cols, w.piv.ptr, status);
            h->launches += 1;
        }
        MI_HIP(hipEventRecord(w.events[4 * step + 1], s));
        hipLaunchKernelGGL(ease_diag64_kernel<NB>, dim3(1), dim3(1024), 0, s, w.A.ptr, ld, k0, step, status, w.D.ptr, w.Dt.ptr);
        hipLaunchKernelGGL(ease_transpose64_kernel<NB>, dim3(npad / 32), dim3(256), 0, s, w.A.ptr, ld, k0, status, w.Ct.ptr);
        // R = D A[k,:]: X[m][c] = sum_q Dt[q][m] A[k0 + q][c];  ND = -A[:,k] D: X[r][m] = sum_q Ct[q][r] D[q][m]
        hipLaunchKernelGGL((ease_gemm64_kernel<2, 0>), dim3(npad / 64, NB / 64), dim3(256), 0, s, w.R.ptr, ld, w.Dt.ptr, (int64_t)NB, w.A.ptr + (int64_t)k0 * ld, ld,
                           NB, status);
        hipLaunchKernelGGL((ease_gemm64_kernel<2, 1>), dim3(NB / 64, npad / 64), dim3(256), 0, s, w.ND.ptr, (int64_t)NB, w.Ct.ptr, ld, w.D.ptr, (int64_t)NB, NB,
                           status);
        MI_HIP(hipEventRecord(w.events[4 * step + 2], s));
        hipLaunchKernelGGL((ease_gemm64_kernel<4, 2>), dim3(tiles, tiles), dim3(256), 0, s, w.A.ptr, ld, w.Ct.ptr, ld, w.R.ptr, ld, NB, status);
        MI_HIP(hipEventRecord(w.events[4 * step + 3], s));
        hipLaunchKernelGGL(ease_writeback64_kernel<NB>, dim3(npad / PANEL_W), dim3(256), 0, s, w.A.ptr, ld, k0, status, w.D.ptr, w.R.ptr, w.ND.ptr);
        h->launches += 6;
    }
    MI_HIP(hipGetLastError());
}

}  // namespace

extern "C" int mi355rec_ease_invert_pivoted(mi355rec_ease_t h) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL argument");
        MI_REQUIRE(h->state == ST_MATRIX, "invert_pivoted needs a matrix that has been set and not yet inverted");
        ensure_device();
        ensure_work(h);                                         // (no memory: the matrix is still there, the state stays ST_MATRIX)
        EasePivotWork &w = h->pivot;
        hipStream_t s = h->stream;
        const int npad = h->npad;
        h->state = ST_FAILED;                                   // until the status word says otherwise
        w.valid = false;
        MI_HIP(hipMemsetAsync(h->status.ptr, 0xFF, sizeof(int), s));      // -1: no step has failed
        h->launches = 0;
        h->timer.start(s);
        hipLaunchKernelGGL(ease_pivot_init_kernel, dim3(div_up(npad, 256)), dim3(256), 0, s, w.piv.ptr, npad, w.info.ptr);
        hipLaunchKernelGGL(ease_widen64_kernel, dim3(std::min<int64_t>(((int64_t)npad * npad + 255) / 256, 65536)), dim3(256), 0, s, h->A.ptr, w.A.ptr,
                           (int64_t)npad * npad);
        h->launches += 2;
        if (h->block == 64) enqueue_pivoted_elimination<64>(h);
        else enqueue_pivoted_elimination<128>(h);
        h->timer.stop(s);
        int failed = -1;
        double info[2] = {0, 0};
        std::vector<int> piv((size_t)npad);
        MI_HIP(hipMemcpyAsync(&failed, h->status.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
        MI_HIP(hipMemcpyAsync(info, w.info.ptr, sizeof(info), hipMemcpyDeviceToHost, s));
        MI_HIP(hipMemcpyAsync(piv.data(), w.piv.ptr, (size_t)npad * sizeof(int), hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
        h->invert_ms = h->timer.elapsed_ms();
        h->failed_step = failed;
        w.pivot_ms = w.update_ms = 0;
        for (int step = 0; step < h->steps; ++step) {
            float a = 0.f, b = 0.f;
            MI_HIP(hipEventElapsedTime(&a, w.events[4 * step], w.events[4 * step + 1]));
            MI_HIP(hipEventElapsedTime(&b, w.events[4 * step + 2], w.events[4 * step + 3]));
            w.pivot_ms += a;
            w.update_ms += b;
        }
        w.min_pivot = info[0];
        w.moved = (int)info[1];
        w.valid = true;
        if (failed < 0) {
            // row g of the permuted matrix is row order[g] of the original; (P G)^-1 = G^-1 P^T, so column order[l] of G^-1 is column l
            // of what was computed: the swaps undone on the columns, last first
            std::vector<int> order((size_t)npad), inv_perm((size_t)npad);
            for (int i = 0; i < npad; ++i) order[i] = i;
            for (int g = 0; g < h->n; ++g)
                if (piv[g] != g) std::swap(order[g], order[piv[g]]);
            for (int l = 0; l < npad; ++l) inv_perm[order[l]] = l;
            MI_HIP(hipMemcpyAsync(w.inv_perm.ptr, inv_perm.data(), (size_t)npad * sizeof(int), hipMemcpyHostToDevice, s));
            h->call_timer.start(s);
            hipLaunchKernelGGL(ease_gather32_kernel, dim3(div_up(npad, 256), std::min(npad, 1024)), dim3(256), 0, s, w.A.ptr, h->A.ptr,
                               (int64_t)npad, npad, w.inv_perm.ptr);
            MI_HIP(hipGetLastError());
            h->call_timer.stop(s);
            h->launches += 1;
            MI_HIP(hipStreamSynchronize(s));
            h->invert_ms += h->call_timer.elapsed_ms();
        }
        h->stats = mi355rec_stats{};
        h->stats.kernel_ms = h->stats.call_ms = h->invert_ms;
        h->stats.n_launches = h->launches;
        h->stats.n_timed = 1;
        h->stats.n_units = h->steps;
        h->stats.algorithmic_flops = 2.0 * (double)h->n * h->n * h->n;
        h->stats.algorithmic_bytes = 16.0 * (double)h->n * h->n * h->steps;     // every step reads and writes the float64 matrix once
        if (failed >= 0)
            fail(MI355REC_E_NUMERIC, "the matrix is singular: a pivot that is 0 (or NaN) in elimination step %d of %d (block size %d)", failed, h->steps,
                 h->block);
        h->state = ST_INVERTED;
    });
}

extern "C" int mi355rec_ease_pivot_info(mi355rec_ease_t h, int32_t *moved_rows, double *min_pivot, double *pivot_ms, double *update_ms) {
    return guarded([&] {
        MI_REQUIRE(h && moved_rows && min_pivot && pivot_ms && update_ms, "NULL argument");
        MI_REQUIRE(h->pivot.valid, "no pivoted inverse has run on the matrix that is set");
        *moved_rows = h->pivot.moved;
        *min_pivot = h->pivot.min_pivot;
        *pivot_ms = h->pivot.pivot_ms;
        *update_ms = h->pivot.update_ms;
    });
}
