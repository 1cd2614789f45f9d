// nmf.hip -- the device half of NMFRecommender on MI355X (gfx950)  [DESIGN.md section 12].
//
// The reference (MatrixFactorization/NMFRecommender.py:58-71) hands URM_train to sklearn.decomposition.NMF: coordinate descent or
// multiplicative updates on W (users x k) and H (k x items), then a second solve for W alone.  The handle keeps the URM in both
// layouts, W and Ht = H^T (items x k) and one value buffer per layout resident; an iteration is driven from Python through the
// step-wise entry points below, because it needs a fresh permutation and the stop statistic on the host anyway.  "Side" s is the
// block being updated (0: W from the CSR layout, 1: Ht from the CSC layout); the other block is held fixed, so both half-steps of
// an iteration are the same code.
//
//   nmf_cd_sweep_kernel  one half-sweep of coordinate descent: a row of the block per group of 16 / 32 / 64 lanes, the row in LDS (a
//                        lane owns the columns lp apart and no other lane reads them), every workgroup walking the permutation in
//                        lock-step.  Per component t: grad = W[i] . HHt[t] - XHt[i,t] as a FRESH dot product (lane-private FMAs, a
//                        butterfly over the group: every lane ends with the same bits), the projected gradient into a float64
//                        violation sum, W[i,t] = max(W[i,t] - grad / HHt[t,t], 0).  Workgroup sums are written in a fixed order and
//                        added by nmf_sum_kernel: no atomics, a sweep is bitwise repeatable.
//   nmf_sddmm_kernel     per cell of a layout, in its own cell order: wh = max(W[i] . Ht[c], eps32); <false>: q = x / wh, the value
//                        stream of the product that follows; <true>: x log(x / wh) into float64 workgroup sums (the divergence).
//                        A piece of a row per group of lanes as in the product, the row's own factors in registers, four cells at a
//                        time so that four gathered rows are in flight and the four sums share their cross-lane exchanges.
//   nmf_scale_kernel     block *= numerator / denominator (a matrix or one value per column), zero denominators replaced, the
//                        Kullback-Leibler floor on Ht.
//   nmf_colsum_*, nmf_dot_kernel, nmf_sum_kernel   float64 reductions in a fixed order.
//   products, Gram, block * matrix: svd.hip's kernels (svd_product.h) and score.hip's f32 MFMA GEMM (gemm_rows_enqueue).
#include "common.h"
#include "score.h"
#include "svd_product.h"

#include <algorithm>
#include <memory>

using namespace mi355rec;

namespace {

constexpr int NT = 256;                    // threads of every kernel here
constexpr int SD_CPL = 4;                  // columns of its own row an SDDMM lane keeps in registers
constexpr int SD_CELLS = 4;                // cells an SDDMM group works on together
constexpr float EPS32 = 1.1920929e-07f;    // sklearn's EPSILON = np.finfo(np.float32).eps
constexpr double EPS64 = 2.220446049250313e-16;
constexpr int RED_BLOCKS = 1024;           // workgroups of a grid-wide reduction
constexpr int CS_SLABS = 512;              // row slabs of a column sum

// the fixed-order sum of one double per thread: thread 0 adds them by thread index
__device__ __forceinline__ void block_sum_to(double v, double *red, double *out) {
    red[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < NT; ++i) s += red[i];
        *out = s;
    }
}

__device__ __forceinline__ float group_sum(float v, int lp) {
    for (int m = lp >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(NT) void nmf_cd_sweep_kernel(float *__restrict__ W, int n, int k, int lp_shift,
                                                           const float *__restrict__ HHt, const float *__restrict__ XHt,
                                                           const int *__restrict__ perm, double *__restrict__ part) {
    extern __shared__ float w_lds[];                   // [q][thread]: column sub + q * lp of the thread's row; thread-private
    __shared__ double red[NT];
    const int lp = 1 << lp_shift, tid = threadIdx.x, sub = tid & (lp - 1);
    const int row = blockIdx.x * (NT >> lp_shift) + (tid >> lp_shift);
    const bool live = row < n;
    const size_t base = (size_t)(live ? row : n - 1) * k;              // rows past the end compute on zeros and write nothing
    const int nq = (k + lp - 1) >> lp_shift;
    for (int q = 0; q < nq; ++q) {
        const int c = sub + (q << lp_shift);
        w_lds[q * NT + tid] = (live && c < k) ? W[base + c] : 0.f;
    }
    const int group_lane0 = (tid & 63) & ~(lp - 1);
    double viol = 0.0;
    for (int s = 0; s < k; ++s) {
        const int t = perm[s];
        const float *hrow = HHt + (size_t)t * k;
        float acc = 0.f;
#pragma unroll 4
        for (int q = 0; q < nq; ++q) {
            const int c = sub + (q << lp_shift);
            if (c < k) acc = fmaf(hrow[c], w_lds[q * NT + tid], acc);
        }
        acc = group_sum(acc, lp);
        const int owner = t & (lp - 1), slot = (t >> lp_shift) * NT + tid;
        const float wt = __shfl(w_lds[slot], group_lane0 | owner);
        const float grad = acc - XHt[base + t], hess = hrow[t];
        const float pg = wt == 0.f ? fminf(0.f, grad) : grad;
        if (live && sub == 0) viol += fabs((double)pg);
        if (hess != 0.f && sub == owner) w_lds[slot] = fmaxf(wt - grad / hess, 0.f);
    }
    if (live)
        for (int q = 0; q < nq; ++q) {
            const int c = sub + (q << lp_shift);
            if (c < k) W[base + c] = w_lds[q * NT + tid];
        }
    block_sum_to(viol, red, part + blockIdx.x);
}

// one piece (at most 512 cells of one row) per group of lp lanes; A: the rows of the layout, B: the gathered side
template <bool LOG>
__global__ __launch_bounds__(NT) void nmf_sddmm_kernel(const int *__restrict__ p_row, const int *__restrict__ p_begin,
                                                        const int *__restrict__ p_end, int n_pieces, const int *__restrict__ idx,
                                                        const float *__restrict__ val, const float *__restrict__ A,
                                                        const float *__restrict__ B, int k, int lp_shift, float *__restrict__ q_out,
                                                        double *__restrict__ part) {
    __shared__ double red[NT];
    const int lp = 1 << lp_shift, tid = threadIdx.x, sub = tid & (lp - 1);
    const int piece = (blockIdx.x * NT + tid) >> lp_shift;
    const bool live = piece < n_pieces;
    const int b = live ? p_begin[piece] : 0, e = live ? p_end[piece] : 0;
    const float *arow = A + (size_t)(live ? p_row[piece] : 0) * k;
    float a[SD_CPL];
#pragma unroll
    for (int q = 0; q < SD_CPL; ++q) a[q] = (sub + q * lp < k) ? arow[sub + q * lp] : 0.f;
    double sum = 0.0;
    // the groups of a wavefront hold pieces of different lengths: every lane walks the longest one, so that the exchanges below
    // are never executed by part of a wavefront
    int len = e - b;
    for (int m = lp; m < 64; m <<= 1) len = max(len, __shfl_xor(len, m));
    const int half = lp >> 1, quarter = lp >> 2;
    const bool hi = (sub & half) != 0, hq = (sub & quarter) != 0;
    const int mine = (hi ? 2 : 0) + (hq ? 1 : 0);      // the cell of the four whose sum ends in this lane's quarter of the group
    for (int o = 0; o < len; o += SD_CELLS) {
        // four cells at a time: their gathered rows are in flight together, and the four sums over the group cost 3 + log2(lp / 4)
        // exchanges instead of 4 log2(lp)
        float acc[SD_CELLS];
        const float *brow[SD_CELLS];
#pragma unroll
        for (int u = 0; u < SD_CELLS; ++u) {
            const int j = b + o + u;
            brow[u] = j < e ? B + (size_t)idx[j] * k : nullptr;
            acc[u] = 0.f;
        }
#pragma unroll
        for (int q = 0; q < SD_CPL; ++q)
#pragma unroll
            for (int u = 0; u < SD_CELLS; ++u)
                if (brow[u] && sub + q * lp < k) acc[u] = fmaf(a[q], brow[u][sub + q * lp], acc[u]);
        for (int c = sub + SD_CPL * lp; c < k; c += lp) {
            const float ac = arow[c];
#pragma unroll
            for (int u = 0; u < SD_CELLS; ++u)
                if (brow[u]) acc[u] = fmaf(ac, brow[u][c], acc[u]);
        }
        // the upper half of the group takes over cells 2 and 3, the lower half cells 0 and 1; then the quarters split the pair
        float k0 = (hi ? acc[2] : acc[0]) + __shfl_xor(hi ? acc[0] : acc[2], half);
        float k1 = (hi ? acc[3] : acc[1]) + __shfl_xor(hi ? acc[1] : acc[3], half);
        float total = (hq ? k1 : k0) + __shfl_xor(hq ? k0 : k1, quarter);
        for (int m = quarter >> 1; m > 0; m >>= 1) total += __shfl_xor(total, m);
        const int j = b + o + mine;
        if (j < e && (sub & (quarter - 1)) == 0) {
            const float x = val ? val[j] : 1.f, wh = fmaxf(total, EPS32);
            if (LOG) {
                if (x > EPS32) sum += (double)x * log((double)x / (double)wh);
            } else {
                q_out[j] = x / wh;
            }
        }
    }
    if (LOG) block_sum_to(sum, red, part + blockIdx.x);
}

// X[i][c] *= num[i][c] / den, den = den_m[i][c] or den_v[c]; a zero den is replaced by zero_to; floor: results below eps64 become 0
__global__ __launch_bounds__(NT) void nmf_scale_kernel(float *__restrict__ X, const float *__restrict__ num, const float *__restrict__ den_m,
                                                        const float *__restrict__ den_v, size_t cells, int k, float zero_to, int floor) {
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e >= cells) return;
    float d = den_m ? den_m[e] : den_v[e % k];
    if (d == 0.f) d = zero_to;
    float x = X[e] * (num[e] / d);
    if (floor && (double)x < EPS64) x = 0.f;
    X[e] = x;
}

__global__ __launch_bounds__(NT) void nmf_fill_kernel(float *__restrict__ X, size_t cells, float value) {
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e < cells) X[e] = value;
}

// part[slab][c] = sum of X[row][c] over the slab's rows, in row order
__global__ __launch_bounds__(NT) void nmf_colsum_kernel(const float *__restrict__ X, int n, int k, int rows_per_slab, double *__restrict__ part) {
    const int c = blockIdx.y * NT + threadIdx.x, slab = blockIdx.x;
    if (c >= k) return;
    const int r0 = slab * rows_per_slab, r1 = min(n, r0 + rows_per_slab);
    double s = 0.0;
    for (int row = r0; row < r1; ++row) s += (double)X[(size_t)row * k + c];
    part[(size_t)slab * k + c] = s;
}

__global__ __launch_bounds__(NT) void nmf_colsum_reduce_kernel(const double *__restrict__ part, int n_slabs, int k, double *__restrict__ out,
                                                                float *__restrict__ out_f) {
    const int c = blockIdx.x * NT + threadIdx.x;
    if (c >= k) return;
    double s = 0.0;
    for (int slab = 0; slab < n_slabs; ++slab) s += part[(size_t)slab * k + c];
    out[c] = s;
    if (out_f) out_f[c] = (float)s;
}

__global__ __launch_bounds__(NT) void nmf_to_float_kernel(const double *__restrict__ in, float *__restrict__ out, size_t cells) {
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e < cells) out[e] = (float)in[e];
}

// part[block] = sum of a[i] * b[i] over the block's contiguous share of [0, len), every thread a contiguous run of it
template <class T>
__global__ __launch_bounds__(NT) void nmf_dot_kernel(const T *__restrict__ a, const T *__restrict__ b, size_t len, double *__restrict__ part) {
    __shared__ double red[NT];
    const size_t per_block = (len + gridDim.x - 1) / gridDim.x, per_thread = (per_block + NT - 1) / NT;
    const size_t b0 = (size_t)blockIdx.x * per_block, b1 = min(len, b0 + per_block);
    const size_t t0 = min(b1, b0 + (size_t)threadIdx.x * per_thread), t1 = min(b1, t0 + per_thread);
    double s = 0.0;
    for (size_t i = t0; i < t1; ++i) s += (double)a[i] * (double)b[i];
    block_sum_to(s, red, part + blockIdx.x);
}

// out[0] (+)= part[0] + part[1] + ...: one workgroup, every thread a contiguous run, the runs added by thread index
__global__ __launch_bounds__(NT) void nmf_sum_kernel(const double *__restrict__ part, int n, double *__restrict__ out, int accumulate) {
    __shared__ double red[NT];
    __shared__ double total;
    const int per_thread = (n + NT - 1) / NT;
    const int t0 = min(n, (int)threadIdx.x * per_thread), t1 = min(n, t0 + per_thread);
    double s = 0.0;
    for (int i = t0; i < t1; ++i) s += part[i];
    block_sum_to(s, red, &total);
    if (threadIdx.x == 0) out[0] = accumulate ? out[0] + total : total;
}

// scal[OUT] of the two divergences from the sums the kernels above left in scal[]
__global__ void nmf_divergence_kernel(double *scal, int loss, double norm_x, double sum_x) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    // frobenius: (|X|^2 + tr((W^T W)(H H^T)) - 2 sum (X H^T) o W) / 2;  Kullback-Leibler: sum x log(x / wh) + (sum W)(sum H) - sum x
    scal[3] = loss == 0 ? (norm_x + scal[1] - 2.0 * scal[2]) / 2.0 : scal[1] + scal[2] - sum_x;
}

enum Phase { PH_PRODUCT = 0, PH_GEMM, PH_SWEEP, PH_SCALE, PH_SDDMM, PH_REDUCE, N_PHASES };
enum Scalar { SC_VIOLATION = 0, SC_A, SC_B, SC_OUT, N_SCALARS };

}  // namespace

struct mi355rec_nmf : Handle {
    int n_users = 0, n_items = 0, k = 0, ones = 0;
    size_t nnz = 0;
    double norm_x = 0.0, sum_x = 0.0;                  // sum of x^2; sum of the x above eps32
    Side sides[2];                                     // [0]: rows = users (the CSR layout), [1]: rows = items (the CSC layout)
    DeviceBuffer<float> block[2], num, den, partial, q[2], Gf, colsum_f;
    DeviceBuffer<double> gram_part, G[2], colsum_part, colsum[2], red_part, scal;
    DeviceBuffer<int> iota, perm;
    GramPlan gram_plan[2];
    int prepared_side = -1, prepared_loss = -1;        // what Gf and num, or colsum_f, currently hold
    double phase_ms[N_PHASES] = {0, 0, 0, 0, 0, 0};
    int open_phase = -1;
    std::vector<int> phase_of;                         // of every event pair used in the current call
    int64_t launches = 0, calls = 0, create_bytes = 0, h2d_bytes = 0, d2h_bytes = 0;

    int rows_of(int s) const { return s == 0 ? n_users : n_items; }
    const float *values(int s) const { return ones ? nullptr : sides[s].val.ptr; }
    int lp_shift() const { return k <= 16 ? 4 : (k <= 32 ? 5 : 6); }

    void start_call() {                                // a call that failed half-way leaves event pairs behind
        dispatch_timers.reset();
        phase_of.clear();
    }
    void begin(int phase) {
        hipEvent_t a, b;
        dispatch_timers.reserve(dispatch_timers.used + 1);
        dispatch_timers.next(a, b, 1 << 30);
        MI_HIP(hipEventRecord(a, stream));
        phase_of.push_back(phase);
    }
    void end() { MI_HIP(hipEventRecord(dispatch_timers.stop[dispatch_timers.used - 1], stream)); }
    // waits for the call's work, books its phases and leaves the figures of the call in `stats`
    void finish_call(int main_phase, double bytes, double flops) {
        MI_HIP(hipStreamSynchronize(stream));
        stats = mi355rec_stats{};
        for (int i = 0; i < dispatch_timers.used; ++i) {
            float ms = 0.f;
            MI_HIP(hipEventElapsedTime(&ms, dispatch_timers.start[i], dispatch_timers.stop[i]));
            phase_ms[phase_of[i]] += ms;
            stats.call_ms += ms;
            if (phase_of[i] == main_phase) stats.kernel_ms += ms;
        }
        stats.n_launches = stats.n_timed = dispatch_timers.used;
        stats.n_units = (int64_t)nnz;
        stats.algorithmic_bytes = bytes;
        stats.algorithmic_flops = flops;
        dispatch_timers.reset();
        phase_of.clear();
        ++calls;
    }

    ~mi355rec_nmf() { shutdown(); }
};

namespace {

void enqueue_gram(mi355rec_nmf *h, int side) {
    gram_enqueue(h->block[side].ptr, h->rows_of(side), h->k, h->gram_plan[side], h->gram_part.ptr, h->G[side].ptr, h->stream);
    h->launches += 2;
}

void enqueue_colsum(mi355rec_nmf *h, int side, float *out_f) {
    const int n = h->rows_of(side), k = h->k;
    const int slabs = std::min(CS_SLABS, div_up(n, 64)), rows = div_up(n, slabs), used = div_up(n, rows);
    hipLaunchKernelGGL(nmf_colsum_kernel, dim3(used, div_up(k, NT)), dim3(NT), 0, h->stream, h->block[side].ptr, n, k, rows, h->colsum_part.ptr);
    MI_HIP(hipGetLastError());
    hipLaunchKernelGGL(nmf_colsum_reduce_kernel, dim3(div_up(k, NT)), dim3(NT), 0, h->stream, h->colsum_part.ptr, used, k, h->colsum[side].ptr, out_f);
    MI_HIP(hipGetLastError());
    h->launches += 2;
}

template <class T>
void enqueue_dot(mi355rec_nmf *h, const T *a, const T *b, size_t len, int scalar) {
    const int blocks = std::max(1, std::min<int>(RED_BLOCKS, div_up((int64_t)len, 4 * NT)));
    hipLaunchKernelGGL(nmf_dot_kernel<T>, dim3(blocks), dim3(NT), 0, h->stream, a, b, len, h->red_part.ptr);
    MI_HIP(hipGetLastError());
    hipLaunchKernelGGL(nmf_sum_kernel, dim3(1), dim3(NT), 0, h->stream, h->red_part.ptr, blocks, h->scal.ptr + scalar, 0);
    MI_HIP(hipGetLastError());
    h->launches += 2;
}

// what a frobenius step on `side` reads of the other block: Gf = its Gram matrix (float32 of the float64 sum), num = URM . other
void prepare_frobenius(mi355rec_nmf *h, int side) {
    hipStream_t s = h->stream;
    const int k = h->k;
    h->begin(PH_REDUCE);
    enqueue_gram(h, 1 - side);
    hipLaunchKernelGGL(nmf_to_float_kernel, dim3(div_up((int64_t)k * k, NT)), dim3(NT), 0, s, h->G[1 - side].ptr, h->Gf.ptr, (size_t)k * k);
    MI_HIP(hipGetLastError());
    h->end();
    h->begin(PH_PRODUCT);
    h->launches += 1 + spmm_enqueue(h->sides[side], h->values(side), h->block[1 - side].ptr, k, h->num.ptr, h->partial.ptr, s);
    h->end();
    h->prepared_side = side;
    h->prepared_loss = 0;
}

void enqueue_sddmm(mi355rec_nmf *h, int side, bool log_sum, int &blocks) {
    const Side &sd = h->sides[side];
    const int shift = h->lp_shift();
    blocks = div_up((int64_t)sd.n_pieces << shift, NT);
    if (log_sum)
        hipLaunchKernelGGL(nmf_sddmm_kernel<true>, dim3(blocks), dim3(NT), 0, h->stream, sd.p_row.ptr, sd.p_begin.ptr, sd.p_end.ptr, sd.n_pieces,
                           sd.idx.ptr, h->values(side), h->block[side].ptr, h->block[1 - side].ptr, h->k, shift, (float *)nullptr, h->red_part.ptr);
    else
        hipLaunchKernelGGL(nmf_sddmm_kernel<false>, dim3(blocks), dim3(NT), 0, h->stream, sd.p_row.ptr, sd.p_begin.ptr, sd.p_end.ptr, sd.n_pieces,
                           sd.idx.ptr, h->values(side), h->block[side].ptr, h->block[1 - side].ptr, h->k, shift, h->q[side].ptr, (double *)nullptr);
    MI_HIP(hipGetLastError());
    h->launches += 1;
}

void require_side(int side) { MI_REQUIRE(side == 0 || side == 1, "side %d: 0 (W, users x k) or 1 (Ht, items x k)", side); }
void require_loss(int loss) { MI_REQUIRE(loss == 0 || loss == 1, "loss %d: 0 (frobenius) or 1 (kullback-leibler)", loss); }

}  // namespace

extern "C" int mi355rec_nmf_create(mi355rec_nmf_t *out, int32_t n_users, int32_t n_items, int32_t k, const int32_t *row_ptr,
                                   const int32_t *row_idx, const float *row_val, const int32_t *col_ptr, const int32_t *col_idx,
                                   const float *col_val) {
    return guarded([&] {
        MI_REQUIRE(out && row_ptr && col_ptr, "NULL argument");
        MI_REQUIRE(n_users > 0 && n_items > 0, "empty URM (%d x %d)", n_users, n_items);
        MI_REQUIRE(k >= 1 && k <= 4096, "number of components k = %d outside [1, 4096]", k);
        MI_REQUIRE(row_ptr[n_users] == col_ptr[n_items], "the two layouts hold %d and %d cells", row_ptr[n_users], col_ptr[n_items]);
        const size_t nnz = (size_t)row_ptr[n_users];
        MI_REQUIRE(nnz == 0 || (row_idx && col_idx && row_val && col_val), "NULL argument");
        MI_REQUIRE(div_up(std::max(n_users, n_items), 128) <= 65535, "more than 8 M rows on a side");
        validate_layout(n_users, n_items, row_ptr, row_idx);
        validate_layout(n_items, n_users, col_ptr, col_idx);
        bool ones = true;
        double norm_x = 0.0, sum_x = 0.0;
        for (size_t i = 0; i < nnz; ++i) {
            MI_REQUIRE(row_val[i] >= 0.f, "negative value %g in the URM", (double)row_val[i]);
            ones = ones && row_val[i] == 1.0f;
            norm_x += (double)row_val[i] * row_val[i];
            if (row_val[i] > EPS32) sum_x += row_val[i];
        }
        *out = nullptr;
        auto h = open_handle<mi355rec_nmf>(1);
        h->n_users = n_users;
        h->n_items = n_items;
        h->k = k;
        h->nnz = nnz;
        h->ones = ones ? 1 : 0;
        h->norm_x = norm_x;
        h->sum_x = sum_x;
        ReleaseScope scope(h->stream);
        hipStream_t s = h->stream;
        h->create_bytes += (int64_t)h->sides[0].build(n_users, row_ptr, row_idx, row_val, ones, s);
        h->create_bytes += (int64_t)h->sides[1].build(n_items, col_ptr, col_idx, col_val, ones, s);
        const int n_max = std::max(n_users, n_items);
        const size_t cap = (size_t)n_max * k;
        h->block[0].alloc_zero(cap, s);
        h->block[1].alloc_zero(cap, s);
        h->num.alloc(cap);
        h->den.alloc(cap);
        h->partial.alloc((size_t)std::max(1, std::max(h->sides[0].n_slots, h->sides[1].n_slots)) * k);
        h->q[0].alloc(std::max<size_t>(nnz, 1));
        h->q[1].alloc(std::max<size_t>(nnz, 1));
        size_t part_cells = 1;
        for (int sd = 0; sd < 2; ++sd) part_cells = std::max(part_cells, h->gram_plan[sd].make(h->rows_of(sd), k));
        h->gram_part.alloc(part_cells);
        for (int sd = 0; sd < 2; ++sd) {
            h->G[sd].alloc((size_t)k * k);
            h->colsum[sd].alloc(k);
        }
        h->Gf.alloc((size_t)k * k);
        h->colsum_f.alloc(k);
        h->colsum_part.alloc((size_t)CS_SLABS * k);
        // workgroup sums: a sweep has one per 256 >> lp_shift rows, an SDDMM one per 256 >> lp_shift pieces
        const int shift = h->lp_shift();
        const int64_t most = std::max<int64_t>(std::max(h->sides[0].n_pieces, h->sides[1].n_pieces), n_max);
        h->red_part.alloc((size_t)std::max<int64_t>(RED_BLOCKS, div_up(most << shift, NT)));
        h->scal.alloc_zero(N_SCALARS, s);
        h->perm.alloc(k);
        h->iota.alloc(n_max);
        iota_enqueue(h->iota.ptr, n_max, s);
        h->dispatch_timers.reserve(8);
        MI_HIP(hipStreamSynchronize(s));
        *out = h.release();
    });
}

extern "C" int mi355rec_nmf_set_block(mi355rec_nmf_t h, int32_t side, const float *X) {
    return guarded([&] {
        require_side(side);
        MI_REQUIRE(h && X, "NULL argument");
        ensure_device();
        const size_t n = (size_t)h->rows_of(side) * h->k;
        MI_HIP(hipMemcpyAsync(h->block[side].ptr, X, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
        MI_HIP(hipStreamSynchronize(h->stream));
        h->prepared_side = -1;
        h->h2d_bytes += (int64_t)(n * sizeof(float));
        ++h->calls;
    });
}

extern "C" int mi355rec_nmf_get_block(mi355rec_nmf_t h, int32_t side, float *X) {
    return guarded([&] {
        require_side(side);
        MI_REQUIRE(h && X, "NULL argument");
        ensure_device();
        const size_t n = (size_t)h->rows_of(side) * h->k;
        MI_HIP(hipMemcpyAsync(X, h->block[side].ptr, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        MI_HIP(hipStreamSynchronize(h->stream));
        h->d2h_bytes += (int64_t)(n * sizeof(float));
        ++h->calls;
    });
}

extern "C" int mi355rec_nmf_fill_block(mi355rec_nmf_t h, int32_t side, float value) {
    return guarded([&] {
        require_side(side);
        MI_REQUIRE(h, "NULL argument");
        MI_REQUIRE(value >= 0.f, "fill value %g is negative", (double)value);
        ensure_device();
        h->start_call();
        const size_t cells = (size_t)h->rows_of(side) * h->k;
        h->begin(PH_SCALE);
        hipLaunchKernelGGL(nmf_fill_kernel, dim3(div_up((int64_t)cells, NT)), dim3(NT), 0, h->stream, h->block[side].ptr, cells, value);
        MI_HIP(hipGetLastError());
        h->end();
        h->launches += 1;
        h->prepared_side = -1;
        h->finish_call(PH_SCALE, 4.0 * cells, 0.0);
    });
}

extern "C" int mi355rec_nmf_cd_sweep(mi355rec_nmf_t h, int32_t side, const int32_t *permutation, int32_t reuse, double *violation) {
    return guarded([&] {
        require_side(side);
        MI_REQUIRE(h && permutation, "NULL argument");
        const int k = h->k;
        std::vector<char> seen(k, 0);
        for (int i = 0; i < k; ++i) {
            const int t = permutation[i];
            MI_REQUIRE(t >= 0 && t < k && !seen[t], "not a permutation of 0 .. %d: entry %d is %d", k - 1, i, t);
            seen[t] = 1;
        }
        MI_REQUIRE(!reuse || (h->prepared_side == side && h->prepared_loss == 0), "reuse: no frobenius products of side %d are held", side);
        ensure_device();
        h->start_call();
        hipStream_t s = h->stream;
        const int n = h->rows_of(side), shift = h->lp_shift(), rows_per_block = NT >> shift;
        MI_HIP(hipMemcpyAsync(h->perm.ptr, permutation, k * sizeof(int), hipMemcpyHostToDevice, s));
        h->h2d_bytes += (int64_t)k * sizeof(int);
        if (!reuse) prepare_frobenius(h, side);
        const int blocks = div_up(n, rows_per_block);
        const size_t lds = (size_t)div_up(k, 1 << shift) * NT * sizeof(float);          // at most 64 KiB (k = 4096), next to 2 KiB of static LDS
        if (lds > 48 * 1024)
            MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(nmf_cd_sweep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        h->begin(PH_SWEEP);
        hipLaunchKernelGGL(nmf_cd_sweep_kernel, dim3(blocks), dim3(NT), lds, s, h->block[side].ptr, n, k, shift, h->Gf.ptr, h->num.ptr,
                           h->perm.ptr, h->red_part.ptr);
        MI_HIP(hipGetLastError());
        h->end();
        h->begin(PH_REDUCE);
        hipLaunchKernelGGL(nmf_sum_kernel, dim3(1), dim3(NT), 0, s, h->red_part.ptr, blocks, h->scal.ptr + SC_VIOLATION, 1);
        MI_HIP(hipGetLastError());
        h->end();
        h->launches += 2;
        if (violation) {
            MI_HIP(hipMemcpyAsync(violation, h->scal.ptr + SC_VIOLATION, sizeof(double), hipMemcpyDeviceToHost, s));
            MI_HIP(hipMemsetAsync(h->scal.ptr + SC_VIOLATION, 0, sizeof(double), s));
            h->d2h_bytes += sizeof(double);
        }
        // the sweep reads a row of HHt per row and step from the cache: its traffic is the block twice and XHt once
        h->finish_call(PH_SWEEP, 12.0 * n * k, 2.0 * (double)n * k * k);
    });
}

extern "C" int mi355rec_nmf_mu_step(mi355rec_nmf_t h, int32_t side, int32_t loss, int32_t reuse) {
    return guarded([&] {
        require_side(side);
        require_loss(loss);
        MI_REQUIRE(h, "NULL argument");
        MI_REQUIRE(!reuse || (h->prepared_side == side && h->prepared_loss == loss), "reuse: nothing of side %d and loss %d is held", side, loss);
        ensure_device();
        h->start_call();
        hipStream_t s = h->stream;
        const int n = h->rows_of(side), k = h->k;
        const size_t cells = (size_t)n * k;
        const int grid = div_up((int64_t)cells, NT);
        if (loss == 0) {
            if (!reuse) prepare_frobenius(h, side);
            h->begin(PH_GEMM);
            gemm_rows_enqueue(h->block[side].ptr, h->iota.ptr, n, k, h->Gf.ptr, k, h->den.ptr, s);       // Gf is symmetric
            h->end();
            h->begin(PH_SCALE);
            hipLaunchKernelGGL(nmf_scale_kernel, dim3(grid), dim3(NT), 0, s, h->block[side].ptr, h->num.ptr, h->den.ptr, (const float *)nullptr,
                               cells, k, EPS32, 0);
            MI_HIP(hipGetLastError());
            h->end();
            h->launches += 2;
            h->finish_call(PH_SCALE, 16.0 * cells, 2.0 * (double)cells * k);
        } else {
            if (!reuse) {
                h->begin(PH_REDUCE);
                enqueue_colsum(h, 1 - side, h->colsum_f.ptr);
                h->end();
                h->prepared_side = side;
                h->prepared_loss = 1;
            }
            int blocks = 0;
            h->begin(PH_SDDMM);
            enqueue_sddmm(h, side, false, blocks);
            h->end();
            h->begin(PH_PRODUCT);
            h->launches += spmm_enqueue(h->sides[side], h->q[side].ptr, h->block[1 - side].ptr, k, h->num.ptr, h->partial.ptr, s);
            h->end();
            h->begin(PH_SCALE);
            // a zero sum of H's rows becomes eps32 under W; a zero sum of W's columns becomes 1 under H, and H is floored at eps64
            hipLaunchKernelGGL(nmf_scale_kernel, dim3(grid), dim3(NT), 0, s, h->block[side].ptr, h->num.ptr, (const float *)nullptr,
                               h->colsum_f.ptr, cells, k, side == 0 ? EPS32 : 1.0f, side == 1 ? 1 : 0);
            MI_HIP(hipGetLastError());
            h->end();
            h->launches += 1;
            h->finish_call(PH_SDDMM, (double)h->nnz * (4.0 * k + 12.0), 2.0 * (double)h->nnz * k);
        }
    });
}

extern "C" int mi355rec_nmf_divergence(mi355rec_nmf_t h, int32_t loss, double *divergence) {
    return guarded([&] {
        require_loss(loss);
        MI_REQUIRE(h && divergence, "NULL argument");
        ensure_device();
        h->start_call();
        hipStream_t s = h->stream;
        const int k = h->k;
        if (loss == 0) {
            h->begin(PH_REDUCE);
            enqueue_gram(h, 0);
            enqueue_gram(h, 1);
            enqueue_dot<double>(h, h->G[0].ptr, h->G[1].ptr, (size_t)k * k, SC_A);
            h->end();
            h->begin(PH_PRODUCT);                      // X H^T into `den`: `num` may hold the products a later step reuses
            h->launches += spmm_enqueue(h->sides[0], h->values(0), h->block[1].ptr, k, h->den.ptr, h->partial.ptr, s);
            h->end();
            h->begin(PH_REDUCE);
            enqueue_dot<float>(h, h->den.ptr, h->block[0].ptr, (size_t)h->n_users * k, SC_B);
            h->end();
        } else {
            int blocks = 0;
            h->begin(PH_SDDMM);
            enqueue_sddmm(h, 0, true, blocks);
            h->end();
            h->begin(PH_REDUCE);
            hipLaunchKernelGGL(nmf_sum_kernel, dim3(1), dim3(NT), 0, s, h->red_part.ptr, blocks, h->scal.ptr + SC_A, 0);
            MI_HIP(hipGetLastError());
            enqueue_colsum(h, 0, nullptr);
            enqueue_colsum(h, 1, nullptr);
            enqueue_dot<double>(h, h->colsum[0].ptr, h->colsum[1].ptr, (size_t)k, SC_B);
            h->end();
            h->launches += 1;
        }
        h->begin(PH_REDUCE);
        hipLaunchKernelGGL(nmf_divergence_kernel, dim3(1), dim3(64), 0, s, h->scal.ptr, loss, h->norm_x, h->sum_x);
        MI_HIP(hipGetLastError());
        h->end();
        h->launches += 1;
        MI_HIP(hipMemcpyAsync(divergence, h->scal.ptr + SC_OUT, sizeof(double), hipMemcpyDeviceToHost, s));
        h->d2h_bytes += sizeof(double);
        h->finish_call(loss == 0 ? PH_PRODUCT : PH_SDDMM, (double)h->nnz * (4.0 * k + 8.0), 2.0 * (double)h->nnz * k);
    });
}

extern "C" int mi355rec_nmf_get_stats(mi355rec_nmf_t h, mi355rec_stats *stats) { return handle_get_stats(h, stats); }

extern "C" int mi355rec_nmf_fit_info(mi355rec_nmf_t h, double *phase_ms, int64_t *launches, int64_t *calls, int64_t *create_bytes,
                                     int64_t *h2d_bytes, int64_t *d2h_bytes, int32_t *all_ones) {
    return guarded([&] {
        MI_REQUIRE(h && phase_ms && launches && calls && create_bytes && h2d_bytes && d2h_bytes && all_ones, "NULL argument");
        for (int p = 0; p < N_PHASES; ++p) phase_ms[p] = h->phase_ms[p];
        *launches = h->launches;
        *calls = h->calls;
        *create_bytes = h->create_bytes;
        *h2d_bytes = h->h2d_bytes;
        *d2h_bytes = h->d2h_bytes;
        *all_ones = h->ones;
    });
}

extern "C" void mi355rec_nmf_destroy(mi355rec_nmf_t h) { handle_destroy(h); }
