// nonpers.hip -- the fits of the reference's non-personalized recommenders on MI355X (gfx950), from the CSR URM_train as it is (no CSC
// copy): TopPop.fit (Base/NonPersonalizedRecommender.py:23-27: stored cells per column) and the three passes of GlobalEffects.fit
// (:71-116: global mean, damped item means of the centred values, damped user means of what is left).
//   The columns come from one stable rocPRIM radix sort of the column ids (with the cell positions along, for GlobalEffects): the
//   cells of column c are then sorted[col_ptr[c] .. col_ptr[c + 1]), col_ptr found by a binary search per column -- no atomics.
//   Element-wise roundings are the reference's (float32 x - mu; float32 (double(d) - item_bias)); every sum is float64 in a fixed
//   order (lane-strided partial sums, one DPP tree): the same bits on every run.
#include "common.h"
#include "wave.cuh"

#include <rocprim/rocprim.hpp>

#include <algorithm>

#pragma clang fp contract(off)

namespace mi355rec {
namespace {

constexpr int SUM_BLOCKS = 256;

// col_ptr[c] = cells with a column id below c, c <= n_cols (the ids are sorted)
__global__ __launch_bounds__(256) void column_bounds_kernel(const uint32_t *sorted, int nnz, int n_cols, int *col_ptr) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c > n_cols) return;
    int lo = 0, hi = nnz;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < (uint32_t)c) lo = mid + 1; else hi = mid;
    }
    col_ptr[c] = lo;
}

__global__ __launch_bounds__(256) void column_counts_kernel(const int *col_ptr, int n_cols, int *counts) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < n_cols) counts[c] = col_ptr[c + 1] - col_ptr[c];
}

__global__ __launch_bounds__(256) void iota_kernel(int *out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = i;
}

// the sum of 256 doubles, one per thread, in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum_256(double v, double *part) {
    part[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    return part[0];
}

__global__ __launch_bounds__(256) void value_partial_kernel(const float *val, int nnz, double *partial) {
    __shared__ double part[256];
    double s = 0.0;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < nnz; q += SUM_BLOCKS * 256) s += (double)val[q];
    const double total = block_sum_256(s, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// mu = float32(sum / nnz) (NonPersonalizedRecommender.py:82)
__global__ __launch_bounds__(256) void mean_kernel(const double *partial, int nnz, float *mu) {
    __shared__ double part[256];
    const double total = block_sum_256(threadIdx.x < SUM_BLOCKS ? partial[threadIdx.x] : 0.0, part);
    if (threadIdx.x == 0) *mu = (float)(total / (double)nnz);
}

// item_bias[c] = sum over the cells of column c of float32(x - mu), / (col_nnz + lambda_item) (:86-96); a wavefront per column
__global__ __launch_bounds__(256) void item_bias_kernel(const int *col_ptr, const int *perm, const float *val, const float *mu_ptr, int n_cols,
                                                        double lambda_item, double *item_bias) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n_cols) return;
    const float mu = *mu_ptr;
    const int a = col_ptr[c], e = col_ptr[c + 1];
    double acc = 0.0;
    for (int t = a + lane; t < e; t += 64) {
        const float d = val[perm[t]] - mu;
        acc += (double)d;
    }
    acc = wave_sum(acc);
    if (lane == 0) item_bias[c] = acc / ((double)(e - a) + lambda_item);
}

// user_bias[r] = sum over the cells of row r of float32(double(float32(x - mu)) - item_bias[col]), / (row_nnz + lambda_user) (:104-110)
__global__ __launch_bounds__(256) void user_bias_kernel(const int *ptr, const int *idx, const float *val, const float *mu_ptr,
                                                        const double *item_bias, int n_rows, double lambda_user, double *user_bias) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const float mu = *mu_ptr;
    const int a = ptr[r], e = ptr[r + 1];
    double acc = 0.0;
    for (int q = a + lane; q < e; q += 64) {
        const float d = val[q] - mu;
        const float left = (float)((double)d - item_bias[idx[q]]);
        acc += (double)left;
    }
    acc = wave_sum(acc);
    if (lane == 0) user_bias[r] = acc / ((double)(e - a) + lambda_user);
}

int id_bits(int n_cols) {
    int bits = 1;
    while (bits < 32 && (1ll << bits) < (long long)n_cols) ++bits;
    return bits;
}

// a CSR matrix in device memory: the caller's arrays (resident) or copies that live as long as this object
struct DeviceCsr {
    DeviceBuffer<int> own_ptr, own_idx;
    DeviceBuffer<float> own_val;
    const int *ptr = nullptr, *idx = nullptr;
    const float *val = nullptr;
    int n_rows = 0, n_cols = 0, nnz = 0;

    void from_host(int rows, int cols, const int32_t *indptr, const int32_t *indices, const float *data, hipStream_t s) {
        MI_REQUIRE(indptr && indptr[0] == 0, "indptr must start at 0");
        for (int r = 0; r < rows; ++r) MI_REQUIRE(indptr[r] <= indptr[r + 1], "indptr is not monotone");
        n_rows = rows; n_cols = cols; nnz = indptr[rows];
        MI_REQUIRE(indices || nnz == 0, "NULL argument");
        for (int q = 0; q < nnz; ++q) MI_REQUIRE(indices[q] >= 0 && indices[q] < cols, "column id %d outside [0, %d)", indices[q], cols);
        own_ptr.upload(indptr, (size_t)rows + 1, s);
        own_idx.upload(indices, (size_t)nnz, s);
        if (data) own_val.upload(data, (size_t)nnz, s);
        ptr = own_ptr.ptr; idx = own_idx.ptr; val = own_val.ptr;
    }
    void resident(int rows, int cols, int cells, const int32_t *d_indptr, const int32_t *d_indices, const float *d_data) {
        MI_REQUIRE(d_indptr && (d_indices || cells == 0), "NULL argument");
        MI_REQUIRE(cells >= 0, "%d stored cells", cells);
        n_rows = rows; n_cols = cols; nnz = cells;
        ptr = d_indptr; idx = d_indices; val = d_data;
    }
};

struct PooledStream {
    hipStream_t s;
    PooledStream() : s(pooled_stream()) {}
    ~PooledStream() {
        (void)hipStreamSynchronize(s);
        pooled_stream_return(s);
    }
};

// the columns of the matrix: col_ptr[n_cols + 1] and -- with_perm -- perm[t] = the CSR position of the t-th cell in column order
// (rows ascending inside a column: the sort is stable)
struct Columns {
    DeviceBuffer<uint32_t> sorted;
    DeviceBuffer<int> iota, perm, col_ptr;
    DeviceBuffer<unsigned char> tmp;

    void build(const DeviceCsr &m, bool with_perm, hipStream_t s) {
        const uint32_t *ids = reinterpret_cast<const uint32_t *>(m.idx);
        const int bits = id_bits(m.n_cols);
        col_ptr.alloc((size_t)m.n_cols + 1);
        if (m.nnz) {
            sorted.alloc(m.nnz);
            size_t bytes = 0;
            if (with_perm) {
                iota.alloc(m.nnz); perm.alloc(m.nnz);
                hipLaunchKernelGGL(iota_kernel, dim3(div_up(m.nnz, 256)), dim3(256), 0, s, iota.ptr, m.nnz);
                MI_HIP(rocprim::radix_sort_pairs(nullptr, bytes, ids, sorted.ptr, iota.ptr, perm.ptr, (size_t)m.nnz, 0, bits, s));
                tmp.alloc(bytes + 256);
                bytes = tmp.count;
                MI_HIP(rocprim::radix_sort_pairs(tmp.ptr, bytes, ids, sorted.ptr, iota.ptr, perm.ptr, (size_t)m.nnz, 0, bits, s));
            } else {
                MI_HIP(rocprim::radix_sort_keys(nullptr, bytes, ids, sorted.ptr, (size_t)m.nnz, 0, bits, s));
                tmp.alloc(bytes + 256);
                bytes = tmp.count;
                MI_HIP(rocprim::radix_sort_keys(tmp.ptr, bytes, ids, sorted.ptr, (size_t)m.nnz, 0, bits, s));
            }
        }
        hipLaunchKernelGGL(column_bounds_kernel, dim3(div_up(m.n_cols + 1, 256)), dim3(256), 0, s, sorted.ptr, m.nnz, m.n_cols, col_ptr.ptr);
        MI_HIP(hipGetLastError());
    }
};

void item_counts(const DeviceCsr &m, hipStream_t s, int32_t *counts_host) {
    Columns cols;
    cols.build(m, false, s);
    DeviceBuffer<int> counts;
    counts.alloc(m.n_cols);
    hipLaunchKernelGGL(column_counts_kernel, dim3(div_up(m.n_cols, 256)), dim3(256), 0, s, cols.col_ptr.ptr, m.n_cols, counts.ptr);
    MI_HIP(hipGetLastError());
    int last = 0;
    counts.download(counts_host, m.n_cols, s);
    MI_HIP(hipMemcpyAsync(&last, cols.col_ptr.ptr + m.n_cols, sizeof(int), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    // (only a resident matrix can get here with one; the sort looks at the low bits of an id, so this catches ids up to the next
    // power of two -- a resident matrix is otherwise trusted, as the similarity builds trust it)
    MI_REQUIRE(last == m.nnz, "a stored column id is outside [0, %d)", m.n_cols);
}

void global_effects(const DeviceCsr &m, hipStream_t s, double lambda_user, double lambda_item, float *mu_host, double *item_bias_host,
                    double *user_bias_host) {
    MI_REQUIRE(m.nnz > 0 && m.val, "GlobalEffects needs at least one stored value");
    Columns cols;
    cols.build(m, true, s);
    int last = 0;
    MI_HIP(hipMemcpyAsync(&last, cols.col_ptr.ptr + m.n_cols, sizeof(int), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    MI_REQUIRE(last == m.nnz, "a stored column id is outside [0, %d)", m.n_cols);     // (before item_bias is indexed by one)
    DeviceBuffer<double> partial, item_bias, user_bias;
    DeviceBuffer<float> mu;
    partial.alloc(SUM_BLOCKS); item_bias.alloc(m.n_cols); user_bias.alloc(m.n_rows); mu.alloc(1);
    hipLaunchKernelGGL(value_partial_kernel, dim3(SUM_BLOCKS), dim3(256), 0, s, m.val, m.nnz, partial.ptr);
    hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, partial.ptr, m.nnz, mu.ptr);
    hipLaunchKernelGGL(item_bias_kernel, dim3(div_up(m.n_cols, 4)), dim3(256), 0, s, cols.col_ptr.ptr, cols.perm.ptr, m.val, mu.ptr, m.n_cols,
                       lambda_item, item_bias.ptr);
    hipLaunchKernelGGL(user_bias_kernel, dim3(div_up(m.n_rows, 4)), dim3(256), 0, s, m.ptr, m.idx, m.val, mu.ptr, item_bias.ptr, m.n_rows,
                       lambda_user, user_bias.ptr);
    MI_HIP(hipGetLastError());
    mu.download(mu_host, 1, s);
    item_bias.download(item_bias_host, m.n_cols, s);
    user_bias.download(user_bias_host, m.n_rows, s);
    MI_HIP(hipStreamSynchronize(s));
}

}  // namespace
}  // namespace mi355rec

using namespace mi355rec;

extern "C" int mi355rec_urm_item_counts(int32_t n_users, int32_t n_items, const int32_t *indptr, const int32_t *indices, int32_t *item_counts_out) {
    return guarded([&] {
        MI_REQUIRE(item_counts_out && n_users > 0 && n_items > 0, "NULL argument or empty matrix");
        ensure_device();
        PooledStream st;
        ReleaseScope scope(st.s);
        DeviceCsr m;
        m.from_host(n_users, n_items, indptr, indices, nullptr, st.s);
        item_counts(m, st.s, item_counts_out);
    });
}

extern "C" int mi355rec_urm_item_counts_resident(int32_t n_users, int32_t n_items, int32_t nnz, const int32_t *d_indptr, const int32_t *d_indices,
                                                 int32_t *item_counts_out) {
    return guarded([&] {
        MI_REQUIRE(item_counts_out && n_users > 0 && n_items > 0, "NULL argument or empty matrix");
        ensure_device();
        PooledStream st;
        ReleaseScope scope(st.s);
        DeviceCsr m;
        m.resident(n_users, n_items, nnz, d_indptr, d_indices, nullptr);
        item_counts(m, st.s, item_counts_out);
    });
}

extern "C" int mi355rec_urm_global_effects(int32_t n_users, int32_t n_items, const int32_t *indptr, const int32_t *indices, const float *data,
                                           double lambda_user, double lambda_item, float *mu, double *item_bias, double *user_bias) {
    return guarded([&] {
        MI_REQUIRE(data && mu && item_bias && user_bias && n_users > 0 && n_items > 0, "NULL argument or empty matrix");
        ensure_device();
        PooledStream st;
        ReleaseScope scope(st.s);
        DeviceCsr m;
        m.from_host(n_users, n_items, indptr, indices, data, st.s);
        global_effects(m, st.s, lambda_user, lambda_item, mu, item_bias, user_bias);
    });
}

extern "C" int mi355rec_urm_global_effects_resident(int32_t n_users, int32_t n_items, int32_t nnz, const int32_t *d_indptr,
                                                    const int32_t *d_indices, const float *d_data, double lambda_user, double lambda_item,
                                                    float *mu, double *item_bias, double *user_bias) {
    return guarded([&] {
        MI_REQUIRE(d_data && mu && item_bias && user_bias && n_users > 0 && n_items > 0, "NULL argument or empty matrix");
        ensure_device();
        PooledStream st;
        ReleaseScope scope(st.s);
        DeviceCsr m;
        m.resident(n_users, n_items, nnz, d_indptr, d_indices, d_data);
        global_effects(m, st.s, lambda_user, lambda_item, mu, item_bias, user_bias);
    });
}
