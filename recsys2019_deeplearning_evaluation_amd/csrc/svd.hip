// svd.hip -- the device half of PureSVD's randomized SVD on MI355X (gfx950)  [DESIGN.md section 11].
//
// The reference (MatrixFactorization/PureSVDRecommender.py:34-47) calls sklearn's randomized_svd: sixteen products of the URM or
// its transpose with a tall, thin dense block, a normalisation of the block after each, and a small dense SVD.  The handle keeps
// the URM in both layouts and one block per side (users x r, items x r) resident; the loop is driven from Python through the
// step-wise entry points below, because the r x r factorisations (Cholesky, eigh) belong to LAPACK on the host.
//
//   svd_spmm_kernel     Y[row] = sum_j val[j] * X[idx[j]]: a row is cut into PIECES of at most SPLIT nonzeros, one piece per group of
//                       16 / 32 / 64 lanes (chosen from r, so that short blocks pack 4 or 2 pieces into a wavefront); a lane owns up to
//                       CPL columns lp apart per pass over the piece and sums them in nonzero order.  One-piece rows write Y
//                       directly, pieces of longer rows write a partial row that svd_long_rows_kernel adds in piece order: no
//                       atomics, a product is bitwise repeatable.  All-ones URMs skip the value stream.
//   svd_gram_kernel     G = X^T X in float64 FMAs: 64 x 64 tiles of the upper triangle, a slab of rows per workgroup, the slabs'
//                       partial tiles added in slab order by svd_gram_reduce_kernel (which mirrors the lower triangle).
//   block * matrix      X <- X T is score.hip's f32 MFMA GEMM (gemm_rows_enqueue) with the identity as its row gather.
// The product and the Gram build are also launchers on a caller's stream (svd_product.h): the NMF handle (nmf.hip) runs the same kernels.
#include "common.h"
#include "score.h"
#include "svd_product.h"

#include <algorithm>
#include <memory>

using namespace mi355rec;

namespace {

constexpr int SPLIT = 512;        // nonzeros of the longest piece
constexpr int CPL = 4;            // columns a lane owns per pass over its piece
constexpr int SPMM_THREADS = 256;
constexpr int GT = 64;            // side of a Gram tile
constexpr int GR = 16;            // block rows staged per step of the Gram kernel

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

// ---- what nmf.hip shares (svd_product.h) ----------------------------------------------------------------------------------------
namespace mi355rec {

// the kernel gathers block rows by the indices of a layout: pointers that decrease or an index outside the other side are refused
void validate_layout(int n, int n_other, const int *ptr, const int *idx) {
    MI_REQUIRE(ptr[0] == 0, "row pointers do not start at 0");
    for (int i = 0; i < n; ++i) MI_REQUIRE(ptr[i] <= ptr[i + 1], "row pointers decrease at %d", i);
    for (int j = 0, e = ptr[n]; j < e; ++j) MI_REQUIRE(idx[j] >= 0 && idx[j] < n_other, "index %d outside [0, %d)", idx[j], n_other);
}

size_t Side::build(int n, const int *row_ptr, const int *row_idx, const float *row_val, bool ones, hipStream_t s) {
    n_rows = n;
    std::vector<int> row, begin, end, slot, lrow, lfirst, lcount;
    row.reserve(n);
    for (int i = 0; i < n; ++i) {
        const int b = row_ptr[i], e = row_ptr[i + 1], len = e - b;
        const int parts = std::max(1, div_up(len, SPLIT));
        if (parts > 1) {
            lrow.push_back(i);
            lfirst.push_back(n_slots);
            lcount.push_back(parts);
        }
        for (int p = 0; p < parts; ++p) {
            row.push_back(i);
            begin.push_back(b + p * SPLIT);
            end.push_back(std::min(e, b + (p + 1) * SPLIT));
            slot.push_back(parts > 1 ? n_slots++ : -1);
        }
    }
    n_pieces = (int)row.size();
    n_long = (int)lrow.size();
    const size_t nnz = (size_t)row_ptr[n];
    idx.alloc(std::max<size_t>(nnz, 1));
    if (nnz) MI_HIP(hipMemcpyAsync(idx.ptr, row_idx, nnz * sizeof(int), hipMemcpyHostToDevice, s));
    if (!ones) {
        val.alloc(std::max<size_t>(nnz, 1));
        if (nnz) MI_HIP(hipMemcpyAsync(val.ptr, row_val, nnz * sizeof(float), hipMemcpyHostToDevice, s));
    }
    p_row.upload(row.data(), row.size(), s);
    p_begin.upload(begin.data(), begin.size(), s);
    p_end.upload(end.data(), end.size(), s);
    p_slot.upload(slot.data(), slot.size(), s);
    if (n_long) {
        l_row.upload(lrow.data(), lrow.size(), s);
        l_first.upload(lfirst.data(), lfirst.size(), s);
        l_count.upload(lcount.data(), lcount.size(), s);
    }
    MI_HIP(hipStreamSynchronize(s));              // the vectors above go out of scope
    return 4 * (nnz * (ones ? 1 : 2) + 4 * row.size() + 3 * lrow.size());
}

int spmm_enqueue(const Side &sd, const float *val, const float *X, int r, float *Y, float *partial, hipStream_t s) {
    const int lp_shift = r <= 16 ? 4 : (r <= 32 ? 5 : 6);
    const int grid = div_up((int64_t)sd.n_pieces << lp_shift, SPMM_THREADS);
    if (!val)
        hipLaunchKernelGGL(svd_spmm_kernel<true>, dim3(grid), dim3(SPMM_THREADS), 0, s, sd.p_row.ptr, sd.p_begin.ptr, sd.p_end.ptr,
                           sd.p_slot.ptr, sd.n_pieces, sd.idx.ptr, (const float *)nullptr, X, r, lp_shift, Y, partial);
    else
        hipLaunchKernelGGL(svd_spmm_kernel<false>, dim3(grid), dim3(SPMM_THREADS), 0, s, sd.p_row.ptr, sd.p_begin.ptr, sd.p_end.ptr,
                           sd.p_slot.ptr, sd.n_pieces, sd.idx.ptr, val, X, r, lp_shift, Y, partial);
    MI_HIP(hipGetLastError());
    if (sd.n_long) {
        hipLaunchKernelGGL(svd_long_rows_kernel, dim3(sd.n_long), dim3(256), 0, s, sd.l_row.ptr, sd.l_first.ptr, sd.l_count.ptr, partial, r, Y);
        MI_HIP(hipGetLastError());
    }
    return sd.n_long ? 2 : 1;
}

size_t GramPlan::make(int n, int r) {
    const int nt = div_up(r, GT), pairs = nt * (nt + 1) / 2;
    slabs = std::max(1, std::min(div_up(n, 4 * GR), 1024 / pairs));
    rows = div_up(div_up(n, slabs), GR) * GR;
    slabs = div_up(n, rows);
    return (size_t)slabs * r * r;
}

void gram_enqueue(const float *X, int n, int r, const GramPlan &plan, double *part, double *G, hipStream_t s) {
    const int nt = div_up(r, GT);
    hipLaunchKernelGGL(svd_gram_kernel, dim3(nt, nt, plan.slabs), dim3(256), 0, s, X, n, r, plan.rows, part);
    MI_HIP(hipGetLastError());
    hipLaunchKernelGGL(svd_gram_reduce_kernel, dim3(div_up((int64_t)r * r, 256)), dim3(256), 0, s, part, plan.slabs, r, G);
    MI_HIP(hipGetLastError());
}

void iota_enqueue(int *out, int n, hipStream_t s) {
    hipLaunchKernelGGL(svd_iota_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, out, n);
    MI_HIP(hipGetLastError());
}

}  // namespace mi355rec

struct mi355rec_svd : Handle {
    int n_users = 0, n_items = 0, r = 0, ones = 0;
    size_t nnz = 0;
    Side sides[2];                                     // [0]: rows = users (the CSR layout), [1]: rows = items (the CSC layout)
    DeviceBuffer<float> block[2], tmp, partial, T;
    DeviceBuffer<double> gram_part, G;
    DeviceBuffer<int> iota;
    GramPlan gram_plan[2];
    double phase_ms[3] = {0, 0, 0};                   // products, Gram, apply
    int64_t launches = 0, calls = 0, create_bytes = 0, h2d_bytes = 0, d2h_bytes = 0;

    int rows_of(int s) const { return s == 0 ? n_users : n_items; }

    ~mi355rec_svd() { shutdown(); }
};

extern "C" int mi355rec_svd_create(mi355rec_svd_t *out, int32_t n_users, int32_t n_items, int32_t r, const int32_t *row_ptr,
                                   const int32_t *row_idx, const float *row_val, const int32_t *col_ptr, const int32_t *col_idx,
                                   const float *col_val) {
    return guarded([&] {
        MI_REQUIRE(out && row_ptr && col_ptr, "NULL argument");
        MI_REQUIRE(n_users > 0 && n_items > 0, "empty URM (%d x %d)", n_users, n_items);
        MI_REQUIRE(r >= 1 && r <= 4096, "block width r = %d outside [1, 4096]", r);
        MI_REQUIRE(row_ptr[n_users] == col_ptr[n_items], "the two layouts hold %d and %d cells", row_ptr[n_users], col_ptr[n_items]);
        const size_t nnz = (size_t)row_ptr[n_users];
        MI_REQUIRE(nnz == 0 || (row_idx && col_idx && row_val && col_val), "NULL argument");
        MI_REQUIRE(div_up(std::max(n_users, n_items), 128) <= 65535, "more than 8 M rows on a side");
        validate_layout(n_users, n_items, row_ptr, row_idx);
        validate_layout(n_items, n_users, col_ptr, col_idx);
        *out = nullptr;
        auto h = open_handle<mi355rec_svd>(1);
        h->n_users = n_users;
        h->n_items = n_items;
        h->r = r;
        h->nnz = nnz;
        bool ones = true;
        for (size_t i = 0; i < nnz && ones; ++i) ones = row_val[i] == 1.0f;
        h->ones = ones ? 1 : 0;
        ReleaseScope scope(h->stream);
        hipStream_t s = h->stream;
        h->create_bytes += (int64_t)h->sides[0].build(n_users, row_ptr, row_idx, row_val, ones, s);
        h->create_bytes += (int64_t)h->sides[1].build(n_items, col_ptr, col_idx, col_val, ones, s);
        const size_t cap = (size_t)std::max(n_users, n_items) * r;
        h->block[0].alloc_zero(cap, s);
        h->block[1].alloc_zero(cap, s);
        h->tmp.alloc(cap);
        h->partial.alloc((size_t)std::max(1, std::max(h->sides[0].n_slots, h->sides[1].n_slots)) * r);
        size_t part_cells = 1;
        for (int sd = 0; sd < 2; ++sd) part_cells = std::max(part_cells, h->gram_plan[sd].make(h->rows_of(sd), r));
        h->gram_part.alloc(part_cells);
        h->G.alloc((size_t)r * r);
        h->T.alloc((size_t)r * r);
        const int n_max = std::max(n_users, n_items);
        h->iota.alloc(n_max);
        iota_enqueue(h->iota.ptr, n_max, s);
        MI_HIP(hipStreamSynchronize(s));
        *out = h.release();
    });
}

extern "C" int mi355rec_svd_set_block(mi355rec_svd_t h, int32_t side, const float *X) {
    return guarded([&] {
        MI_REQUIRE(h && X, "NULL argument");
        MI_REQUIRE(side == 0 || side == 1, "side %d: 0 (users x r) or 1 (items x r)", side);
        ensure_device();
        const size_t n = (size_t)h->rows_of(side) * h->r;
        MI_HIP(hipMemcpyAsync(h->block[side].ptr, X, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
        MI_HIP(hipStreamSynchronize(h->stream));
        h->h2d_bytes += (int64_t)(n * sizeof(float));
        ++h->calls;
    });
}

extern "C" int mi355rec_svd_get_block(mi355rec_svd_t h, int32_t side, float *X) {
    return guarded([&] {
        MI_REQUIRE(h && X, "NULL argument");
        MI_REQUIRE(side == 0 || side == 1, "side %d: 0 (users x r) or 1 (items x r)", side);
        ensure_device();
        const size_t n = (size_t)h->rows_of(side) * h->r;
        MI_HIP(hipMemcpyAsync(X, h->block[side].ptr, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        MI_HIP(hipStreamSynchronize(h->stream));
        h->d2h_bytes += (int64_t)(n * sizeof(float));
        ++h->calls;
    });
}

extern "C" int mi355rec_svd_product(mi355rec_svd_t h, int32_t dst_side) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL argument");
        MI_REQUIRE(dst_side == 0 || dst_side == 1, "side %d: 0 (users = URM . items) or 1 (items = URM^T . users)", dst_side);
        ensure_device();
        hipStream_t s = h->stream;
        const Side &sd = h->sides[dst_side];
        const int r = h->r;
        const float *X = h->block[1 - dst_side].ptr;
        float *Y = h->block[dst_side].ptr;
        h->timer.start(s);
        const int launched = spmm_enqueue(sd, h->ones ? nullptr : sd.val.ptr, X, r, Y, h->partial.ptr, s);
        h->timer.stop(s);
        MI_HIP(hipStreamSynchronize(s));
        const double ms = h->timer.elapsed_ms();
        h->phase_ms[0] += ms;
        h->launches += launched;
        ++h->calls;
        h->stats = mi355rec_stats{};
        h->stats.call_ms = h->stats.kernel_ms = ms;
        h->stats.n_launches = h->stats.n_timed = 1;
        h->stats.n_units = (int64_t)h->nnz;
        h->stats.algorithmic_bytes = (double)h->nnz * (4.0 * r + 8.0);      // a gathered row of the block, an index and a value per cell
        h->stats.algorithmic_flops = 2.0 * (double)h->nnz * r;
    });
}

extern "C" int mi355rec_svd_gram(mi355rec_svd_t h, int32_t side, double *G) {
    return guarded([&] {
        MI_REQUIRE(h && G, "NULL argument");
        MI_REQUIRE(side == 0 || side == 1, "side %d: 0 (users x r) or 1 (items x r)", side);
        ensure_device();
        hipStream_t s = h->stream;
        const int r = h->r, n = h->rows_of(side);
        h->timer.start(s);
        gram_enqueue(h->block[side].ptr, n, r, h->gram_plan[side], h->gram_part.ptr, h->G.ptr, s);
        h->timer.stop(s);
        h->G.download(G, (size_t)r * r, s);
        MI_HIP(hipStreamSynchronize(s));
        h->phase_ms[1] += h->timer.elapsed_ms();
        h->launches += 2;
        h->d2h_bytes += (int64_t)r * r * sizeof(double);
        ++h->calls;
    });
}

extern "C" int mi355rec_svd_apply(mi355rec_svd_t h, int32_t side, const float *T) {
    return guarded([&] {
        MI_REQUIRE(h && T, "NULL argument");
        MI_REQUIRE(side == 0 || side == 1, "side %d: 0 (users x r) or 1 (items x r)", side);
        ensure_device();
        hipStream_t s = h->stream;
        const int r = h->r, n = h->rows_of(side);
        std::vector<float> Tt((size_t)r * r);          // the GEMM multiplies by the rows of its second operand
        for (int i = 0; i < r; ++i)
            for (int j = 0; j < r; ++j) Tt[(size_t)j * r + i] = T[(size_t)i * r + j];
        MI_HIP(hipMemcpyAsync(h->T.ptr, Tt.data(), Tt.size() * sizeof(float), hipMemcpyHostToDevice, s));
        h->timer.start(s);
        gemm_rows_enqueue(h->block[side].ptr, h->iota.ptr, n, r, h->T.ptr, r, h->tmp.ptr, s);
        h->timer.stop(s);
        MI_HIP(hipStreamSynchronize(s));
        h->block[side].swap(h->tmp);
        h->phase_ms[2] += h->timer.elapsed_ms();
        h->launches += 1;
        h->h2d_bytes += (int64_t)r * r * sizeof(float);
        ++h->calls;
    });
}

extern "C" int mi355rec_svd_get_stats(mi355rec_svd_t h, mi355rec_stats *stats) { return handle_get_stats(h, stats); }

extern "C" int mi355rec_svd_fit_info(mi355rec_svd_t h, double *product_ms, double *gram_ms, double *apply_ms, int64_t *launches,
                                     int64_t *calls, int64_t *create_bytes, int64_t *h2d_bytes, int64_t *d2h_bytes, int32_t *all_ones) {
    return guarded([&] {
        MI_REQUIRE(h && product_ms && gram_ms && apply_ms && launches && calls && create_bytes && h2d_bytes && d2h_bytes && all_ones,
                   "NULL argument");
        *product_ms = h->phase_ms[0];
        *gram_ms = h->phase_ms[1];
        *apply_ms = h->phase_ms[2];
        *launches = h->launches;
        *calls = h->calls;
        *create_bytes = h->create_bytes;
        *h2d_bytes = h->h2d_bytes;
        *d2h_bytes = h->d2h_bytes;
        *all_ones = h->ones;
    });
}

extern "C" void mi355rec_svd_destroy(mi355rec_svd_t h) { handle_destroy(h); }
