// sim_setup.cuh -- the kernels of the Compute_Similarity constructor (value scan, feature weighting, centring, CSR -> CSC, column
// costs and norms, profile stream, walk lists) and the small kernels behind its CSR / dense outputs.  Included by sim.hip after
// sim_kernels.cuh.
#pragma once

namespace mi355rec {
namespace {

// ---------------------------------------- set-up kernels -------------------------------------------

// One pass over the stored values: out[0] bit s SET when some value times 2^s (s = 0..3) is not an integer, out[1] the bits of
// max |value|, out[2] non-zero when some value is not exactly 1.
__global__ void value_scan_kernel(const float *x, size_t n, unsigned *out) {
    unsigned bad = 0, top = 0, not_unit = 0;
    auto look = [&](float v) {
        top = max(top, __float_as_uint(fabsf(v)));
        not_unit |= v != 1.0f;
#pragma unroll
        for (int sh = 0; sh <= 3; ++sh) {
            const float t = v * (float)(1 << sh);
            if (!(t == rintf(t))) bad |= 1u << sh;       // (NaN / inf never qualify)
        }
    };
    // (16 bytes per load: with one float per thread and step the scan of 80 MB took 0.2 ms -- a tenth of the HBM rate)
    const size_t n4 = n / 4, stride = (size_t)gridDim.x * blockDim.x;
    const float4 *x4 = reinterpret_cast<const float4 *>(x);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 v = x4[i];
        look(v.x); look(v.y); look(v.z); look(v.w);
    }
    for (size_t i = 4 * n4 + blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += stride) look(x[i]);
    // one atomic per wavefront and word (a million threads on one address each cost 0.15 ms)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        bad |= (unsigned)__shfl_xor((int)bad, off);
        top = max(top, (unsigned)__shfl_xor((int)top, off));
        not_unit |= (unsigned)__shfl_xor((int)not_unit, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicOr(&out[0], bad);
        if (top) atomicMax(&out[1], top);
        if (not_unit) atomicOr(&out[2], 1u);
    }
}

__global__ void fill_kernel(float *x, size_t n, float v) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) x[i] = v;
}

// NumPy's float32 pairwise summation (numpy/_core/src/umath/loops_utils.h, FLOAT_pairwise_sum): < 8 elements
// sequentially, <= 128 with eight running partial sums, above that split in halves (rounded to a multiple of 8).
__device__ float numpy_pairwise_sum(const float *a, int n) {
    if (n < 8) {
        float r = 0.f;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        float r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
        int i = 8;
        for (; i < n - (n % 8); i += 8) {
            r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
            r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
        }
        float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return numpy_pairwise_sum(a, n2) + numpy_pairwise_sum(a + n2, n - n2);
}

// Mean of the stored cells of every segment (CSR row or CSC column).  Mean-centred data is a difference of nearly
// equal numbers, so the float32 rounding of the SUM is visible in the result: the reference's
// `dataMatrix.sum(axis=...)` on a float32 matrix is np.add.reduceat(data, indptr), i.e. first element + NumPy's
// pairwise sum of the rest, in float32 -- reproduced bit for bit (checked against SciPy on the CPU).
__global__ void segment_mean_kernel(const int *ptr, const float *val, int n_segments, float *mean) {
    const int sgm = blockIdx.x * blockDim.x + threadIdx.x;
    if (sgm >= n_segments) return;
    const int s = ptr[sgm], e = ptr[sgm + 1];
    float sum = 0.f;
    if (e > s) sum = e - s > 1 ? val[s] + numpy_pairwise_sum(val + s + 1, e - s - 1) : val[s];
    mean[sgm] = e > s ? (float)((double)sum / (double)(e - s)) : 0.f;
}

// applyAdjustedCosine (.pyx:275-310): subtract from every stored cell the mean of its row.
__global__ void row_center_kernel(const int *ptr, float *val, int n_rows, const float *mean) {
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= n_rows) return;
    const float m = mean[wave];
    for (int q = ptr[wave] + lane; q < ptr[wave + 1]; q += 64) val[q] -= m;
}

// Padded length (multiple of 8 entries) of every (row, accumulator tile) segment; slot n_seg gets 0 so that the
// exclusive scan over n_seg + 1 slots ends with the total.
__global__ void seg_len_kernel(const int *csr_ptr, const int *row_tile_ptr, int n_rows, int n_tiles, int *len_pad) {
    const long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long n_seg = (long long)n_rows * n_tiles;
    if (k > n_seg) return;
    int len = 0;
    if (k < n_seg) {
        const int u = (int)(k / n_tiles), t = (int)(k % n_tiles);
        if (n_tiles == 1) len = csr_ptr[u + 1] - csr_ptr[u];
        else len = row_tile_ptr[(size_t)u * (n_tiles + 1) + t + 1] - row_tile_ptr[(size_t)u * (n_tiles + 1) + t];
    }
    len_pad[k] = (len + 7) & ~7;
}

// The profile stream of the column kernel (one wavefront per segment): ids relative to the tile base as uint16,
// values as they are after pre-processing; padding entries point at the 4 spare accumulator cells and carry 0.
__global__ void seg_fill_kernel(const int *csr_ptr, const int *row_tile_ptr, const int *csr_idx, const float *csr_val,
                                const int *seg_ptr, int n_rows, int n_tiles, int tile_w, unsigned short *seg_idx16,
                                float *seg_val, int group_lanes, short *seg_val16, float int_half) {
    const long long k = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (k >= (long long)n_rows * n_tiles) return;
    const int u = (int)(k / n_tiles), t = (int)(k % n_tiles);
    int a, b;
    if (n_tiles == 1) {
        a = csr_ptr[u];
        b = csr_ptr[u + 1];
    } else {
        a = row_tile_ptr[(size_t)u * (n_tiles + 1) + t];
        b = row_tile_ptr[(size_t)u * (n_tiles + 1) + t + 1];
    }
    const int dst = seg_ptr[k], padded = seg_ptr[k + 1] - dst, len = b - a;
    // Lane-interleaved order inside every FULL block of 8 G entries (G = lanes per profile in the column kernel, 0 = off): the
    // kernel's lane g loads the 16-byte chunk g of a block and its e-th ds_add takes the chunk's entry e, so with the entries
    // stored in row order one instruction carries entries g * 8 + e -- ids at stride 8 of a sorted profile, and where a long
    // profile is dense (the popular items of a heavy user: ids nearly consecutive) that is 4 distinct LDS banks for 32 lanes.
    // Stored as chunk g = entries {g, g + G, g + 2 G, ...}, one instruction carries G CONSECUTIVE entries of the profile: consecutive
    // ids, distinct banks.  The kernel does not care in which order a segment's entries arrive; the tail of a segment (less than a
    // block) stays in row order, so the chunk-granular end-of-segment test still holds.  Measured at ML-20M shape: accumulation
    // 659 -> 640 workgroup-ms, kernel 4.02 -> 3.98 ms (the atomic unit itself, not the bank pattern, is what bounds the scatter).
    // One lane per 16-byte chunk of the stream (8 entries): the row-order entries first, first + step, ... are read (neighbouring
    // lanes on neighbouring entries inside a block), packed and stored as ONE aligned 16-byte word per lane -- 2-byte stores
    // at a stride of 16 bytes took 0.18 ms for the 40 MB of ids.  The counts kernel never reads values: none are written for it.
    const int block = 8 * group_lanes, n_blocked = block > 0 ? (padded / block) * block : 0;
    const int n_chunks = padded >> 3, tile_base = t * tile_w;
    uint4 *idx_out = reinterpret_cast<uint4 *>(seg_idx16 + dst);
    for (int c = lane; c < n_chunks; c += 64) {
        int first = c * 8, step = 1;
        if (first < n_blocked) {
            const int blk = c / group_lanes;
            first = blk * block + (c - blk * group_lanes);
            step = group_lanes;
        }
        unsigned id[8];
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int q = first + e * step;
            const bool real = q < len;
            id[e] = (unsigned)(real ? csr_idx[a + q] - tile_base : tile_w + (q & 3)) & 0xFFFFu;
            v[e] = (real && (seg_val || seg_val16)) ? csr_val[a + q] : 0.f;
        }
        idx_out[c] = make_uint4(id[0] | (id[1] << 16), id[2] | (id[3] << 16), id[4] | (id[5] << 16), id[6] | (id[7] << 16));
        if (seg_val16) {
            unsigned h[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = (unsigned)__float2int_rn(v[e] * int_half) & 0xFFFFu;     // exact: the value grid was checked
            reinterpret_cast<uint4 *>(seg_val16 + dst)[c] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
        } else if (seg_val) {
            float4 *val_out = reinterpret_cast<float4 *>(seg_val + dst);
            val_out[2 * c] = make_float4(v[0], v[1], v[2], v[3]);
            val_out[2 * c + 1] = make_float4(v[4], v[5], v[6], v[7]);
        }
    }
}

// row_tile_ptr[u][t] = first position of CSR row u whose column id is >= t * tile_w (rows have sorted ids).
__global__ void row_tile_ptr_kernel(const int *ptr, const int *idx, int n_rows, int tile_w, int n_tiles, int *out) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= (long long)n_rows * (n_tiles + 1)) return;
    const int u = (int)(e / (n_tiles + 1)), t = (int)(e % (n_tiles + 1));
    int lo = ptr[u], hi = ptr[u + 1];
    const long long bound = (long long)t * tile_w;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (idx[mid] < bound) lo = mid + 1; else hi = mid;
    }
    out[e] = lo;
}

// CSC column pointers from the column keys sorted by the radix sort: csc_ptr[c] = first position whose key is >= c
// (one thread per column, binary search; a histogram with global atomics took 2.6 ms at ML-20M shape -- the head
// columns serialise on their counters).
__global__ void csc_ptr_kernel(const int *sorted_cols, size_t nnz, int n_cols, int *csc_ptr) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_cols) return;
    size_t lo = 0, hi = nnz;
    while (lo < hi) {
        const size_t mid = (lo + hi) >> 1;
        if (sorted_cols[mid] < c) lo = mid + 1; else hi = mid;
    }
    csc_ptr[c] = (int)lo;
}

// Row id of every stored cell (one wave per row): the payload of the CSR -> CSC sort for all-ones data.
__global__ void expand_rows_kernel(const int *ptr, int n_rows, int *row_of) {
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= n_rows) return;
    for (int q = ptr[wave] + lane; q < ptr[wave + 1]; q += 64) row_of[q] = wave;
}

// Payload of the CSR -> CSC sort for valued data: (row id, value bits) of every stored cell in one 8-byte word, so that the sort
// itself carries the cells into column order (a sorted permutation + a gather of rows and values through it spent 0.7 ms on its
// 2 x 20 M random 4-byte reads at the ML-20M shape).
__global__ void expand_cells_kernel(const int *ptr, const float *val, int n_rows, unsigned long long *cell) {
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= n_rows) return;
    for (int q = ptr[wave] + lane; q < ptr[wave + 1]; q += 64)
        cell[q] = (unsigned long long)(unsigned)wave | ((unsigned long long)__float_as_uint(val[q]) << 32);
}

// CSC view from the sorted cells: users inside a column stay in ascending order (the sort is stable).
__global__ void split_cells_kernel(const unsigned long long *cell, size_t nnz, int *csc_idx, float *csc_val) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nnz; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long c = cell[i];
        csc_idx[i] = (int)(unsigned)c;
        csc_val[i] = __uint_as_float((unsigned)(c >> 32));
    }
}

// cost = sum of the profile lengths of a column's rows, for ALL columns with the cells dealt evenly: a wavefront per 4 096 cells of
// the column-ordered arrays (one wavefront per column spent 1.2 ms on the longest column of the ML-20M shape alone).  `col_of` is the
// sorted key array of the CSR -> CSC sort.  Runs of one column are summed in registers, one atomic per run and wavefront; the few
// cells of a stretch of 64 that spans several columns add themselves.
// COUNTED (the walk list of all-ones data as the column view: `csc_idx` = slice numbers, `csr_ptr` = scan of the rows' lengths filed
// under their FIRST slice): bits 40.. of the sum count the entries with a non-zero length = the column's users.
constexpr int COST_CHUNK = 4096;
constexpr int COST_COUNT_SHIFT = 40;
template <bool COUNTED>
__global__ __launch_bounds__(256) void column_cost_kernel(const int *col_of, const int *csc_idx, const int *csr_ptr, size_t nnz,
                                                          unsigned long long *cost) {
    const size_t wave = (blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const size_t first = wave * COST_CHUNK, last = first + COST_CHUNK < nnz ? first + COST_CHUNK : nnz;
    if (first >= nnz) return;
    int cur = -1;
    unsigned long long part = 0;
    auto flush = [&]() {
        for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
        if (lane == 0 && cur >= 0 && part) atomicAdd(&cost[cur], part);
        part = 0;
    };
    for (size_t q0 = first; q0 < last; q0 += 64) {
        const size_t q = q0 + lane;
        const bool live = q < last;
        const int col = live ? col_of[q] : -1;
        const int u = live ? csc_idx[q] : 0;
        unsigned long long len = live ? (unsigned long long)(csr_ptr[u + 1] - csr_ptr[u]) : 0ull;
        if (COUNTED && len) len |= 1ull << COST_COUNT_SHIFT;
        const int col0 = __builtin_amdgcn_readfirstlane(col);
        if (__all(!live || col == col0)) {
            if (col0 != cur) {
                flush();
                cur = col0;
            }
            part += len;
        } else {
            flush();
            cur = -1;
            if (live) atomicAdd(&cost[col], len);
        }
    }
    flush();
}

// applyPearsonCorrelation (.pyx:234-271): subtract the column mean from every stored cell, both views.
__global__ void col_center_kernel(const int *col_of, float *val, size_t nnz, const float *mean) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nnz; i += (size_t)gridDim.x * blockDim.x)
        val[i] -= mean[col_of[i]];
}
__global__ void col_center_csc_kernel(const int *csc_ptr, float *csc_val, int n_cols, const float *mean) {
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= n_cols) return;
    const float m = mean[wave];
    for (int q = csc_ptr[wave] + lane; q < csc_ptr[wave + 1]; q += 64) csc_val[q] -= m;
}

// numpy_pairwise_sum over the SQUARES of a[0 .. n) (each square rounded to float32 first, like dataMatrix.power(2))
__device__ float numpy_pairwise_sum_sq(const float *a, int n) {
    if (n < 8) {
        float r = 0.f;
        for (int i = 0; i < n; ++i) r = __fadd_rn(r, __fmul_rn(a[i], a[i]));
        return r;
    }
    if (n <= 128) {
        float r[8];
        for (int j = 0; j < 8; ++j) r[j] = __fmul_rn(a[j], a[j]);
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] = __fadd_rn(r[j], __fmul_rn(a[i + j], a[i + j]));
        float res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])), __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
        for (; i < n; ++i) res = __fadd_rn(res, __fmul_rn(a[i], a[i]));
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return __fadd_rn(numpy_pairwise_sum_sq(a, n2), numpy_pairwise_sum_sq(a + n2, n - n2));
}

// `dataMatrix.power(2).sum(axis=0)` as the reference gets it (.pyx:169): float32 squares, float32 sums, in SciPy's order for the
// format at hand -- order 0 (CSR: ones @ X): a column's squares one after the other in row order (the CSC view built here keeps
// each column's cells in row order); order 1 (CSC: np.add.reduceat): first square + NumPy's pairwise sum of the rest.  One thread
// per column: the additions of a column are a dependent chain by definition (0.3 ms for the longest column at ML-20M shape).
__global__ void column_sumsq_f32_kernel(const int *csc_ptr, const float *csc_val, int n_cols, int order, double *sumsq) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    const int s = csc_ptr[c], e = csc_ptr[c + 1];
    float sum = 0.f;
    if (order == 0) {
        for (int q = s; q < e; ++q) sum = __fadd_rn(sum, __fmul_rn(csc_val[q], csc_val[q]));
    } else if (e > s) {
        sum = __fmul_rn(csc_val[s], csc_val[s]);
        if (e - s > 1) sum = __fadd_rn(sum, numpy_pairwise_sum_sq(csc_val + s + 1, e - s - 1));
    }
    sumsq[c] = (double)sum;
}
// Order 0 for long columns, one WAVEFRONT per column: the chain of float32 additions cannot be split, but its operands can be
// fetched 64 at a time (coalesced, the next chunk in flight) and handed from lane to lane with v_readlane -- 8 cycles per cell
// instead of one exposed global load each (13 ms for the 100 000-cell columns of the ML-20M shape with one thread per column).
// Lanes past the end contribute +0.0f, which leaves a non-negative float32 sum unchanged.
__global__ __launch_bounds__(256) void column_sumsq_f32_rowwise_kernel(const int *csc_ptr, const float *csc_val, int n_cols, double *sumsq) {
    const int lane = threadIdx.x & 63;
    const int c = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6);
    if (c >= n_cols) return;
    const int s = csc_ptr[c], e = csc_ptr[c + 1];
    float sum = 0.f;
    float v = s + lane < e ? csc_val[s + lane] : 0.f;
    for (int q = s; q < e; q += 64) {
        const float sq = __fmul_rn(v, v);
        v = q + 64 + lane < e ? csc_val[q + 64 + lane] : 0.f;            // next chunk
#pragma unroll
        for (int l = 0; l < 64; ++l)
            sum = __fadd_rn(sum, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sq), l)));
    }
    if (lane == 0) sumsq[c] = (double)sum;
}

// all-ones data: the sum of a column's squares is its number of stored cells, exactly, in any order (float32 holds every count
// below 2^24; beyond that the serial float32 chain decides)
__global__ void column_count_sumsq_kernel(const int *csc_ptr, int n_cols, double *sumsq) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n_cols) sumsq[c] = (double)(csc_ptr[c + 1] - csc_ptr[c]);
}
__global__ void iota_kernel(int *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = i;
}

// sumOfSquared -> norms (.pyx:169-177)
__global__ void norms_kernel(const double *sumsq, int n_cols, int set_based, int asymmetric, int euclidean, float alpha,
                             float *norm, float *norm_alpha, float *norm_1ma) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    double s = sumsq[c];
    if (euclidean) {   // float32 like the reference: item_distance_initial and its square root (Euclidean.py:112-113)
        norm_alpha[c] = (float)s;
        norm[c] = __fsqrt_rn((float)s);
        return;
    }
    if (!set_based) s = sqrt(s);
    norm[c] = (float)s;
    if (asymmetric) {
        norm_1ma[c] = (float)pow(s, 2.0 * (1.0 - (double)alpha));
        norm_alpha[c] = (float)pow(s, 2.0 * (double)alpha);
    }
}

// ---- walk lists: what the column kernel's accumulation walks (see SimParams::walk8) ------------------------------------------------
// A user's profile segment is cut into slices of at most WALK_SLICE chunks (of 8 entries); the slices of ALL rows are ordered by
// descending length once (a few hundred thousand of them), the (column, slice) pairs are generated in that order from the CSR rows
// and a STABLE sort by column leaves every column's slices longest first.
constexpr int WALK_SLICE = 128;

// slices per row (tiled accumulators: the row itself is the entry -- its segments differ per tile)
__global__ void walk_row_slices_kernel(const int *csr_ptr, const int *seg_ptr, int n_rows, int tiled, int *n_slices) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_rows) return;
    const int len = csr_ptr[u + 1] - csr_ptr[u];
    int n = 0;
    if (len > 0) n = tiled ? 1 : ((seg_ptr[u + 1] - seg_ptr[u]) / 8 + WALK_SLICE - 1) / WALK_SLICE;
    n_slices[u] = n;
}

// one record per slice: key = its chunks (tiled: the row's chunks over all tiles, clamped), value = row | slice << 32
__global__ void walk_slice_records_kernel(const int *csr_ptr, const int *seg_ptr, const int *slice_off, int n_rows, int tiled, int n_tiles,
                                          unsigned *key, unsigned long long *rec) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_rows) return;
    const int at = slice_off[u], n = slice_off[u + 1] - at;
    if (n == 0) return;
    if (tiled) {
        const int chunks = (seg_ptr[(size_t)(u + 1) * n_tiles] - seg_ptr[(size_t)u * n_tiles]) / 8;
        key[at] = (unsigned)min(chunks / 4, 255);
        rec[at] = (unsigned long long)(unsigned)u;
        return;
    }
    const int chunks = (seg_ptr[u + 1] - seg_ptr[u]) / 8;
    for (int j = 0; j < n; ++j) {
        key[at + j] = (unsigned)min(WALK_SLICE, chunks - j * WALK_SLICE);
        rec[at + j] = (unsigned long long)(unsigned)u | ((unsigned long long)j << 32);
    }
}

// per record (sorted order): the cells it emits (= the row's length), the row's length filed under its first slice only (what a
// column's cost and user count are summed from), and the slice's bounds in the profile stream
__global__ void walk_record_lengths_kernel(const unsigned long long *rec, const int *csr_ptr, const int *seg_ptr, int n_rec, int tiled,
                                           int *len, int *first_len, uint2 *tab) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rec) {
        const unsigned long long rc = rec[r];
        const int u = (int)(unsigned)rc, j = (int)(rc >> 32);
        const int n = csr_ptr[u + 1] - csr_ptr[u];
        len[r] = n;
        first_len[r] = j == 0 ? n : 0;
        if (!tiled) {
            const int s0 = seg_ptr[u], s1 = seg_ptr[u + 1];
            tab[r] = make_uint2((unsigned)(s0 + j * WALK_SLICE * 8), (unsigned)min(s1, s0 + (j + 1) * WALK_SLICE * 8));
        }
    }
    if (r == n_rec) {
        len[r] = 0;
        first_len[r] = 0;
    }
}

// the packed sums of column_cost_kernel<true>: cost, users (as the column's sum of squares and as an int)
__global__ void walk_unpack_cost_kernel(const unsigned long long *packed, int n_cols, long long *cost, double *sumsq, int *count) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cols) return;
    const unsigned long long v = packed[c];
    cost[c] = (long long)(v & ((1ull << COST_COUNT_SHIFT) - 1ull));
    sumsq[c] = (double)(v >> COST_COUNT_SHIFT);
    count[c] = (int)(v >> COST_COUNT_SHIFT);
}

// One workgroup per slice record (in sorted order): its (column, entry) pairs, one per stored cell of the row.  WIDE: 16-byte entries
// with the column-side value of the cell (times the row's weight), else 4-byte entries: the record's number (tiled: the row).
template <bool WIDE>
__global__ __launch_bounds__(256) void walk_generate_kernel(const unsigned long long *rec, const int *out_off, const int *csr_ptr, const int *csr_idx,
                                                            const float *csr_val, const int *seg_ptr, const float *row_w, int unit_col, int tiled,
                                                            int *key, void *entries) {
    const int r = blockIdx.x;
    const unsigned long long rc = rec[r];
    const int u = (int)(unsigned)rc, j = (int)(rc >> 32);
    const int a = csr_ptr[u], len = csr_ptr[u + 1] - a, at = out_off[r];
    unsigned ex = (unsigned)u, ey = 0u;
    if (!tiled && WIDE) {
        const int s0 = seg_ptr[u], s1 = seg_ptr[u + 1];
        ex = (unsigned)(s0 + j * WALK_SLICE * 8);
        ey = (unsigned)min(s1, s0 + (j + 1) * WALK_SLICE * 8);
    }
    const float w = row_w ? row_w[u] : 1.f;
    for (int i = threadIdx.x; i < len; i += 256) {
        key[at + i] = csr_idx[a + i];
        if (WIDE) {
            float cv = unit_col ? 1.f : csr_val[a + i];
            if (row_w) cv *= w;
            reinterpret_cast<uint4 *>(entries)[at + i] = make_uint4(ex, ey, __float_as_uint(cv), 0u);
        } else {
            reinterpret_cast<int *>(entries)[at + i] = tiled ? u : r;
        }
    }
}

// ---- BM25 / TF-IDF re-weighting of the stored values (Base/IR_feature_weighting.py:13-75) ---------------------------------
// Per row and per column of the CSR: the sum of the stored values and their number; one wavefront per row, the column side
// through atomics (20 M cells at ML-20M shape: a few hundred microseconds, once per build).  float64 throughout -- the
// reference mixes float32 (row sums, length norm) and float64 (idf); the float32 results agree to a few 1e-7 relative.
__global__ __launch_bounds__(256) void weighting_stats_kernel(const int *csr_ptr, const int *csr_idx, const float *csr_val, int n_rows,
                                                              double *row_sum, double *col_sum, int *col_cnt, double *total) {
    const int lane = threadIdx.x & 63;
    const int row = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6);
    if (row >= n_rows) return;
    double sum = 0.0;
    for (int q = csr_ptr[row] + lane; q < csr_ptr[row + 1]; q += 64) {
        const double v = (double)csr_val[q];
        sum += v;
        atomicAdd(&col_sum[csr_idx[q]], v);
        atomicAdd(&col_cnt[csr_idx[q]], 1);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane == 0) {
        row_sum[row] = sum;
        if (sum != 0.0) atomicAdd(&total[row & 63], sum);
    }
}

// okapi_BM_25 (:35-49): idf = log(N / (1 + cells of the term)), length_norm = (1 - B) + B * document_sum / mean document sum,
// value * (K1 + 1) / (K1 * length_norm + value) * idf, a zero denominator replaced by 1e-9;  TF_IDF (:69-73): sqrt(value) * idf.
__global__ __launch_bounds__(256) void weighting_apply_kernel(const int *csr_ptr, const int *csr_idx, float *csr_val, int n_rows, int n_cols,
                                                              const double *row_sum, const double *col_sum, const int *col_cnt,
                                                              const double *total, int mode, int documents_are_rows, double k1, double b) {
    const int lane = threadIdx.x & 63;
    const int row = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 6);
    if (row >= n_rows) return;
    double all = 0.0;
    for (int w = 0; w < 64; ++w) all += total[w];
    const double n_docs = documents_are_rows ? (double)n_rows : (double)n_cols;
    const double mean_len = all / n_docs;
    const int begin = csr_ptr[row], end = csr_ptr[row + 1];
    for (int q = begin + lane; q < end; q += 64) {
        const int col = csr_idx[q];
        const double v = (double)csr_val[q];
        const double cells_of_term = documents_are_rows ? (double)col_cnt[col] : (double)(end - begin);
        const double idf = log(n_docs / (1.0 + cells_of_term));
        double out;
        if (mode == MI355REC_WEIGHT_BM25) {
            const double doc_sum = documents_are_rows ? row_sum[row] : col_sum[col];
            double den = k1 * ((1.0 - b) + b * doc_sum / mean_len) + v;
            if (den == 0.0) den += 1e-9;
            out = v * (k1 + 1.0) / den * idf;
        } else {
            out = sqrt(v) * idf;
        }
        csr_val[q] = (float)out;
    }
}

// largest |value| (bit pattern of a non-negative float orders like the unsigned integer)
__global__ void absmax_kernel(const float *val, size_t nnz, unsigned *out) {
    unsigned m = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nnz; i += (size_t)gridDim.x * blockDim.x)
        m = max(m, __float_as_uint(fabsf(val[i])));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// smallest non-zero |value| (same ordering; `out` starts at 0xFFFFFFFF and stays there when every stored value is zero)
__global__ void absmin_nonzero_kernel(const float *val, size_t nnz, unsigned *out) {
    unsigned m = 0xFFFFFFFFu;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nnz; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned b = __float_as_uint(fabsf(val[i]));
        if (b) m = min(m, b);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63) == 0 && m != 0xFFFFFFFFu) atomicMin(out, m);
}

// CSR assembly of the result (.pyx:603-605: row = neighbour, column = source item) -- sort keys: the neighbour id of
// every slab entry, padding entries (-1) mapped past the last row so that they sort to the end.
__global__ void csr_keys_kernel(const int *slab_idx, size_t n, int n_cols, int *key, int *pos) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int r = slab_idx[e];
        key[e] = r >= 0 ? r : n_cols;
        pos[e] = (int)e;
    }
}

// After the stable sort by neighbour id: entry t of the CSR arrays comes from slab position pos[t]; its column is the
// slab row (source item).  Positions ascend inside a row, hence so do the columns: indices come out sorted.
__global__ void csr_gather_kernel(const int *pos, const float *slab_val, size_t n, int topK, int start_col, int *indices,
                                  float *data) {
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
        const int e = pos[t];
        indices[t] = start_col + e / topK;
        data[t] = slab_val[e];
    }
}

// [n_local][n_cols] -> [n_cols][n_local] (32x32 tiles through LDS)
__global__ void transpose_kernel(const float *in, float *out, int rows, int cols) {
    __shared__ float tile[32][33];
    int x = blockIdx.x * 32 + threadIdx.x, y = blockIdx.y * 32 + threadIdx.y;
    for (int k = 0; k < 32; k += 8)
        if (x < cols && y + k < rows) tile[threadIdx.y + k][threadIdx.x] = in[(size_t)(y + k) * cols + x];
    __syncthreads();
    x = blockIdx.y * 32 + threadIdx.x;
    y = blockIdx.x * 32 + threadIdx.y;
    for (int k = 0; k < 32; k += 8)
        if (x < rows && y + k < cols) out[(size_t)(y + k) * rows + x] = tile[threadIdx.x][threadIdx.y + k];
}

}  // namespace
}  // namespace mi355rec
