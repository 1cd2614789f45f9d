// slim_readout.cuh -- reading the model out: per-row top-K and dense get_S, the sparse store's prune / list kernels, and the four
// slim_w_* kernels of W = similarityMatrixTopK(get_S(), k).  Included by slim.hip after slim_flow.cuh and topk.cuh.
#pragma once

#include "slim_flow.cuh"

namespace mi355rec {
namespace {

// get_S (.pyx:343-391): row r of S with the diagonal zeroed (symmetric store mirrored), then the per-row top-K.
template <class T, int THREADS>
__global__ __launch_bounds__(THREADS) void slim_topk_kernel(const SlimParams<T> p, int topK, int n_pad, int *out_idx,
                                                            float *out_val) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *acc = smem;
    uint32_t *aux = reinterpret_cast<uint32_t *>(smem + n_pad);
    __shared__ SelectScratch sc;
    __shared__ uint32_t s_npos, s_nneg, s_ncand;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int r = blockIdx.x; r < p.n_items; r += gridDim.x) {
        if (tid == 0) { s_npos = 0; s_nneg = 0; s_ncand = 0; }
        __syncthreads();
        uint32_t npos = 0, nneg = 0;
        for (int c = tid; c < p.n_items; c += THREADS) {
            const float v = c == r ? 0.f : stored_value(p, r, c);
            acc[c] = v;
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
        // symmetric store: Triangular_Matrix.get_scipy_csr ranks the FULL row (zeros compete, :1384-1404);
        // dense store: similarityMatrixTopK ranks the non-zero cells only (Base/Recommender_utils.py:100-104)
        block_topk_emit<THREADS>(acc, p.n_items, topK, s_npos, s_nneg, p.symmetric ? TOPK_ZEROS_COMPETE : TOPK_NONZERO, aux, sc, &s_ncand,
                                 out_idx + (size_t)r * topK, out_val + (size_t)r * topK);
        __syncthreads();
    }
}

template <class T>
__global__ void slim_dense_kernel(const SlimParams<T> p, float *out) {
    const size_t n = (size_t)p.n_items;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n * n; e += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(e / n), c = (int)(e % n);
        out[e] = r == c ? 0.f : stored_value(p, r, c);
    }
}

// ---- the sparse-tree store's semantics on the dense array (Sparse_Matrix_Tree_CSR, .pyx:582-1030) --------------------------
// A cell "has a node" once add_value has written it.  Cells without a node hold the bit pattern of -0.0: it reads as zero,
// any update a + lr * g of a step turns it into an ordinary value, and no arithmetic of the epoch produces it again (an
// update that is exactly -0.0 would; that needs a gradient that underflowed to zero).
constexpr unsigned long long NO_NODE = 0x8000000000000000ull;
constexpr int PRUNE_THREADS = 256;

__global__ __launch_bounds__(256) void slim_no_nodes_kernel(unsigned long long *S, size_t n_cells) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n_cells; e += (size_t)gridDim.x * blockDim.x) S[e] = NO_NODE;
}

// unsigned key in the order of the doubles
__device__ __forceinline__ unsigned long long order_key(unsigned long long bits) {
    return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
}

// topK_selection_from_list on every row (.pyx:957-1030), as rebalance_tree(TopK) :785-805 and get_scipy_csr(TopK) :740-780 apply
// it: a row with fewer than TopK nodes is left alone, otherwise the TopK largest values stay; among equal values the HIGHER
// columns stay (glibc's qsort is a stable merge sort and compare_struct_on_data :553-568 never answers "equal", so ties keep
// their column order and the last TopK of the sorted array are taken).  Dropped nodes are freed: no node, value zero.
//
// One workgroup per row.  The row is streamed once to count its nodes (most of the work: n_items^2 * 8 bytes per call, HBM
// bound).  A row that has to be cut is read again (from L2) and its nodes are packed, in column order, into LDS, where an
// 8-bit radix select finds the TopK-th value; rows with more than PRUNE_CAP nodes run the same select over the row itself.
// The select stops as soon as the bucket holding the TopK-th value is wanted whole.
constexpr int PRUNE_CAP = 2048;

struct PruneShared {
    unsigned hist[256];
    unsigned wave_count[PRUNE_THREADS / 64];
    unsigned keep, bucket;
    unsigned long long prefix;
    unsigned long long keys[PRUNE_CAP];
    int cols[PRUNE_CAP];
};

// the row itself as the select's source: position = column
struct RowSource {
    unsigned long long *row;
    int n;
    __device__ __forceinline__ int size() const { return n; }
    __device__ __forceinline__ bool key(int at, unsigned long long &k) const {
        const unsigned long long b = row[at];
        k = order_key(b);
        return b != NO_NODE;
    }
    __device__ __forceinline__ void drop(int at) const { row[at] = NO_NODE; }
};
// the packed nodes in LDS (column order)
struct PackedSource {
    unsigned long long *row;
    const unsigned long long *keys;
    const int *cols;
    int len;
    __device__ __forceinline__ int size() const { return len; }
    __device__ __forceinline__ bool key(int at, unsigned long long &k) const { k = keys[at]; return true; }
    __device__ __forceinline__ void drop(int at) const { row[cols[at]] = NO_NODE; }
};

template <class Src>
__device__ __forceinline__ void select_and_drop(const Src src, const int topK, PruneShared &sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int size = src.size();
    // radix select, most significant byte first: after a pass the wanted value's leading bytes are `prefix`, `keep` of the
    // keys that share them stay (all keys above them stay anyway)
    unsigned keep = (unsigned)topK, bucket = 0;
    unsigned long long prefix = 0;
    int shift = 64;
    while (shift > 0) {
        shift -= 8;
        sh.hist[tid] = 0;                                           // (PRUNE_THREADS == 256)
        __syncthreads();
        for (int at = tid; at < size; at += PRUNE_THREADS) {
            unsigned long long k;
            if (!src.key(at, k)) continue;
            if (shift == 56 || (k >> (shift + 8)) == prefix) atomicAdd(&sh.hist[(unsigned)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (wave == 0) {                                            // lane l owns digits 4l .. 4l+3; suffix sums from the top digit down
            const unsigned h0 = sh.hist[4 * lane], h1 = sh.hist[4 * lane + 1], h2 = sh.hist[4 * lane + 2], h3 = sh.hist[4 * lane + 3];
            const unsigned own = h0 + h1 + h2 + h3;
            unsigned incl = own;                                    // sum over lanes >= this one
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned v = __shfl_down(incl, off);
                if (lane + off < 64) incl += v;
            }
            const unsigned long long reach = __ballot(incl >= keep);
            const int owner = 63 - __builtin_clzll(reach);          // the highest lane whose suffix reaches `keep`
            if (lane == owner) {
                unsigned above = incl - own;                        // keys in higher digits
                int d = 3;
                unsigned hd = h3;
                if (above + hd < keep) { above += hd; d = 2; hd = h2; }
                if (d == 2 && above + hd < keep) { above += hd; d = 1; hd = h1; }
                if (d == 1 && above + hd < keep) { above += hd; d = 0; hd = h0; }
                sh.prefix = (prefix << 8) | (unsigned long long)(4 * lane + d);
                sh.keep = keep - above;
                sh.bucket = hd;
            }
        }
        __syncthreads();
        prefix = sh.prefix;
        keep = sh.keep;
        bucket = sh.bucket;
        if (bucket == keep) break;                                  // the whole bucket stays: nothing left to split
    }
    // keys whose leading bytes are below `prefix` go; of the `bucket` keys equal to it the `keep` highest columns stay
    const unsigned drop_ties = bucket - keep;                       // > 0 only after all 8 passes: equal VALUES
    unsigned ties_before = 0;                                       // ties in lower columns (only tracked when some must go)
    for (int at0 = 0; at0 < size; at0 += PRUNE_THREADS) {
        const int at = at0 + tid;
        bool tie = false, drop = false;
        if (at < size) {
            unsigned long long k;
            if (src.key(at, k)) {
                k >>= shift;
                drop = k < prefix;
                tie = k == prefix;
            }
        }
        if (drop_ties) {
            const unsigned long long m = __ballot(tie);
            __syncthreads();
            if (lane == 0) sh.wave_count[wave] = (unsigned)__builtin_popcountll(m);
            __syncthreads();
            unsigned before = ties_before, total = 0;
#pragma unroll
            for (int w = 0; w < PRUNE_THREADS / 64; ++w) {
                if (w < wave) before += sh.wave_count[w];
                total += sh.wave_count[w];
            }
            before += (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull));
            if (tie && before < drop_ties) drop = true;             // the first (lowest-column) `drop_ties` ties go
            ties_before += total;
        }
        if (drop) src.drop(at);
    }
    __syncthreads();
}

// with_diag: get_S gives the diagonal a node holding zero first (.pyx:350-351).
__global__ __launch_bounds__(PRUNE_THREADS) void slim_prune_kernel(unsigned long long *S, int n, int topK, int with_diag) {
    __shared__ PruneShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // every wavefront owns one contiguous quarter of the row (whole 64-column groups)
    const int seg = ((n + PRUNE_THREADS - 1) / PRUNE_THREADS) * 64;
    const int c_begin = min(wave * seg, n), c_end = min(c_begin + seg, n);
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        unsigned long long *row = S + (size_t)r * n;
        if (with_diag && tid == 0) row[r] = 0ull;               // a node holding +0.0
        __syncthreads();
        unsigned mine = 0;
        int c = c_begin + lane;
        for (; c + 192 < c_end; c += 256) {                     // four independent loads in flight per lane
            const unsigned long long b0 = row[c], b1 = row[c + 64], b2 = row[c + 128], b3 = row[c + 192];
            mine += (b0 != NO_NODE) + (b1 != NO_NODE) + (b2 != NO_NODE) + (b3 != NO_NODE);
        }
        for (; c < c_end; c += 64) mine += row[c] != NO_NODE;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
        if (lane == 0) sh.wave_count[wave] = mine;
        __syncthreads();
        unsigned len = 0, base = 0;
#pragma unroll
        for (int w = 0; w < PRUNE_THREADS / 64; ++w) {
            if (w < wave) base += sh.wave_count[w];
            len += sh.wave_count[w];
        }
        __syncthreads();
        if (topK <= 0 || len <= (unsigned)topK) continue;        // (len == TopK: the selection keeps everything)
        if (len <= (unsigned)PRUNE_CAP) {
            // pack (key, column) in column order: wavefront w writes from `base`, lanes by ballot rank
            for (int c0 = c_begin; c0 < c_end; c0 += 64) {
                const int cc = c0 + lane;
                const unsigned long long b = cc < c_end ? row[cc] : NO_NODE;
                const bool node = b != NO_NODE;
                const unsigned long long m = __ballot(node);
                if (node) {
                    const unsigned at = base + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull));
                    sh.keys[at] = order_key(b);
                    sh.cols[at] = cc;
                }
                base += (unsigned)__builtin_popcountll(m);
            }
            __syncthreads();
            select_and_drop(PackedSource{row, sh.keys, sh.cols, (int)len}, topK, sh);
        } else {
            select_and_drop(RowSource{row, n}, topK, sh);
        }
    }
}

// from_linked_list_to_python_list (.pyx:862-875) for every row after the selection: the non-zero nodes in column order.
__global__ __launch_bounds__(PRUNE_THREADS) void slim_list_kernel(const unsigned long long *S, int n, int width, int *out_idx, float *out_val) {
    __shared__ unsigned s_wave[PRUNE_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        const unsigned long long *row = S + (size_t)r * n;
        unsigned at = 0;
        for (int c0 = 0; c0 < n; c0 += PRUNE_THREADS) {
            const int c = c0 + tid;
            double v = 0.0;
            if (c < n) {
                const unsigned long long b = row[c];
                if (b != NO_NODE) v = __longlong_as_double((long long)b);
            }
            const bool listed = v != 0.0;
            const unsigned long long m = __ballot(listed);
            if (lane == 0) s_wave[wave] = (unsigned)__builtin_popcountll(m);
            __syncthreads();
            unsigned pos = at, total = 0;
#pragma unroll
            for (int w = 0; w < PRUNE_THREADS / 64; ++w) {
                if (w < wave) pos += s_wave[w];
                total += s_wave[w];
            }
            pos += (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull));
            if (listed && pos < (unsigned)width) {
                out_idx[(size_t)r * width + pos] = c;
                out_val[(size_t)r * width + pos] = (float)v;
            }
            at += total;
            __syncthreads();
        }
        for (unsigned q = min(at, (unsigned)width) + tid; q < (unsigned)width; q += PRUNE_THREADS) {
            out_idx[(size_t)r * width + q] = -1;
            out_val[(size_t)r * width + q] = 0.f;
        }
    }
}

}  // namespace
}  // namespace mi355rec

namespace {      // (not mi355rec's: these four kernels keep the names they have had)
using mi355rec::float_key;

// W = similarityMatrixTopK(get_S(), k) on the device (Base/Recommender_utils.py:55-122 applied to the per-row selection of .pyx:343-391;
// SLIM_BPR_Cython.py:186-197 does this at every validation, and on the host the column step alone -- 9 000 over-full columns ranked one
// by one -- was 0.09 s at ML-20M size against 2 ms for the epoch it follows).  From the (row, K) slabs: one radix sort of the non-zero
// entries by (column, value descending, row descending) ranks every column -- the host function's stable ascending sort drops the first
// len - k entries of a column, i.e. of equal values it keeps the HIGHEST rows --, entries ranked below k are dropped, a second sort by
// (row, column) puts the survivors into canonical CSR order.  Items are 16-bit here (n_items <= 65 535), like everywhere on this path.
__global__ void slim_w_rank_keys_kernel(const int *idx, const float *val, size_t n_slots, int topK, unsigned long long *key, int *slot) {
    const size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (q >= n_slots) return;
    const int col = idx[q];
    const float v = val[q];
    slot[q] = (int)q;
    if (col < 0 || v == 0.f) {
        key[q] = ~0ull;                                   // (padding and zeros sort behind every column)
        return;
    }
    const unsigned row = (unsigned)(q / (size_t)topK);
    key[q] = ((unsigned long long)(unsigned)col << 48) | ((unsigned long long)(~float_key(v)) << 16) | (unsigned long long)(0xFFFFu - row);
}
// position of every column's first entry in the ranked order (binary search on the column field; n_items + 1 entries, the last = the
// number of real entries)
__global__ void slim_w_col_start_kernel(const unsigned long long *ranked, size_t n_slots, int n_items, int *start) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_items) return;
    size_t lo = 0, hi = n_slots;
    while (lo < hi) {
        const size_t mid = (lo + hi) >> 1;
        const unsigned long long k = ranked[mid];
        const bool before = k != ~0ull && (int)(k >> 48) < c;
        if (before) lo = mid + 1; else hi = mid;
    }
    start[c] = (int)lo;
}
// the survivors' (row, column) keys and values, in ranked order; everything else sorts behind them
__global__ void slim_w_keep_kernel(const unsigned long long *ranked, const int *slot, const int *col_start, const float *val, size_t n_slots, int topK,
                                   int k_cols, unsigned *key2, float *val2) {
    const size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (q >= n_slots) return;
    const unsigned long long k = ranked[q];
    key2[q] = ~0u;
    val2[q] = 0.f;
    if (k == ~0ull) return;
    const int col = (int)(k >> 48);
    if ((int)q - col_start[col] >= k_cols) return;
    const int s = slot[q];
    key2[q] = ((unsigned)(s / topK) << 16) | (unsigned)col;
    val2[q] = val[s];
}
__global__ void slim_w_csr_kernel(const unsigned *key2, size_t n_slots, int n_items, int *indptr, int *indices) {
    const size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (q < n_slots && key2[q] != ~0u) indices[q] = (int)(key2[q] & 0xFFFFu);
    if (q <= (size_t)n_items) {                          // first entry whose row is >= q
        size_t lo = 0, hi = n_slots;
        while (lo < hi) {
            const size_t mid = (lo + hi) >> 1;
            const bool before = key2[mid] != ~0u && (key2[mid] >> 16) < (unsigned)q;
            if (before) lo = mid + 1; else hi = mid;
        }
        indptr[q] = (int)lo;
    }
}

}  // namespace
