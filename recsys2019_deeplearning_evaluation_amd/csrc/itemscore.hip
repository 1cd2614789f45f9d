// itemscore.hip -- ranking for models that give every user the SAME item scores, on MI355X (gfx950): the reference's TopPop and
// GlobalEffects (Base/NonPersonalizedRecommender.py:30-43, 119-132: _compute_item_score repeats one vector of n_items scores for
// every user of the batch) under the filter + top-cutoff half of BaseRecommender.recommend (Base/BaseRecommender.py:131-222).
// The vector is sorted ONCE per model; a user's list is the head of that order minus the user's seen items:
//   order_keys_kernel      per model: the sort key of every item (finite scores only), one stable rocPRIM radix sort orders the ids by
//                          (score descending, id ascending); rank_scatter_kernel writes the inverse, rank_of[item].
//   (per call with an item mask: the order is compacted by the mask -- rocprim::select, one pass -- and the inverse rebuilt.)
//   itemscore_rank_kernel  one workgroup of THREADS lanes per user.  With L seen items the list lies inside the first cutoff + L
//                          positions of the order (of those, at most L are seen: at least `cutoff` are not).  A window of
//                          W = 32 * THREADS positions at a time: the positions rank_of[seen item] inside the window are set in an LDS
//                          bitmap (a word per lane), popcounts and a prefix sum over the words give every lane the output slot of its
//                          first clear bit, and order[position] of the clear bits is stored until `cutoff` items are out.  Work per
//                          user: cutoff + L, not n_items; LDS per workgroup: THREADS words whatever n_items and L are.
//   itemscore_cand_kernel  candidate rows (EvaluatorNegativeItemSample): the vector gathered at the user's candidates, then
//                          cand_filter_rank (cand.cuh) as for the other scorers.
//   itemscore_fill_kernel / itemscore_seen_kernel  return_scores=True: the vector broadcast into the batch's rows, -inf where a filter
//                          applies.
// No atomics on global memory; the lists are written with plain stores.
#include "common.h"
#include "itemscore.h"
#include "topk.cuh"
#include "cand.cuh"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cmath>

namespace mi355rec {
namespace {

constexpr int WAVE_WINDOW = 64 * 32, GROUP_WINDOW = 256 * 32;   // W of the two kernel shapes: a wavefront / a 256-lane workgroup per user
constexpr int DEFAULT_WINDOW = GROUP_WINDOW;                     // the faster one at the ML-20M shape
constexpr uint32_t NOT_LISTED = 0xFFFFFFFFu;                     // sort key of a non-finite score: behind every finite one

__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) < INFINITY; }     // (false for NaN)

// keys ascending = scores descending; -0.0 ranks with +0.0 (float_key alone would put it below)
__global__ __launch_bounds__(256) void order_keys_kernel(const float *vec, int n, uint32_t *keys, int *ids) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = vec[i];
    if (v == 0.f) v = 0.f;
    keys[i] = is_finite(v) ? ~float_key(v) : NOT_LISTED;
    ids[i] = i;
}

// rank_of[order[p]] = p for p < length[0]; the other entries of rank_of have been set to -1
__global__ __launch_bounds__(256) void rank_scatter_kernel(const int *order, const int *length, int *rank_of) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < length[0]) rank_of[order[p]] = p;
}

struct AllowedItem {
    const unsigned char *allowed;
    __device__ bool operator()(const int &item) const { return allowed[item] != 0; }
};

struct ItemRankParams {
    int cutoff, remove_seen;
    const int *order, *rank_of, *length;
    const int *users, *seen_ptr, *seen_idx;
    int *ranked;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void itemscore_rank_kernel(const ItemRankParams p) {
    constexpr int W = THREADS * 32, WAVES = THREADS / 64;
    __shared__ uint32_t bits[THREADS];          // bit r of the window: position base + r of the order is a seen item
    __shared__ uint32_t wave_tot[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, u = p.users[b];
    const int len = p.length[0];
    const int s0 = p.remove_seen ? p.seen_ptr[u] : 0, s1 = p.remove_seen ? p.seen_ptr[u + 1] : 0;
    // the list lies inside the first cutoff + L positions: at most L of them are seen (fewer when the row repeats an item)
    const int bound = (int)min((long long)len, (long long)p.cutoff + (long long)(s1 - s0));
    int *out = p.ranked + (size_t)b * p.cutoff;
    int emitted = 0;                            // (the same in every lane)
    for (int base = 0; base < bound && emitted < p.cutoff; base += W) {
        const int wlen = min(W, bound - base);
        bits[tid] = 0;
        __syncthreads();
        for (int q = s0 + tid; q < s1; q += THREADS) {      // the seen row need not be sorted and may repeat an item
            const int r = p.rank_of[p.seen_idx[q]] - base;  // (-1 -- an item outside the order -- stays negative)
            if ((unsigned)r < (unsigned)wlen) atomicOr(&bits[r >> 5], 1u << (r & 31));
        }
        __syncthreads();
        const int first = tid * 32;
        const int nvalid = min(32, max(0, wlen - first));
        const uint32_t valid = nvalid >= 32 ? 0xFFFFFFFFu : ((1u << nvalid) - 1u);
        uint32_t clear = ~bits[tid] & valid;
        const uint32_t cnt = (uint32_t)__popc(clear);
        uint32_t incl = cnt;                    // clear bits of this lane's word and of the words before it in the wavefront
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        uint32_t before = 0, total = __shfl(incl, 63);
        if (WAVES > 1) {
            if (lane == 63) wave_tot[wave] = incl;
            __syncthreads();
            total = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                if (w < wave) before += wave_tot[w];
                total += wave_tot[w];
            }
        }
        int pos = emitted + (int)(before + incl - cnt);
        while (clear && pos < p.cutoff) {
            const int bit = __ffs(clear) - 1;
            out[pos++] = p.order[base + first + bit];
            clear &= clear - 1u;
        }
        emitted = (int)min((long long)p.cutoff, (long long)emitted + (long long)total);
        __syncthreads();                        // bits and wave_tot are written again by the next window
    }
    for (int t = emitted + tid; t < p.cutoff; t += THREADS) out[t] = -1;
}

// scores[b][j] = vec[j], -inf where the mask excludes j; the seen items of the batch's users afterwards (a launch of its own: the two
// stores to a seen cell must not race)
__global__ __launch_bounds__(256) void itemscore_fill_kernel(const float *vec, const unsigned char *allowed, int n_items, float *scores) {
    float *row = scores + (size_t)blockIdx.y * n_items;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n_items; j += gridDim.x * 256) row[j] = allowed && !allowed[j] ? -INFINITY : vec[j];
}

__global__ __launch_bounds__(256) void itemscore_seen_kernel(const int *users, const int *seen_ptr, const int *seen_idx, int n_items, float *scores) {
    const int u = users[blockIdx.x];
    float *row = scores + (size_t)blockIdx.x * n_items;
    for (int q = seen_ptr[u] + threadIdx.x; q < seen_ptr[u + 1]; q += 256) row[seen_idx[q]] = -INFINITY;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void itemscore_cand_kernel(const CandParams c, const float *vec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cand_smem[];
    uint64_t *cand = reinterpret_cast<uint64_t *>(cand_smem);
    __shared__ SelectScratch sc;
    __shared__ uint32_t s_nfinite;
    const int tid = threadIdx.x;
    const int b = blockIdx.x, u = c.users[b];
    const int row = c.by_user ? u : b;
    const int c0 = c.cand_ptr[row], ncand = c.cand_ptr[row + 1] - c0;
    const int *items = c.cand_idx + c0;
    if (tid == 0) { s_nfinite = 0; sc.out_count = 0; }
    for (int i = tid; i < ncand; i += THREADS) {
        const int item = items[i];
        float v = vec[item];
        if (v == 0.f) v = 0.f;
        cand[i] = cand_entry((c.allowed && !c.allowed[item]) || !is_finite(v) ? -INFINITY : v, i);
    }
    cand_filter_rank<THREADS>(c, u, items, ncand, cand, sc, &s_nfinite, c.ranked + (size_t)b * c.cutoff);
}

size_t sort_bytes(mi355rec_itemscorer *h) {
    size_t bytes = 0;
    MI_HIP(rocprim::radix_sort_pairs(nullptr, bytes, h->keys.ptr, h->keys_sorted.ptr, h->ids.ptr, h->order.ptr, (size_t)h->n_items, 0, 32,
                                     h->stream));
    return bytes;
}

size_t select_bytes(mi355rec_itemscorer *h) {
    size_t bytes = 0;
    MI_HIP(rocprim::select(nullptr, bytes, h->order.ptr, h->m_order.ptr, h->m_length.ptr, (size_t)h->n_items, AllowedItem{nullptr}, h->stream));
    return bytes;
}

void scatter_ranks(hipStream_t s, const int *order, const int *length, int n_order, int n_items, int *rank_of) {
    MI_HIP(hipMemsetAsync(rank_of, 0xFF, sizeof(int) * (size_t)n_items, s));
    if (n_order) hipLaunchKernelGGL(rank_scatter_kernel, dim3(div_up(n_order, 256)), dim3(256), 0, s, order, length, rank_of);
}

// the vector goes up, its order and the inverse are rebuilt; ends with the stream drained (`item_scores` and n_order are host memory)
void upload_vector(mi355rec_itemscorer *h, const float *item_scores) {
    hipStream_t s = h->stream;
    const int n = h->n_items;
    int n_order = 0;
    for (int i = 0; i < n; ++i) n_order += std::isfinite(item_scores[i]);
    MI_HIP(hipMemcpyAsync(h->vec.ptr, item_scores, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, s));
    MI_HIP(hipMemcpyAsync(h->length.ptr, &n_order, sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(order_keys_kernel, dim3(div_up(n, 256)), dim3(256), 0, s, h->vec.ptr, n, h->keys.ptr, h->ids.ptr);
    size_t bytes = h->tmp.count;
    MI_HIP(rocprim::radix_sort_pairs(h->tmp.ptr, bytes, h->keys.ptr, h->keys_sorted.ptr, h->ids.ptr, h->order.ptr, (size_t)n, 0, 32, s));
    scatter_ranks(s, h->order.ptr, h->length.ptr, n_order, n, h->rank_of.ptr);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(s));
    h->n_order = n_order;
}

void create(mi355rec_itemscorer_t *out, int n_users, int n_items, const float *item_scores, const int32_t *seen_indptr,
            const int32_t *seen_indices, bool resident, int64_t seen_nnz) {
    MI_REQUIRE(out && item_scores && seen_indptr && (seen_indices || seen_nnz == 0), "NULL argument");
    MI_REQUIRE(n_users > 0 && n_items > 0, "empty model");
    if (!resident) {
        MI_REQUIRE(seen_indptr[0] == 0, "seen indptr must start at 0");
        for (int u = 0; u < n_users; ++u) MI_REQUIRE(seen_indptr[u] <= seen_indptr[u + 1], "seen indptr is not monotone");
        seen_nnz = seen_indptr[n_users];
        for (int64_t q = 0; q < seen_nnz; ++q)
            MI_REQUIRE(seen_indices[q] >= 0 && seen_indices[q] < n_items, "seen item id %d outside [0, %d)", seen_indices[q], n_items);
    }
    MI_REQUIRE(seen_nnz >= 0 && seen_nnz <= INT32_MAX, "%lld seen cells do not fit int32 row pointers", (long long)seen_nnz);
    auto h = open_handle<mi355rec_itemscorer>(1);
    hipStream_t s = h->stream;
    h->n_users = n_users; h->n_items = n_items; h->window_bits = DEFAULT_WINDOW;
    h->seen_ptr.alloc((size_t)n_users + 1);
    h->seen_idx.alloc(std::max<size_t>((size_t)seen_nnz, 1));
    const hipMemcpyKind kind = resident ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    MI_HIP(hipMemcpyAsync(h->seen_ptr.ptr, seen_indptr, sizeof(int) * ((size_t)n_users + 1), kind, s));
    if (seen_nnz) MI_HIP(hipMemcpyAsync(h->seen_idx.ptr, seen_indices, sizeof(int) * (size_t)seen_nnz, kind, s));
    h->allowed.alloc(n_items);
    h->vec.alloc(n_items);
    h->order.alloc(n_items); h->rank_of.alloc(n_items); h->length.alloc(1);
    h->m_order.alloc(n_items); h->m_rank_of.alloc(n_items); h->m_length.alloc(1);
    h->keys.alloc(n_items); h->keys_sorted.alloc(n_items); h->ids.alloc(n_items);
    h->tmp.alloc(std::max(sort_bytes(h.get()), select_bytes(h.get())) + 256);
    upload_vector(h.get(), item_scores);
    *out = h.release();
}

}  // namespace
}  // namespace mi355rec

using namespace mi355rec;

Ranking mi355rec_itemscorer::enqueue(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed, bool keep_scores) {
    hipStream_t s = stream;
    if (keep_scores && n > 65535) fail(MI355REC_E_UNSUPPORTED, "score rows of %d users in one call: at most 65535", n);
    reserve((size_t)n * cutoff, keep_scores ? (size_t)n * n_items : 0, 0);
    timer.start(s);
    ItemRankParams p{};
    p.cutoff = cutoff; p.remove_seen = remove_seen;
    p.order = order.ptr; p.rank_of = rank_of.ptr; p.length = length.ptr;
    if (allowed) {                              // the order without the excluded items, and its inverse
        if (n_order) {
            size_t bytes = tmp.count;
            MI_HIP(rocprim::select(tmp.ptr, bytes, order.ptr, m_order.ptr, m_length.ptr, (size_t)n_order, AllowedItem{allowed}, s));
        } else {
            MI_HIP(hipMemsetAsync(m_length.ptr, 0, sizeof(int), s));
        }
        scatter_ranks(s, m_order.ptr, m_length.ptr, n_order, n_items, m_rank_of.ptr);
        p.order = m_order.ptr; p.rank_of = m_rank_of.ptr; p.length = m_length.ptr;
    }
    p.users = users; p.seen_ptr = seen_ptr.ptr; p.seen_idx = seen_idx.ptr;
    p.ranked = ranked.ptr;
    if (window_bits == WAVE_WINDOW) hipLaunchKernelGGL(itemscore_rank_kernel<64>, dim3(n), dim3(64), 0, s, p);
    else hipLaunchKernelGGL(itemscore_rank_kernel<256>, dim3(n), dim3(256), 0, s, p);
    if (keep_scores) {
        hipLaunchKernelGGL(itemscore_fill_kernel, dim3(std::min(div_up(n_items, 256), 64), n), dim3(256), 0, s, vec.ptr, allowed, n_items,
                           scores.ptr);
        if (remove_seen)
            hipLaunchKernelGGL(itemscore_seen_kernel, dim3(n), dim3(256), 0, s, users, seen_ptr.ptr, seen_idx.ptr, n_items, scores.ptr);
    }
    MI_HIP(hipGetLastError());
    timer.stop(s);
    return Ranking{ranked.ptr, s};
}

Ranking mi355rec_itemscorer::enqueue_candidates(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                                                const CandidateRows &rows) {
    hipStream_t s = stream;
    check_candidate_cutoff(cutoff);
    reserve((size_t)n * cutoff, 0, 0);
    const CandParams c = cand_params(this, users, cutoff, remove_seen, allowed, rows);
    const size_t lds = (size_t)cand_buffer_entries(rows.longest) * 8;
    auto k = itemscore_cand_kernel<CAND_THREADS>;
    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    timer.start(s);
    hipLaunchKernelGGL(k, dim3(n), dim3(CAND_THREADS), lds, s, c, (const float *)vec.ptr);
    MI_HIP(hipGetLastError());
    timer.stop(s);
    return Ranking{ranked.ptr, s};
}

void mi355rec_itemscorer::fill_recommend_stats(const int32_t *, int) { stats.kernel_ms = stats.call_ms = timer.elapsed_ms(); }

extern "C" int mi355rec_itemscorer_create(mi355rec_itemscorer_t *out, int32_t n_users, int32_t n_items, const float *item_scores,
                                          const int32_t *seen_indptr, const int32_t *seen_indices) {
    return guarded([&] { create(out, n_users, n_items, item_scores, seen_indptr, seen_indices, false, 0); });
}

extern "C" int mi355rec_itemscorer_create_resident(mi355rec_itemscorer_t *out, int32_t n_users, int32_t n_items, const float *item_scores,
                                                   const int32_t *d_seen_indptr, const int32_t *d_seen_indices, int64_t seen_nnz) {
    return guarded([&] { create(out, n_users, n_items, item_scores, d_seen_indptr, d_seen_indices, true, seen_nnz); });
}

extern "C" int mi355rec_itemscorer_update(mi355rec_itemscorer_t h, const float *item_scores) {
    return guarded([&] {
        MI_REQUIRE(h && item_scores, "NULL argument");
        ensure_device();
        MI_HIP(hipStreamSynchronize(h->stream));        // (a ranking still running reads the old order)
        upload_vector(h, item_scores);
    });
}

extern "C" int mi355rec_itemscorer_recommend(mi355rec_itemscorer_t h, const int32_t *user_ids, int32_t n, int32_t cutoff, int32_t remove_seen,
                                             const uint8_t *item_allowed, int32_t *ranked, float *scores) {
    return guarded([&] { recommend(h, user_ids, n, cutoff, remove_seen, item_allowed, ranked, scores); });
}

extern "C" int mi355rec_itemscorer_recommend_candidates(mi355rec_itemscorer_t h, const int32_t *user_ids, int32_t n, const int32_t *cand_indptr,
                                                        const int32_t *cand_indices, int32_t cutoff, int32_t remove_seen,
                                                        const uint8_t *item_allowed, int32_t *ranked) {
    return guarded([&] { recommend_candidates(h, user_ids, n, cand_indptr, cand_indices, cutoff, remove_seen, item_allowed, ranked); });
}

extern "C" int mi355rec_itemscorer_window_bits(mi355rec_itemscorer_t h, int32_t *bits) {
    return guarded([&] {
        MI_REQUIRE(h && bits, "NULL argument");
        *bits = h->window_bits;
    });
}

extern "C" int mi355rec_itemscorer_set_window_bits(mi355rec_itemscorer_t h, int32_t bits) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL argument");
        MI_REQUIRE(bits == WAVE_WINDOW || bits == GROUP_WINDOW, "window of %d bits: %d (a wavefront per user) or %d (a workgroup per user)", bits,
                   WAVE_WINDOW, GROUP_WINDOW);
        h->window_bits = bits;
    });
}

extern "C" int mi355rec_itemscorer_get_stats(mi355rec_itemscorer_t h, mi355rec_stats *stats) { return handle_get_stats(h, stats); }

extern "C" void mi355rec_itemscorer_destroy(mi355rec_itemscorer_t h) { handle_destroy(h); }
