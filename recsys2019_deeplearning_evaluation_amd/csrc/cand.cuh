// cand.cuh -- what the kernels that rank candidate rows share (cand.hip: the factor and the similarity scorers; itemscore.hip: the
// shared item vector): the candidates sit in LDS as (key << 32 | ~position), the user's seen items are looked up in the (ascending)
// candidate row, and block_rank_emit of topk.cuh ranks what is left.  Internal linkage throughout: every translation unit gets its
// own copy of the device code.
#pragma once

#include "common.h"
#include "score.h"
#include "topk.cuh"

#include <algorithm>

namespace mi355rec {
namespace {

static_assert(CAND_MAX == AUX_WORDS / 2, "a candidate row is one block_rank_emit over the 32 KiB candidate buffer");
constexpr int CAND_THREADS = 256;

struct CandParams {
    int cutoff, remove_seen, by_user;
    const int *users, *seen_ptr, *seen_idx;
    const int *cand_ptr, *cand_idx;
    const unsigned char *allowed;   // nullable, as RankParams::allowed
    int *ranked;
};

__device__ __forceinline__ uint64_t cand_entry(float v, int pos) {
    if (!(v > -INFINITY)) v = -INFINITY;                            // (NaN is not admissible either, as in the full-row ranking)
    return ((uint64_t)float_key(v) << 32) | (uint32_t)(~(uint32_t)pos);
}

// cand[0 .. ncand): the candidates' entries, mask filter applied, written by the caller (no barrier needed behind the writes);
// *nfinite and sc.out_count are 0.  Seen items -> -inf, then the ranking of the admissible ones, -1 padded.
template <int THREADS>
__device__ __forceinline__ void cand_filter_rank(const CandParams &p, int u, const int *items, int ncand, uint64_t *cand, SelectScratch &sc,
                                                 uint32_t *nfinite, int *out) {
    const int tid = threadIdx.x, lane = tid & 63;
    __syncthreads();
    if (p.remove_seen) {            // _remove_seen_on_scores (BaseRecommender.py:110-117); the seen row need not be sorted, `items` is
        for (int q = p.seen_ptr[u] + tid; q < p.seen_ptr[u + 1]; q += THREADS) {
            const int s = p.seen_idx[q];
            int lo = 0, hi = ncand;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (items[mid] < s) lo = mid + 1; else hi = mid;
            }
            if (lo < ncand && items[lo] == s) cand[lo] = cand_entry(-INFINITY, lo);
        }
        __syncthreads();
    }
    uint32_t nfin = 0;
    for (int i = tid; i < ncand; i += THREADS) nfin += (uint32_t)(cand[i] >> 32) > float_key(-INFINITY);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nfin += __shfl_down(nfin, off);
    if (lane == 0 && nfin) atomicAdd(nfinite, nfin);
    __syncthreads();
    // the -inf entries hold the lowest keys: they rank behind every admissible candidate and K stops in front of them
    const uint32_t K = min((uint32_t)p.cutoff, *nfinite);
    block_rank_emit<THREADS>(cand, ncand, p.cutoff, K, 0u, sc, out, nullptr, 0, items);
}

// entries of the LDS candidate buffer: the row, or the power of two block_rank_emit's bitonic branch pads a row above 1024 to
inline int cand_buffer_entries(int longest) {
    if (longest <= 1024) return std::max(2, (longest + 1) & ~1);
    int P = 2048;
    while (P < longest) P <<= 1;
    return P;
}

inline CandParams cand_params(ScorerHandle *h, const int *users, int cutoff, int remove_seen, const unsigned char *allowed, const CandidateRows &rows) {
    CandParams c{};
    c.cutoff = cutoff; c.remove_seen = remove_seen; c.by_user = rows.by_user;
    c.users = users; c.seen_ptr = h->seen_ptr.ptr; c.seen_idx = h->seen_idx.ptr;
    c.cand_ptr = rows.ptr; c.cand_idx = rows.idx;
    c.allowed = allowed; c.ranked = h->ranked.ptr;
    return c;
}

}  // namespace
}  // namespace mi355rec
