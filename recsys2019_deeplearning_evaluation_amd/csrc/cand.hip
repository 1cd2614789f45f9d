// cand.hip -- scoring and ranking of candidate rows on MI355X (gfx950): every user ranks a short list of items of its own -- the
// reference's EvaluatorNegativeItemSample
// (Base/Evaluation/Evaluator.py:455-539: the test items plus sampled negatives of a user go to recommend() as items_to_compute,
// Base/BaseRecommender.py:131-222: everything else becomes -inf, then the seen / custom filters and the top-cutoff).
//   cand_score_rank_kernel   factor models, one workgroup per user: U[u] . V[c] (+ biases) for the user's candidates ONLY -- groups of
//                            G lanes share a candidate (lanes across the factors, 16-byte loads where the rows allow it, four
//                            candidates' rows in flight per group, a shuffle reduction); no score matrix, no GEMM.
//   spscore_cand_kernel      similarity models, score row in LDS: spscore_kernel's accumulation, then only the candidates are read
//                            from the row.
//   cand_gather_rank_kernel  similarity models, score row in HBM (spscore_wide_kernel as it is): the candidates are gathered.
// All three end in cand_filter_rank: the candidates sit in LDS as (key << 32 | ~position), the user's seen items are looked up in
// the (ascending) candidate row, and block_rank_emit of topk.cuh ranks what is left -- value descending, ties towards the lower
// position, which is the lower item id.
// A translation unit of its own: score.hip's kernels share topk.cuh's routines with these, and the device code generated for
// them must not depend on who else instantiates a routine (score.hip's device assembly is the parent's, function by function).
#include "common.h"
#include "score.h"
#include "topk.cuh"
#include "cand.cuh"

#include <algorithm>

namespace mi355rec {
namespace {

struct CandScoreParams {
    CandParams c;
    int k, use_bias, lanes, vec;    // lanes: G, a power of two <= 64; vec: rows are read in 16-byte quads (k % 4 == 0)
    int cand_pad;                   // entries of the LDS candidate buffer (even)
    const float *U, *V, *bu, *bi;
    float mu;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void cand_score_rank_kernel(const CandScoreParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cand_smem[];
    uint64_t *cand = reinterpret_cast<uint64_t *>(cand_smem);
    float *s_u = reinterpret_cast<float *>(cand_smem + (size_t)p.cand_pad * 8);
    __shared__ SelectScratch sc;
    __shared__ uint32_t s_nfinite;
    const int tid = threadIdx.x;
    const int b = blockIdx.x, u = p.c.users[b];
    const int row = p.c.by_user ? u : b;
    const int c0 = p.c.cand_ptr[row], ncand = p.c.cand_ptr[row + 1] - c0;
    const int *items = p.c.cand_idx + c0;
    if (tid == 0) { s_nfinite = 0; sc.out_count = 0; }
    for (int t = tid; t < p.k; t += THREADS) s_u[t] = p.U[(size_t)u * p.k + t];
    __syncthreads();
    const int G = p.lanes, NG = THREADS / G, g = tid / G, part = tid & (G - 1);
    const float user_term = p.use_bias ? p.bu[u] + p.mu : 0.f;
    constexpr int R = 4;            // rows in flight per group
    for (int base = 0; base < ncand; base += NG * R) {      // (uniform trip count: every lane takes part in the shuffles)
        int pos[R], item[R];
        const float *vrow[R];
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            pos[r] = base + r * NG + g;
            item[r] = items[min(pos[r], ncand - 1)];        // (a position past the end reads the last row again and is dropped below)
            vrow[r] = p.V + (size_t)item[r] * p.k;
            acc[r] = 0.f;
        }
        if (p.vec) {
            for (int q = part; q < (p.k >> 2); q += G) {
                const float4 a = reinterpret_cast<const float4 *>(s_u)[q];
                float4 v[R];
#pragma unroll
                for (int r = 0; r < R; ++r) v[r] = reinterpret_cast<const float4 *>(vrow[r])[q];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fmaf(a.w, v[r].w, fmaf(a.z, v[r].z, fmaf(a.y, v[r].y, fmaf(a.x, v[r].x, acc[r]))));
            }
        } else {
            for (int q = part; q < p.k; q += G) {
                const float a = s_u[q];
                float v[R];
#pragma unroll
                for (int r = 0; r < R; ++r) v[r] = vrow[r][q];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fmaf(a, v[r], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            for (int off = 1; off < G; off <<= 1) acc[r] += __shfl_xor(acc[r], off);
            if (part == 0 && pos[r] < ncand) {
                float s = acc[r];
                if (p.use_bias) s += p.bi[item[r]] + user_term;
                if (p.c.allowed && !p.c.allowed[item[r]]) s = -INFINITY;
                cand[pos[r]] = cand_entry(s, pos[r]);
            }
        }
    }
    cand_filter_rank<THREADS>(p.c, u, items, ncand, cand, sc, &s_nfinite, p.c.ranked + (size_t)b * p.c.cutoff);
}

// spscore_kernel's accumulation (one wavefront per stored cell of A[u], LDS float atomics), then the candidates alone are read
// from the row: no pass over the n_out cells after the zeroing.
struct SpCandParams {
    CandParams c;
    int n_pad;                      // floats of the LDS score row (a multiple of 4), the candidate buffer behind it
    const int *a_ptr, *a_idx, *b_ptr, *b_idx;
    const float *a_val, *b_val;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void spscore_cand_kernel(const SpCandParams p) {
    const CandParams &c = p.c;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *acc = smem;
    uint64_t *cand = reinterpret_cast<uint64_t *>(smem + p.n_pad);
    __shared__ SelectScratch sc;
    __shared__ uint32_t s_nfinite;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int WAVES = THREADS / 64;
    const int b = blockIdx.x, u = c.users[b];
    const int row = c.by_user ? u : b;
    const int c0 = c.cand_ptr[row], ncand = c.cand_ptr[row + 1] - c0;
    const int *items = c.cand_idx + c0;
    if (tid == 0) { s_nfinite = 0; sc.out_count = 0; }
    for (int j = tid; j < p.n_pad; j += THREADS) acc[j] = 0.f;
    __syncthreads();
    for (int q = p.a_ptr[u] + wave; q < p.a_ptr[u + 1]; q += WAVES) {
        const int m = p.a_idx[q];
        const float w = p.a_val[q];
        for (int t = p.b_ptr[m] + lane; t < p.b_ptr[m + 1]; t += 64) atomicAdd(&acc[p.b_idx[t]], w * p.b_val[t]);
    }
    __syncthreads();
    for (int i = tid; i < ncand; i += THREADS) {
        const int item = items[i];
        cand[i] = cand_entry(c.allowed && !c.allowed[item] ? -INFINITY : acc[item], i);
    }
    cand_filter_rank<THREADS>(c, u, items, ncand, cand, sc, &s_nfinite, c.ranked + (size_t)b * c.cutoff);
}

// the candidates of score rows in HBM (spscore_wide_kernel has accumulated them): scores[b][n_items], unfiltered
template <int THREADS>
__global__ __launch_bounds__(THREADS) void cand_gather_rank_kernel(const CandParams c, const float *scores, int n_items) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cand_smem[];
    uint64_t *cand = reinterpret_cast<uint64_t *>(cand_smem);
    __shared__ SelectScratch sc;
    __shared__ uint32_t s_nfinite;
    const int tid = threadIdx.x;
    const int b = blockIdx.x, u = c.users[b];
    const int row = c.by_user ? u : b;
    const int c0 = c.cand_ptr[row], ncand = c.cand_ptr[row + 1] - c0;
    const int *items = c.cand_idx + c0;
    const float *srow = scores + (size_t)b * n_items;
    if (tid == 0) { s_nfinite = 0; sc.out_count = 0; }
    for (int i = tid; i < ncand; i += THREADS) {
        const int item = items[i];
        cand[i] = cand_entry(c.allowed && !c.allowed[item] ? -INFINITY : srow[item], i);
    }
    cand_filter_rank<THREADS>(c, u, items, ncand, cand, sc, &s_nfinite, c.ranked + (size_t)b * c.cutoff);
}

}  // namespace

void check_candidate_cutoff(int cutoff) {
    if (cutoff > MAX_TOPK) fail(MI355REC_E_UNSUPPORTED, "candidate lists of %d entries: at most %d", cutoff, MAX_TOPK);
}

int check_candidate_rows(const int32_t *indptr, const int32_t *indices, int n_rows, int n_items) {
    MI_REQUIRE(indptr && (indices || indptr[n_rows] == 0), "NULL argument");
    MI_REQUIRE(indptr[0] == 0, "candidate indptr must start at 0");
    int longest = 0;
    for (int r = 0; r < n_rows; ++r) {
        const int a = indptr[r], e = indptr[r + 1];
        MI_REQUIRE(a <= e, "candidate indptr is not monotone");
        for (int q = a; q < e; ++q) {
            MI_REQUIRE(indices[q] >= 0 && indices[q] < n_items, "candidate row %d: item id %d outside [0, %d)", r, indices[q], n_items);
            MI_REQUIRE(q == a || indices[q - 1] < indices[q], "candidate row %d: item ids must be strictly ascending", r);
        }
        longest = std::max(longest, e - a);
    }
    if (longest > CAND_MAX) fail(MI355REC_E_UNSUPPORTED, "a candidate row of %d items: at most %d", longest, CAND_MAX);
    return longest;
}

void recommend_candidates(ScorerHandle *h, const int32_t *user_ids, int n, const int32_t *cand_indptr, const int32_t *cand_indices,
                          int cutoff, int remove_seen, const uint8_t *item_allowed, int32_t *ranked) {
    MI_REQUIRE(h && user_ids && cand_indptr && ranked, "NULL argument");
    MI_REQUIRE(n > 0, "empty user batch");
    MI_REQUIRE(cutoff >= 1 && cutoff <= h->n_items, "cutoff must be in [1, n_items]");
    for (int i = 0; i < n; ++i)
        if (user_ids[i] < 0 || user_ids[i] >= h->n_users) h->bad_user(user_ids[i]);
    const int longest = check_candidate_rows(cand_indptr, cand_indices, n, h->n_items);
    check_candidate_cutoff(cutoff);     // (before anything is uploaded; enqueue_candidates checks for every caller)
    ensure_device();
    hipStream_t s = h->stream;
    const size_t nnz = (size_t)cand_indptr[n];
    if (h->users.count < (size_t)n || h->cand_ptr.count < (size_t)n + 1 || h->cand_idx.count < std::max<size_t>(nnz, 1)) {
        MI_HIP(hipStreamSynchronize(s));
        if (h->users.count < (size_t)n) h->users.alloc(n);
        if (h->cand_ptr.count < (size_t)n + 1) h->cand_ptr.alloc((size_t)n + 1);
        if (h->cand_idx.count < std::max<size_t>(nnz, 1)) h->cand_idx.alloc(std::max<size_t>(nnz, 1));
    }
    MI_HIP(hipMemcpyAsync(h->users.ptr, user_ids, sizeof(int) * n, hipMemcpyHostToDevice, s));
    MI_HIP(hipMemcpyAsync(h->cand_ptr.ptr, cand_indptr, sizeof(int) * ((size_t)n + 1), hipMemcpyHostToDevice, s));
    if (nnz) MI_HIP(hipMemcpyAsync(h->cand_idx.ptr, cand_indices, sizeof(int) * nnz, hipMemcpyHostToDevice, s));
    if (item_allowed) MI_HIP(hipMemcpyAsync(h->allowed.ptr, item_allowed, h->n_items, hipMemcpyHostToDevice, s));
    h->enqueue_candidates(h->users.ptr, n, cutoff, remove_seen, item_allowed ? h->allowed.ptr : nullptr,
                          CandidateRows{h->cand_ptr.ptr, h->cand_idx.ptr, false, longest});
    h->ranked.download(ranked, (size_t)n * cutoff, s);
    MI_HIP(hipStreamSynchronize(s));
    h->stats = mi355rec_stats{};
    h->stats.kernel_ms = h->stats.call_ms = h->timer.elapsed_ms();      // the candidate kernel(s): there is no GEMM to tell apart
    h->stats.n_launches = h->stats.n_timed = 1;
    h->stats.n_units = n;
}

}  // namespace mi355rec

using namespace mi355rec;

Ranking mi355rec_scorer::enqueue_candidates(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                                            const CandidateRows &rows) {
    hipStream_t s = stream;
    check_candidate_cutoff(cutoff);
    reserve((size_t)n * cutoff, 0, 0);
    CandScoreParams p{};
    p.c = cand_params(this, users, cutoff, remove_seen, allowed, rows);
    p.k = k; p.use_bias = use_bias;
    p.vec = (k & 3) == 0;
    const int units = p.vec ? k >> 2 : k;
    p.lanes = 1;
    while (p.lanes < 64 && p.lanes < units) p.lanes <<= 1;
    p.cand_pad = cand_buffer_entries(rows.longest);
    p.U = U.ptr; p.V = V.ptr; p.bu = bu.ptr; p.bi = bi.ptr; p.mu = mu;
    const size_t lds = (size_t)p.cand_pad * 8 + (size_t)((k + 3) & ~3) * 4;
    if (lds + 1024 > 160 * 1024) fail(MI355REC_E_UNSUPPORTED, "%d factors do not fit LDS next to the candidate buffer", k);
    auto kernel = cand_score_rank_kernel<CAND_THREADS>;
    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipExtLaunchKernelGGL(kernel, dim3(n), dim3(CAND_THREADS), (unsigned)lds, s, timer.t0, timer.t1, 0, p);
    MI_HIP(hipGetLastError());
    return Ranking{ranked.ptr, s};
}

Ranking mi355rec_spscorer::enqueue_candidates(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                                              const CandidateRows &rows) {
    if (exact) return spexact_enqueue_candidates(this, users, n, cutoff, remove_seen, allowed, rows);
    hipStream_t s = stream;
    check_candidate_cutoff(cutoff);
    const bool in_lds = score_row_fits_lds(n_items, cutoff);
    reserve((size_t)n * cutoff, in_lds ? 0 : (size_t)n * n_items, 0);
    const CandParams c = cand_params(this, users, cutoff, remove_seen, allowed, rows);
    timer.start(s);
    if (in_lds) {
        SpCandParams p{};
        p.c = c; p.n_pad = (n_items + 3) & ~3;
        p.a_ptr = a_ptr.ptr; p.a_idx = a_idx.ptr; p.a_val = a_val.ptr;
        p.b_ptr = b_ptr.ptr; p.b_idx = b_idx.ptr; p.b_val = b_val.ptr;
        const size_t lds = (size_t)p.n_pad * 4 + (size_t)AUX_WORDS * 4;
        auto k = spscore_cand_kernel<1024>;
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, dim3(n), dim3(1024), lds, s, p);
    } else {
        spscorer_enqueue_wide_rows(this, users, n);
        const size_t lds = (size_t)cand_buffer_entries(rows.longest) * 8;
        auto k = cand_gather_rank_kernel<CAND_THREADS>;
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, dim3(n), dim3(CAND_THREADS), lds, s, c, (const float *)scores.ptr, n_items);
    }
    MI_HIP(hipGetLastError());
    timer.stop(s);
    return Ranking{ranked.ptr, s};
}

extern "C" int mi355rec_scorer_recommend_candidates(mi355rec_scorer_t h, const int32_t *user_ids, int32_t n, const int32_t *cand_indptr,
                                                    const int32_t *cand_indices, int32_t cutoff, int32_t remove_seen,
                                                    const uint8_t *item_allowed, int32_t *ranked) {
    return guarded([&] { recommend_candidates(h, user_ids, n, cand_indptr, cand_indices, cutoff, remove_seen, item_allowed, ranked); });
}

extern "C" int mi355rec_spscorer_recommend_candidates(mi355rec_spscorer_t h, const int32_t *user_ids, int32_t n, const int32_t *cand_indptr,
                                                      const int32_t *cand_indices, int32_t cutoff, int32_t remove_seen,
                                                      const uint8_t *item_allowed, int32_t *ranked) {
    return guarded([&] { recommend_candidates(h, user_ids, n, cand_indptr, cand_indices, cutoff, remove_seen, item_allowed, ranked); });
}

extern "C" int mi355rec_scorer_score_capacity(mi355rec_scorer_t h, int64_t *cells) {
    return guarded([&] {
        MI_REQUIRE(h && cells, "NULL argument");
        *cells = (int64_t)h->scores.count;
    });
}
