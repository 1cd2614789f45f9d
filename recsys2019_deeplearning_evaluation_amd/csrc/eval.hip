// eval.hip -- holdout metrics on MI355X (gfx950): the per-user loop of the reference's EvaluatorHoldout
// (Base/Evaluation/Evaluator.py:294-374 _compute_metrics_on_recommendation_list, the metric functions of
// Base/Evaluation/metrics.py) run over ranked lists that are already in HBM.
//
//   eval_metric_kernel  one wavefront per user, list positions across the lanes (64-wide chunks): is_relevant[j] by a binary
//                       search of ranked[j] in the user's sorted test row (its relevance comes along), wave ballots give the hit
//                       counts, masked wave sums give every per-cutoff quantity in one pass; the float32 DCG terms go to LDS and
//                       are summed the way NumPy's pairwise float32 reduction sums them.  Per-user values -> HBM, fp64,
//                       [user][cutoff][value]; every list entry adds 1 to counts[b][item] (b = the smallest cutoff that holds it).
//   eval_sum_kernel     each (cutoff, value) column summed over all users in a fixed order (no floating-point atomics).
//   eval_counts_kernel  counts[b] -> counts of every cutoff: a running sum over b.
// The lists come either from a device scorer (score.h: ScorerHandle::enqueue, the kernel runs on the scorer's stream and reads its
// `ranked` buffer in place) or from the host (the lists path).  For the reference's EvaluatorNegativeItemSample (Evaluator.py:455-539)
// the scorers rank each user's candidate row only (ScorerHandle::enqueue_candidates; the rows are uploaded once by
// mi355rec_eval_set_candidates); the metric kernel and finish are the same.
// With an item diversity matrix set (mi355rec_eval_set_diversity) every metric launch is followed, on the same stream and in front of
// the `done` event, by eval_diversity_kernel (eval_diversity.cuh): DIVERSITY_SIMILARITY into a buffer of its own, summed by
// eval_sum_kernel in finish.
#include "common.h"
#include "score.h"
#include "itemscore.h"
#include "wave.cuh"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>

#pragma clang fp contract(off)

#include "eval_diversity.cuh"

namespace mi355rec {
namespace {

constexpr int NV = MI355REC_EVAL_VALUES;
constexpr int MAX_CUTOFFS = 64;
constexpr int MAX_WIDTH = 32768;    // the DCG terms of a list live in LDS (4 bytes per position)
enum { V_ROC, V_PREC, V_PREC_MIN, V_RECALL, V_AP, V_RR, V_NDCG, V_HITS, V_ARHR, V_NOVELTY, V_POP, V_COVERED };

struct EvalParams {
    int n_items, width, n_cut, n_sorted;
    const int *cut;                 // [n_cut] cutoffs as given
    const int *cut_sorted;          // [n_sorted] distinct cutoffs ascending (the counter buckets)
    const int *test_ptr, *test_idx; // test rows, sorted by item id
    const float *test_rel;          // their relevance (float32: ndcg's rank_scores, metrics.py:191)
    const float *idcg;              // [n_users]
    const float *logs;              // [width] np.log(np.arange(width, dtype=np.float32) + 2) (metrics.py:208)
    const double *novelty, *popularity;   // per-item terms (metrics.py:567-572, 619-621)
    const int *users;               // the evaluation's users; this block is positions [first, first + n)
    int first;
    const int *ranked;              // [n][width], -1 padded at the end
    double *vals;                   // [n_eval][n_cut][NV]
    int *counts;                    // [n_sorted][n_items]
};

// NumPy's pairwise float32 summation (np.sum of a contiguous float32 array): leaves of at most 128 entries summed with 8
// accumulators, longer ranges split at a multiple of 8 near the middle.  metrics.py:208-209 sums the DCG terms this way.
__device__ __forceinline__ float pairwise_leaf(const float *a, int n) {
    if (n < 8) {
        float r = 0.f;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
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
template <int DEPTH> __device__ __noinline__ float pairwise_sum(const float *a, int n) {
    if (n <= 128) return pairwise_leaf(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise_sum<DEPTH - 1>(a, n2) + pairwise_sum<DEPTH - 1>(a + n2, n - n2);
}
template <> __device__ __noinline__ float pairwise_sum<0>(const float *a, int n) { return pairwise_leaf(a, n); }

// float32 a / b, correctly rounded (a double quotient of two floats rounds to the float quotient)
__device__ __forceinline__ float div_f32(float a, float b) { return (float)((double)a / (double)b); }

__global__ __launch_bounds__(64) void eval_metric_kernel(const EvalParams p) {
    extern __shared__ float dterm[];                    // [width] DCG term of every position (0 where not relevant)
    __shared__ double s_sum[MAX_CUTOFFS][5];            // per cutoff: sum of hit positions, AP terms, 1/rank of hits, novelty, popularity
    __shared__ int s_cnt[MAX_CUTOFFS][2];               // per cutoff: list length, hits
    const int lane = threadIdx.x;
    const int b = blockIdx.x, pos = p.first + b, u = p.users[pos];
    const int *row = p.ranked + (size_t)b * p.width;
    const int t0 = p.test_ptr[u], t1 = p.test_ptr[u + 1];
    for (int c = lane; c < p.n_cut; c += 64) {
        for (int q = 0; q < 5; ++q) s_sum[c][q] = 0.0;
        s_cnt[c][0] = s_cnt[c][1] = 0;
    }
    __syncthreads();
    int hits_before = 0, first_hit = -1;
    for (int base = 0; base < p.width; base += 64) {
        const int j = base + lane;
        const int item = j < p.width ? row[j] : -1;
        const bool valid = item >= 0;
        bool hit = false;
        float rel = 0.f;
        if (valid) {                                    // np.in1d(recommended, relevant) (Evaluator.py:323) + it2rel (metrics.py:188-191)
            int lo = t0, hi = t1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (p.test_idx[mid] < item) lo = mid + 1; else hi = mid;
            }
            if (lo < t1 && p.test_idx[lo] == item) { hit = true; rel = p.test_rel[lo]; }
            int bucket = 0;                             // the smallest cutoff holding position j
            while (bucket < p.n_sorted && p.cut_sorted[bucket] <= j) ++bucket;
            atomicAdd(&p.counts[(size_t)bucket * p.n_items + item], 1);
        }
        const unsigned long long hit_mask = __ballot(hit), valid_mask = __ballot(valid);
        const unsigned long long upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);
        const int h_incl = hits_before + __popcll(hit_mask & upto);
        if (first_hit < 0 && hit_mask) first_hit = base + __ffsll((long long)hit_mask) - 1;
        if (j < p.width) {                              // dcg(): (2^rel - 1) / log(position + 2) in float32 (metrics.py:207-209)
            const float num = hit ? (float)exp2((double)rel) - 1.f : 0.f;
            dterm[j] = div_f32(num, p.logs[j]);
        }
        // average_precision (metrics.py:65-74): hits so far (float32 cumsum) / (1 + position), in float64
        const double ap = hit ? (double)(float)h_incl / (double)(j + 1) : 0.0;
        const double rh = hit ? 1.0 / (double)(j + 1) : 0.0;              // arhr (metrics.py:122-133)
        const double nov = valid ? p.novelty[item] : 0.0;
        const double pop = valid ? p.popularity[item] : 0.0;
        for (int c = 0; c < p.n_cut; ++c) {             // (uniform loop: every lane takes part in the wave sums)
            const int lim = min(p.cut[c], p.width);
            if (base >= lim) continue;
            const bool in = j < lim;
            const unsigned long long in_mask = __ballot(in);
            const double s_pos = wave_sum(in && hit ? (double)j : 0.0);
            const double s_ap = wave_sum(in ? ap : 0.0);
            const double s_rh = wave_sum(in ? rh : 0.0);
            const double s_nov = wave_sum(in ? nov : 0.0);
            const double s_pop = wave_sum(in ? pop : 0.0);
            if (lane == 0) {
                s_sum[c][0] += s_pos; s_sum[c][1] += s_ap; s_sum[c][2] += s_rh; s_sum[c][3] += s_nov; s_sum[c][4] += s_pop;
                s_cnt[c][0] += __popcll(valid_mask & in_mask);
                s_cnt[c][1] += __popcll(hit_mask & in_mask);
            }
        }
        hits_before = h_incl;
        hits_before = __shfl(hits_before, 63);
    }
    __syncthreads();
    if (lane != 0) return;
    const int n_test = t1 - t0;
    for (int c = 0; c < p.n_cut; ++c) {
        const int L = s_cnt[c][0], H = s_cnt[c][1], N = L - H;
        double *out = p.vals + ((size_t)pos * p.n_cut + c) * NV;
        // roc_auc (metrics.py:102-118): negatives ranked after each hit, summed as float32 counts, / (hits * negatives)
        float roc = 1.f;
        if (N > 0) {
            const long long after = (long long)H * (L - 1) - (long long)s_sum[c][0] - (long long)H * H + (long long)H * (H + 1) / 2;
            roc = H > 0 ? div_f32((float)after, (float)((long long)H * N)) : 0.f;
        }
        out[V_ROC] = roc;
        out[V_PREC] = L > 0 ? div_f32((float)H, (float)L) : 0.f;                          // precision (metrics.py:136-144)
        out[V_PREC_MIN] = L > 0 ? div_f32((float)H, (float)min(n_test, L)) : 0.f;         // (metrics.py:147-155)
        out[V_RECALL] = div_f32((float)H, (float)n_test);                                 // recall (metrics.py:159-164)
        out[V_AP] = L > 0 ? s_sum[c][1] / (double)min(n_test, L) : 0.0;
        out[V_RR] = first_hit >= 0 && first_hit < L ? 1.0 / (double)(first_hit + 1) : 0.0;   // rr (metrics.py:167-175)
        const float dcg = pairwise_sum<9>(dterm, L);
        out[V_NDCG] = dcg == 0.f ? 0.f : div_f32(dcg, p.idcg[u]);                          // ndcg (metrics.py:180-204)
        out[V_HITS] = H;
        out[V_ARHR] = s_sum[c][2];
        out[V_NOVELTY] = s_sum[c][3];
        out[V_POP] = L > 0 ? s_sum[c][4] / (double)L : 0.0;                                // AveragePopularity (metrics.py:614-621)
        out[V_COVERED] = L > 0;                                                            // Coverage_User (metrics.py:361-362)
    }
}

// sums[col] = sum over users of vals[user][col], in the same order whatever the blocks were
__global__ __launch_bounds__(256) void eval_sum_kernel(const double *vals, int n_eval, int n_cols, double *sums) {
    __shared__ double part[256];
    const int col = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < n_eval; i += 256) s += vals[(size_t)i * n_cols + col];
    part[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) part[t] += part[t + w];
        __syncthreads();
    }
    if (t == 0) sums[col] = part[0];
}

__global__ __launch_bounds__(256) void eval_counts_kernel(int *counts, int n_sorted, int n_items) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    int run = 0;
    for (int b = 0; b < n_sorted; ++b) {
        run += counts[(size_t)b * n_items + i];
        counts[(size_t)b * n_items + i] = run;
    }
}

// np.sum(x, dtype=np.float32) on the host, the same pairwise order as pairwise_sum above
float host_pairwise(const float *a, long n) {
    if (n < 8) {
        float r = 0.f;
        for (long i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128) {
        float r[8];
        for (int k = 0; k < 8; ++k) r[k] = a[k];
        long i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int k = 0; k < 8; ++k) r[k] += a[i + k];
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    long n2 = n / 2;
    n2 -= n2 % 8;
    return host_pairwise(a, n2) + host_pairwise(a + n2, n - n2);
}

}  // namespace
}  // namespace mi355rec

using namespace mi355rec;

struct mi355rec_eval : Handle {
    int n_users = 0, n_items = 0, n_cut = 0, n_sorted = 0, width = 0, n_eval = 0;
    hipEvent_t done = nullptr;          // recorded after every metric launch, on whichever stream ran it
    std::vector<int> cut_host, sorted_host, users_host;
    std::vector<unsigned char> allowed_host;
    bool allowed_valid = false;
    DeviceBuffer<int> cut, cut_sorted, test_ptr, test_idx, users, lists, counts;
    DeviceBuffer<float> test_rel, idcg, logs;
    DeviceBuffer<double> novelty, popularity, vals, sums;
    DeviceBuffer<unsigned char> allowed;
    DeviceBuffer<int> cand_ptr, cand_idx;       // candidate rows of every user (mi355rec_eval_set_candidates)
    int cand_longest = -1;                      // -1: no candidate rows
    DeviceBuffer<unsigned char> div_matrix;     // item diversity matrix, n_items x n_items cells of div_elem bytes (mi355rec_eval_set_diversity)
    DeviceBuffer<unsigned long long> div_bad;
    DeviceBuffer<double> div_vals, div_sums;    // [n_eval][n_cut] per-user values of the evaluation, [n_cut] their sums
    int div_elem = 0;                           // 0: no matrix
    bool div_begun = false, div_finished = false;
    double div_upload_ms = 0.0, div_check_ms = 0.0;

    ~mi355rec_eval() {
        shutdown([&] {
            if (done) { (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
        });
    }
};

namespace {
void check_block(mi355rec_eval *h, int first, int n) {
    MI_REQUIRE(h->n_eval > 0, "mi355rec_eval_begin has not been called");
    MI_REQUIRE(n > 0 && first >= 0 && first + n <= h->n_eval, "block [%d, %d) outside the %d evaluated users", first, first + n, h->n_eval);
}

void launch_metrics(mi355rec_eval *h, hipStream_t s, const int *ranked, int first, int n) {
    EvalParams p{};
    p.n_items = h->n_items; p.width = h->width; p.n_cut = h->n_cut; p.n_sorted = h->n_sorted;
    p.cut = h->cut.ptr; p.cut_sorted = h->cut_sorted.ptr;
    p.test_ptr = h->test_ptr.ptr; p.test_idx = h->test_idx.ptr; p.test_rel = h->test_rel.ptr;
    p.idcg = h->idcg.ptr; p.logs = h->logs.ptr;
    p.novelty = h->novelty.ptr; p.popularity = h->popularity.ptr;
    p.users = h->users.ptr; p.first = first; p.ranked = ranked;
    p.vals = h->vals.ptr; p.counts = h->counts.ptr;
    const int lds = h->width * 4;
    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(eval_metric_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(eval_metric_kernel, dim3(n), dim3(64), lds, s, p);
    MI_HIP(hipGetLastError());
    if (h->div_begun) {
        DivParams d{};
        d.n_items = h->n_items; d.width = h->width; d.n_cut = h->n_cut; d.first = first;
        d.cut = h->cut.ptr; d.ranked = ranked; d.matrix = h->div_matrix.ptr; d.vals = h->div_vals.ptr;
        if (h->div_elem == 4) launch_diversity_typed<float>(d, n, s);
        else launch_diversity_typed<double>(d, n, s);
        MI_HIP(hipGetLastError());
    }
    MI_HIP(hipEventRecord(h->done, s));
}

// the device copy of the item mask, uploaded again only when its contents change (the same mask serves every block)
const unsigned char *device_mask(mi355rec_eval *h, const uint8_t *allowed) {
    if (!allowed) return nullptr;
    if (!h->allowed_valid || std::memcmp(h->allowed_host.data(), allowed, h->n_items) != 0) {
        MI_HIP(hipEventSynchronize(h->done));           // (a block still running may read the old mask)
        h->allowed_host.assign(allowed, allowed + h->n_items);
        MI_HIP(hipMemcpy(h->allowed.ptr, allowed, h->n_items, hipMemcpyHostToDevice));
        h->allowed_valid = true;
    }
    return h->allowed.ptr;
}

// A block of users through a scorer: its lists stay in HBM.  `rows`: rank the candidate rows only (negative-sample evaluation).
void add_from_scorer(mi355rec_eval *h, ScorerHandle *sc, int first, int n, int remove_seen, const uint8_t *allowed,
                     const CandidateRows *rows = nullptr) {
    MI_REQUIRE(h && sc, "NULL argument");
    check_block(h, first, n);
    const int su = sc->n_users, si = sc->n_items;
    MI_REQUIRE(si == h->n_items, "the recommender scores %d items, URM_test has %d", si, h->n_items);
    for (int i = first; i < first + n; ++i)
        MI_REQUIRE(h->users_host[i] < su, "Cold users not allowed. Users in trained model are %d, requested prediction for user %d",
                   su, h->users_host[i]);
    ensure_device();
    const unsigned char *mask = device_mask(h, allowed);
    MI_HIP(hipStreamWaitEvent(sc->stream, h->done, 0)); // (begin's zeroing, a lists-path block on the evaluator's stream)
    const int *users = h->users.ptr + first;
    const Ranking r = rows ? sc->enqueue_candidates(users, n, h->width, remove_seen, mask, *rows)
                           : sc->enqueue(users, n, h->width, remove_seen, mask, false);
    launch_metrics(h, r.stream, r.ranked, first, n);    // behind the ranking, on the scorer's stream: the next block's ranking
}                                                       // cannot overwrite `ranked` before this kernel has read it

// Negative-sample evaluation (Evaluator.py:455-539, EvaluatorNegativeItemSample): every user ranks the candidates of its row only.
void add_from_scorer_candidates(mi355rec_eval *h, ScorerHandle *sc, int first, int n, int remove_seen, const uint8_t *allowed) {
    MI_REQUIRE(h, "NULL argument");
    MI_REQUIRE(h->cand_longest >= 0, "mi355rec_eval_set_candidates has not been called");
    const CandidateRows rows{h->cand_ptr.ptr, h->cand_idx.ptr, true, h->cand_longest};
    add_from_scorer(h, sc, first, n, remove_seen, allowed, &rows);
}
}  // namespace

extern "C" int mi355rec_eval_create(mi355rec_eval_t *out, int32_t n_users, int32_t n_items, const int32_t *test_indptr,
                                    const int32_t *test_indices, const double *test_relevance, const int32_t *cutoffs,
                                    int32_t n_cutoffs, const float *log_table, int32_t log_len) {
    return guarded([&] {
        MI_REQUIRE(out && test_indptr && test_indices && test_relevance && cutoffs && log_table, "NULL argument");
        MI_REQUIRE(n_users > 0 && n_items > 0, "empty URM_test");
        MI_REQUIRE(n_cutoffs > 0 && n_cutoffs <= MAX_CUTOFFS, "between 1 and %d cutoffs", MAX_CUTOFFS);
        std::unique_ptr<mi355rec_eval> h(new mi355rec_eval());
        h->n_users = n_users; h->n_items = n_items; h->n_cut = n_cutoffs;
        h->cut_host.assign(cutoffs, cutoffs + n_cutoffs);
        for (int c : h->cut_host) MI_REQUIRE(c >= 1, "cutoffs must be positive");
        h->sorted_host = h->cut_host;
        std::sort(h->sorted_host.begin(), h->sorted_host.end());
        MI_REQUIRE(std::adjacent_find(h->sorted_host.begin(), h->sorted_host.end()) == h->sorted_host.end(), "repeated cutoff");
        h->n_sorted = n_cutoffs;
        h->width = std::min(h->sorted_host.back(), n_items);
        if (h->width > MAX_WIDTH) fail(MI355REC_E_UNSUPPORTED, "lists of %d entries: at most %d", h->width, MAX_WIDTH);
        // test rows sorted by item id, relevance permuted along; ideal DCG of all ratings, descending (metrics.py:194, 207-209)
        const size_t nnz = (size_t)test_indptr[n_users];
        std::vector<int> idx(test_indices, test_indices + nnz);
        std::vector<float> rel(nnz), idcg(n_users);
        std::vector<std::pair<int, double>> pairs;
        std::vector<double> desc;
        std::vector<float> terms;
        int longest = 0;
        for (int u = 0; u < n_users; ++u) longest = std::max(longest, test_indptr[u + 1] - test_indptr[u]);
        MI_REQUIRE(log_len >= std::max(longest, h->width), "log_table needs %d entries", std::max(longest, h->width));
        for (int u = 0; u < n_users; ++u) {
            const int a = test_indptr[u], e = test_indptr[u + 1];
            MI_REQUIRE(a <= e, "test indptr is not monotone");
            pairs.clear(); desc.clear(); terms.clear();
            for (int q = a; q < e; ++q) {
                MI_REQUIRE(test_indices[q] >= 0 && test_indices[q] < n_items, "test item id %d out of range", test_indices[q]);
                pairs.emplace_back(test_indices[q], test_relevance[q]);
                desc.push_back(test_relevance[q]);
            }
            std::sort(pairs.begin(), pairs.end(), [](const std::pair<int, double> &x, const std::pair<int, double> &y) { return x.first < y.first; });
            for (int q = a; q < e; ++q) { idx[q] = pairs[q - a].first; rel[q] = (float)pairs[q - a].second; }
            std::sort(desc.begin(), desc.end(), [](double x, double y) { return x > y; });
            for (size_t q = 0; q < desc.size(); ++q) terms.push_back((float)((std::pow(2.0, desc[q]) - 1.0) / (double)log_table[q]));
            idcg[u] = host_pairwise(terms.data(), (long)terms.size());
        }
        ensure_device();
        h->open(0);
        MI_HIP(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
        hipStream_t s = h->stream;
        h->cut.upload(h->cut_host.data(), n_cutoffs, s);
        h->cut_sorted.upload(h->sorted_host.data(), n_cutoffs, s);
        h->test_ptr.upload(test_indptr, (size_t)n_users + 1, s);
        h->test_idx.upload(idx.data(), nnz, s);
        h->test_rel.upload(rel.data(), nnz, s);
        h->idcg.upload(idcg.data(), n_users, s);
        h->logs.upload(log_table, h->width, s);
        h->allowed.alloc(n_items);
        MI_HIP(hipStreamSynchronize(s));
        MI_HIP(hipEventRecord(h->done, s));
        *out = h.release();
    });
}

extern "C" int mi355rec_eval_begin(mi355rec_eval_t h, const double *novelty_term, const double *popularity_term, const int32_t *user_ids,
                                   int32_t n_eval) {
    return guarded([&] {
        MI_REQUIRE(h && novelty_term && popularity_term && user_ids, "NULL argument");
        MI_REQUIRE(n_eval > 0, "no users to evaluate");
        for (int i = 0; i < n_eval; ++i) MI_REQUIRE(user_ids[i] >= 0 && user_ids[i] < h->n_users, "user id %d out of range", user_ids[i]);
        ensure_device();
        hipStream_t s = h->stream;
        MI_HIP(hipEventSynchronize(h->done));           // (the previous evaluation's last block)
        h->n_eval = n_eval;
        h->users_host.assign(user_ids, user_ids + n_eval);
        h->users.upload(user_ids, n_eval, s);
        h->novelty.upload(novelty_term, h->n_items, s);
        h->popularity.upload(popularity_term, h->n_items, s);
        h->vals.alloc_zero((size_t)n_eval * h->n_cut * NV, s);
        h->counts.alloc_zero((size_t)h->n_sorted * h->n_items, s);
        h->div_begun = h->div_elem != 0;
        h->div_finished = false;
        if (h->div_begun) h->div_vals.alloc_zero(evalplan::div_value_cells(n_eval, h->n_cut), s);
        MI_HIP(hipStreamSynchronize(s));
        MI_HIP(hipEventRecord(h->done, s));
    });
}

extern "C" int mi355rec_eval_add_lists(mi355rec_eval_t h, int32_t first, int32_t n, const int32_t *ranked) {
    return guarded([&] {
        MI_REQUIRE(h && ranked, "NULL argument");
        check_block(h, first, n);
        for (int b = 0; b < n; ++b) {
            const int32_t *row = ranked + (size_t)b * h->width;
            bool ended = false;
            for (int j = 0; j < h->width; ++j) {
                if (row[j] == -1) { ended = true; continue; }
                MI_REQUIRE(!ended, "list %d: an item follows the -1 padding", first + b);
                MI_REQUIRE(row[j] >= 0 && row[j] < h->n_items, "list %d: item id %d outside [0, %d)", first + b, row[j], h->n_items);
            }
        }
        ensure_device();
        hipStream_t s = h->stream;
        MI_HIP(hipStreamWaitEvent(s, h->done, 0));
        if (h->lists.count < (size_t)n * h->width) {
            MI_HIP(hipStreamSynchronize(s));
            h->lists.alloc((size_t)n * h->width);
        }
        MI_HIP(hipMemcpyAsync(h->lists.ptr, ranked, sizeof(int) * (size_t)n * h->width, hipMemcpyHostToDevice, s));
        launch_metrics(h, s, h->lists.ptr, first, n);
        MI_HIP(hipStreamSynchronize(s));                // (the host lists may go away when this returns)
    });
}

// One entry point per scorer type: the typed pointer of the C header is what keeps a wrong handle out.
extern "C" int mi355rec_eval_add_scorer(mi355rec_eval_t h, mi355rec_scorer_t scorer, int32_t first, int32_t n, int32_t remove_seen,
                                        const uint8_t *item_allowed) {
    return guarded([&] { add_from_scorer(h, scorer, first, n, remove_seen, item_allowed); });
}

extern "C" int mi355rec_eval_add_spscorer(mi355rec_eval_t h, mi355rec_spscorer_t scorer, int32_t first, int32_t n, int32_t remove_seen,
                                          const uint8_t *item_allowed) {
    return guarded([&] { add_from_scorer(h, scorer, first, n, remove_seen, item_allowed); });
}

extern "C" int mi355rec_eval_add_itemscorer(mi355rec_eval_t h, mi355rec_itemscorer_t scorer, int32_t first, int32_t n, int32_t remove_seen,
                                            const uint8_t *item_allowed) {
    return guarded([&] { add_from_scorer(h, scorer, first, n, remove_seen, item_allowed); });
}

extern "C" int mi355rec_eval_add_dscorer(mi355rec_eval_t h, mi355rec_dscorer_t scorer, int32_t first, int32_t n, int32_t remove_seen,
                                         const uint8_t *item_allowed) {
    return guarded([&] { add_from_scorer(h, scorer, first, n, remove_seen, item_allowed); });
}

extern "C" int mi355rec_eval_set_candidates(mi355rec_eval_t h, const int32_t *indptr, const int32_t *indices) {
    return guarded([&] {
        MI_REQUIRE(h && indptr, "NULL argument");
        check_candidate_cutoff(h->width);
        const int longest = check_candidate_rows(indptr, indices, h->n_users, h->n_items);
        ensure_device();
        hipStream_t s = h->stream;
        MI_HIP(hipEventSynchronize(h->done));           // (a block still running may read the old rows)
        h->cand_longest = -1;
        const size_t nnz = (size_t)indptr[h->n_users];
        h->cand_ptr.upload(indptr, (size_t)h->n_users + 1, s);
        if (nnz) h->cand_idx.upload(indices, nnz, s);
        else h->cand_idx.alloc(1);
        MI_HIP(hipStreamSynchronize(s));
        h->cand_longest = longest;
    });
}

extern "C" int mi355rec_eval_add_scorer_candidates(mi355rec_eval_t h, mi355rec_scorer_t scorer, int32_t first, int32_t n,
                                                   int32_t remove_seen, const uint8_t *item_allowed) {
    return guarded([&] { add_from_scorer_candidates(h, scorer, first, n, remove_seen, item_allowed); });
}

extern "C" int mi355rec_eval_add_spscorer_candidates(mi355rec_eval_t h, mi355rec_spscorer_t scorer, int32_t first, int32_t n,
                                                     int32_t remove_seen, const uint8_t *item_allowed) {
    return guarded([&] { add_from_scorer_candidates(h, scorer, first, n, remove_seen, item_allowed); });
}

extern "C" int mi355rec_eval_add_itemscorer_candidates(mi355rec_eval_t h, mi355rec_itemscorer_t scorer, int32_t first, int32_t n,
                                                       int32_t remove_seen, const uint8_t *item_allowed) {
    return guarded([&] { add_from_scorer_candidates(h, scorer, first, n, remove_seen, item_allowed); });
}

extern "C" int mi355rec_eval_add_dscorer_candidates(mi355rec_eval_t h, mi355rec_dscorer_t scorer, int32_t first, int32_t n,
                                                    int32_t remove_seen, const uint8_t *item_allowed) {
    return guarded([&] { add_from_scorer_candidates(h, scorer, first, n, remove_seen, item_allowed); });
}

extern "C" int mi355rec_eval_finish(mi355rec_eval_t h, double *sums, int32_t *item_counts) {
    return guarded([&] {
        MI_REQUIRE(h && sums && item_counts, "NULL argument");
        MI_REQUIRE(h->n_eval > 0, "mi355rec_eval_begin has not been called");
        ensure_device();
        hipStream_t s = h->stream;
        MI_HIP(hipStreamWaitEvent(s, h->done, 0));
        if (h->sums.count < (size_t)h->n_cut * NV) h->sums.alloc((size_t)h->n_cut * NV);
        hipLaunchKernelGGL(eval_sum_kernel, dim3(h->n_cut * NV), dim3(256), 0, s, h->vals.ptr, h->n_eval, h->n_cut * NV, h->sums.ptr);
        hipLaunchKernelGGL(eval_counts_kernel, dim3(div_up(h->n_items, 256)), dim3(256), 0, s, h->counts.ptr, h->n_sorted, h->n_items);
        if (h->div_begun) {
            if (h->div_sums.count < (size_t)h->n_cut) h->div_sums.alloc(h->n_cut);
            hipLaunchKernelGGL(eval_sum_kernel, dim3(h->n_cut), dim3(256), 0, s, h->div_vals.ptr, h->n_eval, h->n_cut, h->div_sums.ptr);
        }
        MI_HIP(hipGetLastError());
        std::vector<int> sorted_counts((size_t)h->n_sorted * h->n_items);
        h->sums.download(sums, (size_t)h->n_cut * NV, s);
        h->counts.download(sorted_counts.data(), sorted_counts.size(), s);
        MI_HIP(hipStreamSynchronize(s));
        MI_HIP(hipEventRecord(h->done, s));
        h->div_finished = h->div_begun;
        for (int c = 0; c < h->n_cut; ++c) {            // (bucket rows are in ascending cutoff order, the output in the given one)
            const int b = (int)(std::lower_bound(h->sorted_host.begin(), h->sorted_host.end(), h->cut_host[c]) - h->sorted_host.begin());
            std::memcpy(item_counts + (size_t)c * h->n_items, sorted_counts.data() + (size_t)b * h->n_items, sizeof(int) * h->n_items);
        }
    });
}

extern "C" int mi355rec_eval_get_per_user(mi355rec_eval_t h, double *out) {
    return guarded([&] {
        MI_REQUIRE(h && out, "NULL argument");
        MI_REQUIRE(h->n_eval > 0, "mi355rec_eval_begin has not been called");
        ensure_device();
        MI_HIP(hipEventSynchronize(h->done));
        MI_HIP(hipMemcpy(out, h->vals.ptr, sizeof(double) * (size_t)h->n_eval * h->n_cut * NV, hipMemcpyDeviceToHost));
    });
}

// The item diversity matrix of DIVERSITY_SIMILARITY: uploaded in chunks, its range checked by a device reduction.  It takes effect with
// the next mi355rec_eval_begin.
extern "C" int mi355rec_eval_set_diversity(mi355rec_eval_t h, const void *matrix, int32_t elem_bytes) {
    return guarded([&] {
        using namespace evalplan;
        using clock = std::chrono::steady_clock;
        const auto ms = [](clock::time_point a, clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        MI_REQUIRE(h, "NULL argument");
        ensure_device();
        hipStream_t s = h->stream;
        if (!matrix) {
            MI_HIP(hipEventSynchronize(h->done));       // (a block still running may read the matrix)
            h->div_elem = 0;
            h->div_begun = h->div_finished = false;     // (an evaluation under way goes on without the metric)
            h->div_matrix.release();
            return;
        }
        MI_REQUIRE(div_elem_ok(elem_bytes), "item diversity matrix cells of %d bytes: 4 (float32) or 8 (float64)", elem_bytes);
        if (!div_width_ok(h->width))
            fail(MI355REC_E_UNSUPPORTED, "DIVERSITY_SIMILARITY on lists of %d entries: at most %d", h->width, DIV_MAX_WIDTH);
        MI_HIP(hipEventSynchronize(h->done));
        h->div_elem = 0;
        h->div_begun = h->div_finished = false;
        const uint64_t cells = div_matrix_cells(h->n_items), bytes = div_matrix_bytes(h->n_items, elem_bytes);
        const auto t0 = clock::now();
        if (h->div_matrix.count != bytes) h->div_matrix.alloc(bytes);
        for (uint64_t c = 0; c < div_upload_chunks(bytes); ++c) {
            const uint64_t at = c * DIV_UPLOAD_CHUNK, n = std::min<uint64_t>(DIV_UPLOAD_CHUNK, bytes - at);
            MI_HIP(hipMemcpyAsync(h->div_matrix.ptr + at, static_cast<const unsigned char *>(matrix) + at, n, hipMemcpyHostToDevice, s));
        }
        MI_HIP(hipStreamSynchronize(s));
        const auto t1 = clock::now();
        h->div_bad.alloc_zero(1, s);
        if (elem_bytes == 4)
            hipLaunchKernelGGL(eval_diversity_range_kernel<float>, dim3(div_range_blocks(cells)), dim3(256), 0, s,
                               reinterpret_cast<const float *>(h->div_matrix.ptr), (unsigned long long)cells, h->div_bad.ptr);
        else
            hipLaunchKernelGGL(eval_diversity_range_kernel<double>, dim3(div_range_blocks(cells)), dim3(256), 0, s,
                               reinterpret_cast<const double *>(h->div_matrix.ptr), (unsigned long long)cells, h->div_bad.ptr);
        MI_HIP(hipGetLastError());
        unsigned long long bad = 0;
        h->div_bad.download(&bad, 1, s);
        MI_HIP(hipStreamSynchronize(s));
        MI_HIP(hipEventRecord(h->done, s));
        h->div_upload_ms = ms(t0, t1);
        h->div_check_ms = ms(t1, clock::now());
        if (bad) {
            h->div_matrix.release();
            fail(MI355REC_E_INVALID, "item_diversity_matrix contains value greater than 1.0 or lower than 0.0: %llu cells (NaN included)", bad);
        }
        h->div_elem = elem_bytes;
    });
}

extern "C" int mi355rec_eval_get_diversity(mi355rec_eval_t h, double *sums, double *per_user) {
    return guarded([&] {
        MI_REQUIRE(h && sums, "NULL argument");
        MI_REQUIRE(h->div_finished, "mi355rec_eval_finish has not been called on an evaluation with an item diversity matrix");
        ensure_device();
        MI_HIP(hipEventSynchronize(h->done));
        MI_HIP(hipMemcpy(sums, h->div_sums.ptr, sizeof(double) * (size_t)h->n_cut, hipMemcpyDeviceToHost));
        if (per_user)
            MI_HIP(hipMemcpy(per_user, h->div_vals.ptr, sizeof(double) * evalplan::div_value_cells(h->n_eval, h->n_cut), hipMemcpyDeviceToHost));
    });
}

extern "C" int mi355rec_eval_diversity_info(mi355rec_eval_t h, int32_t *elem_bytes, double *upload_ms, double *check_ms) {
    return guarded([&] {
        MI_REQUIRE(h && elem_bytes && upload_ms && check_ms, "NULL argument");
        *elem_bytes = h->div_elem;
        *upload_ms = h->div_upload_ms;
        *check_ms = h->div_check_ms;
    });
}

extern "C" void mi355rec_eval_destroy(mi355rec_eval_t h) { handle_destroy(h); }
