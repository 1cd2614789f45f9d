// score.h -- the scorer handles (factor, sparse-similarity and -- densescore.hip -- dense-similarity models) and the "score + rank on
// the handle's stream" half of mi355rec_scorer_recommend / mi355rec_spscorer_recommend (score.hip) and mi355rec_dscorer_recommend
// (densescore.hip), shared with the holdout evaluator (eval.hip), whose metric kernel reads the ranked lists
// where these leave them; and the same for candidate rows (cand.hip: mi355rec_*scorer_recommend_candidates, the negative-sample
// evaluator).
#pragma once

#include "common.h"

namespace mi355rec {

// ranking of score rows that stay in HBM (score.hip, "wide ranking")
struct WideRanker {
    DeviceBuffer<int> ids_in, ids_out, offsets;
    DeviceBuffer<float> keys_out;
    DeviceBuffer<unsigned char> tmp;
    size_t capacity = 0;
    int offsets_n = 0, offsets_items = 0;

    // scores: [n][n_items] in HBM (unfiltered); ranked: [n][cutoff] on the device
    void rank(hipStream_t s, float *scores, int n, int n_items, int cutoff, const int *users, const int *seen_ptr, const int *seen_idx,
              const unsigned char *allowed, int remove_seen, int *ranked);
};

// what the two scorers share: mi355rec_*scorer_recommend and the evaluator's add_from_scorer are written against these members
struct ScorerHandle : Handle {
    WideRanker wide;
    int n_users = 0, n_items = 0;       // rows that can be asked for, width of a score row
    DeviceBuffer<int> seen_ptr, seen_idx, users, ranked;
    DeviceBuffer<int> cand_ptr, cand_idx;   // the candidate rows of the last mi355rec_*scorer_recommend_candidates
    DeviceBuffer<float> scores;
    DeviceBuffer<unsigned char> allowed;
};

}  // namespace mi355rec

struct mi355rec_scorer : mi355rec::ScorerHandle {    // `timer`: the GEMM dispatch; `call_timer`: GEMM + ranking
    int k = 0, use_bias = 0;
    float mu = 0.f;
    mi355rec::DeviceBuffer<float> U, V, bu, bi;

    ~mi355rec_scorer() { shutdown(); }
};

struct mi355rec_spscorer : mi355rec::ScorerHandle {  // `timer`: the scoring dispatch
    int n_mid = 0;
    mi355rec::DeviceBuffer<int> a_ptr, a_idx, b_ptr, b_idx;
    mi355rec::DeviceBuffer<float> a_val, b_val;
    double nnz_a = 0, nnz_b = 0;

    ~mi355rec_spscorer() { shutdown(); }
};

struct mi355rec_dscorer : mi355rec::ScorerHandle {   // densescore.hip.  `timer`: the scoring dispatch; `call_timer`: scoring + ranking
    int n_mid = 0, unroll = 0;
    int64_t ldb = 0;                                 // floats between two rows of B (n_items rounded up to 4)
    mi355rec::DeviceBuffer<int> a_ptr, a_idx;        // A as stored: the order of a row's cells is the order of the sum
    mi355rec::DeviceBuffer<float> a_val, B;
    std::vector<int> a_ptr_host;                     // (the stats count the stored cells of a batch's profiles)

    ~mi355rec_dscorer() { shutdown(); }
};

namespace mi355rec {

struct Ranking {
    const int *ranked;      // [n][cutoff] on the device, -1 padded; valid until the next enqueue on the same handle
    hipStream_t stream;     // the handle's stream: the work above is queued there, nothing has been waited for
};

// users: n device user ids; allowed: nullable device mask of n_items bytes; keep_scores: leave the filtered score rows in the
// handle's score buffer (the public functions' return_scores).
Ranking scorer_enqueue(mi355rec_scorer_t h, const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                       bool keep_scores);
Ranking spscorer_enqueue(mi355rec_spscorer_t h, const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                         bool keep_scores);
Ranking dscorer_enqueue(mi355rec_dscorer_t h, const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                        bool keep_scores);
// What a scorer that writes full score rows itself (densescore.hip) takes from score.hip (host functions): room for n rows of
// h->scores and n lists of h->ranked (grown after the stream has drained), and scorer_enqueue's filter + ranking of those rows --
// score_rank_kernel where score_row_fits_lds, the WideRanker otherwise; keep_scores leaves the filtered rows in h->scores.
void grow_score_rows(ScorerHandle *h, int n, int cutoff);
void rank_rows_enqueue(ScorerHandle *h, const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                       bool keep_scores);
// ease.hip: the weights W = P / (-diag P) of an inverted matrix where they stand in HBM (n x n floats, row pitch *ld), scaled now if
// they were not yet; returns with the handle's stream drained.  MI355REC_E_INVALID without a successful invert.
void ease_weights_device(mi355rec_ease *h, const float **W, int64_t *ld, int *n);
// ---- candidate rows: each user ranks a short list of items of its own (Evaluator.py:455-539, EvaluatorNegativeItemSample) ----------
constexpr int CAND_MAX = 4096;          // longest candidate row: one block_rank_emit (topk.cuh) over the whole row

// a CSR of candidate rows on the device, item ids strictly ascending inside a row (check_candidate_rows)
struct CandidateRows {
    const int *ptr, *idx;
    bool by_user;           // the row of batch entry b is users[b] (one row per user of the model), not b
    int longest;            // entries of the longest row (sizes the LDS candidate buffer)
};

// Host check of a candidate CSR: monotone indptr starting at 0, ids inside [0, n_items) and strictly ascending in every row
// (MI355REC_E_INVALID), no row longer than CAND_MAX (MI355REC_E_UNSUPPORTED).  Returns the length of the longest row.
int check_candidate_rows(const int32_t *indptr, const int32_t *indices, int n_rows, int n_items);
void check_candidate_cutoff(int cutoff);    // a list wider than MAX_TOPK (topk.cuh) is MI355REC_E_UNSUPPORTED: the one place that says so

// scorer_enqueue / spscorer_enqueue over candidate rows: only a user's candidates are ranked (value descending, ties towards the
// lower item id), after the same seen / mask filters.  The factor scorer computes U[u] . V[c] for the candidates alone -- no GEMM, no
// score matrix; the sparse scorer accumulates its row as before and gathers the candidates from it.  `timer` spans the candidate
// kernel(s) (mi355rec_*scorer_recommend_candidates reports it as kernel_ms and call_ms); `call_timer` is not used.
Ranking scorer_enqueue_candidates(mi355rec_scorer_t h, const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                                  const CandidateRows &rows);
Ranking spscorer_enqueue_candidates(mi355rec_spscorer_t h, const int *users, int n, int cutoff, int remove_seen,
                                    const unsigned char *allowed, const CandidateRows &rows);
Ranking dscorer_enqueue_candidates(mi355rec_dscorer_t h, const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                                   const CandidateRows &rows);
// what cand.hip takes from score.hip (host functions): whether a score row of n_items floats is ranked in LDS at this cutoff, and
// spscorer_enqueue's accumulation of rows that are not -- h->scores[b][n_items] = A[users[b], :] . B, zeroed first, unfiltered, not
// ranked; the caller has grown h->scores.
bool score_row_fits_lds(int n_items, int cutoff);
void spscorer_enqueue_wide_rows(mi355rec_spscorer_t h, const int *users, int n);
// C[b][j] = A[rows[b]] . Bt[j] for b < n, j < m (A: rows of k floats, Bt: m x k, C: n x m, all row-major on the device): the scorer's
// f32 MFMA GEMM without biases, queued on `s`.  n <= 128 * 65535.
void gemm_rows_enqueue(const float *A, const int *rows, int n, int k, const float *Bt, int m, float *C, hipStream_t s);

}  // namespace mi355rec
