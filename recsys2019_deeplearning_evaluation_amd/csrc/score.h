// score.h -- the scorer handles (factor, sparse-similarity and -- densescore.hip -- dense-similarity models; itemscore.h adds the shared
// item vector) and their one interface, ScorerHandle: `enqueue` and `enqueue_candidates` put "score + rank" on the handle's stream and
// leave the lists in `ranked`.  The public mi355rec_*scorer_recommend[_candidates] (recommend / recommend_candidates below) and the
// holdout evaluators (eval.hip: add_from_scorer, whose metric kernel reads the lists where they stand) are written against it.
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

struct Ranking {
    const int *ranked;      // [n][cutoff] on the device, -1 padded; valid until the next enqueue on the same handle
    hipStream_t stream;     // the handle's stream: the work above is queued there, nothing has been waited for
};

// ---- candidate rows: each user ranks a short list of items of its own (Evaluator.py:455-539, EvaluatorNegativeItemSample) ----------
constexpr int CAND_MAX = 4096;          // longest candidate row: one block_rank_emit (topk.cuh) over the whole row

// a CSR of candidate rows on the device, item ids strictly ascending inside a row (check_candidate_rows)
struct CandidateRows {
    const int *ptr, *idx;
    bool by_user;           // the row of batch entry b is users[b] (one row per user of the model), not b
    int longest;            // entries of the longest row (sizes the LDS candidate buffer)
};

// What every scorer is: recommend / recommend_candidates and the evaluator's add_from_scorer see these members only.  The members
// are defined next to the scorer's kernels (score.hip, cand.hip, densescore.hip, itemscore.hip).
struct ScorerHandle : Handle {
    WideRanker wide;
    int n_users = 0, n_items = 0;       // rows that can be asked for, width of a score row
    DeviceBuffer<int> seen_ptr, seen_idx, users, ranked;
    DeviceBuffer<int> cand_ptr, cand_idx;   // the candidate rows of the last mi355rec_*scorer_recommend_candidates
    DeviceBuffer<float> scores;
    DeviceBuffer<unsigned char> allowed;

    // Score + rank, enqueued on the handle's stream.  users: n device user ids; allowed: nullable device mask of n_items bytes;
    // keep_scores: leave the filtered score rows in `scores` (the public functions' return_scores).
    virtual Ranking enqueue(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed, bool keep_scores) = 0;
    // The same over candidate rows: only a user's candidates are ranked (value descending, ties towards the lower item id), after
    // the same seen / mask filters, and no n x n_items score matrix is kept unless the rows have to be accumulated in HBM.  `timer`
    // spans the candidate kernel(s) (recommend_candidates reports it as kernel_ms and call_ms); `call_timer` is not used.
    virtual Ranking enqueue_candidates(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                                       const CandidateRows &rows) = 0;
    // the scorer's own complaint about a user id outside [0, n_users): "user id %d out of range" unless overridden
    [[noreturn]] virtual void bad_user(int user) const;
    [[noreturn]] void cold_user(int user) const;    // the reference's "Cold users not allowed..." (factor and item-vector models)
    // the stats of a finished recommend() that depend on the scorer: its timers, its flops and bytes
    virtual void fill_recommend_stats(const int32_t *user_ids, int n) = 0;

    // Room for that many cells of `ranked` and `scores`.  Buffers only grow after the stream has drained: a caller that does not
    // synchronise between blocks -- the holdout evaluator -- may still have kernels reading the old ones.  `wide_cells` is what the
    // WideRanker is about to be asked for (0: nothing): it grows its own buffers, and is drained for here as well.
    void reserve(size_t ranked_cells, size_t score_cells, size_t wide_cells);

protected:
    ~ScorerHandle() = default;          // (handle_destroy deletes through the exact type)
};

}  // namespace mi355rec

struct mi355rec_scorer final : mi355rec::ScorerHandle {      // `timer`: the GEMM dispatch; `call_timer`: GEMM + ranking
    int k = 0, use_bias = 0;
    float mu = 0.f;
    mi355rec::DeviceBuffer<float> U, V, bu, bi;

    mi355rec::Ranking enqueue(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed, bool keep_scores) override;
    // U[u] . V[c] for the candidates alone (cand.hip): no GEMM, no score matrix
    mi355rec::Ranking enqueue_candidates(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                                         const mi355rec::CandidateRows &rows) override;
    [[noreturn]] void bad_user(int user) const override { cold_user(user); }
    void fill_recommend_stats(const int32_t *user_ids, int n) override;
    ~mi355rec_scorer() { shutdown(); }
};

struct mi355rec_spscorer final : mi355rec::ScorerHandle {    // `timer`: the scoring dispatch
    int n_mid = 0;
    int exact = 0;                                   // mi355rec_spscorer_set_exact: both enqueues go through spexact.hip
    mi355rec::DeviceBuffer<int> a_ptr, a_idx, b_ptr, b_idx;
    mi355rec::DeviceBuffer<int> cuts;               // exact mode: where every row of B crosses into each slice of a score row
    mi355rec::DeviceBuffer<float> a_val, b_val;
    // What a new B is written into (update_b, update_from_slim): swapped with b_ptr / b_idx / b_val once the new B has been accepted,
    // never before -- so they then hold the B that was replaced, and serve the next call.  After the first replacement b_idx and
    // b_val may be larger than B: nnz_b, not their count, says how many cells B has.
    mi355rec::DeviceBuffer<int> spare_ptr, spare_idx;
    mi355rec::DeviceBuffer<float> spare_val;
    double nnz_a = 0, nnz_b = 0;

    mi355rec::Ranking enqueue(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed, bool keep_scores) override;
    // the row is accumulated as before and the candidates are gathered from it (cand.hip)
    mi355rec::Ranking enqueue_candidates(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                                         const mi355rec::CandidateRows &rows) override;
    void fill_recommend_stats(const int32_t *user_ids, int n) override;
    ~mi355rec_spscorer() { shutdown(); }
};

struct mi355rec_dscorer final : mi355rec::ScorerHandle {     // densescore.hip.  `timer`: the scoring dispatch; `call_timer`: scoring + ranking
    int n_mid = 0, unroll = 0;
    int64_t ldb = 0;                                 // floats between two rows of B (n_items rounded up to 4)
    mi355rec::DeviceBuffer<int> a_ptr, a_idx;        // A as stored: the order of a row's cells is the order of the sum
    mi355rec::DeviceBuffer<float> a_val, B;
    std::vector<int> a_ptr_host;                     // (the stats count the stored cells of a batch's profiles)

    mi355rec::Ranking enqueue(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed, bool keep_scores) override;
    mi355rec::Ranking enqueue_candidates(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                                         const mi355rec::CandidateRows &rows) override;
    void fill_recommend_stats(const int32_t *user_ids, int n) override;
    ~mi355rec_dscorer() { shutdown(); }
};

namespace mi355rec {

// The bodies of mi355rec_*scorer_recommend (score.hip) and mi355rec_*scorer_recommend_candidates (cand.hip; row r of the candidate
// CSR belongs to user_ids[r]): the arguments are checked, user ids, candidate rows and the item mask go up, the scorer enqueues,
// the lists (and the score rows, when asked for) come down, the stats of the call are filled in.
void recommend(ScorerHandle *h, const int32_t *user_ids, int n, int cutoff, int remove_seen, const uint8_t *item_allowed, int32_t *ranked,
               float *scores);
void recommend_candidates(ScorerHandle *h, const int32_t *user_ids, int n, const int32_t *cand_indptr, const int32_t *cand_indices,
                          int cutoff, int remove_seen, const uint8_t *item_allowed, int32_t *ranked);

// What a scorer that writes full score rows itself (densescore.hip) takes from score.hip (a host function): the factor scorer's
// filter + ranking of h->scores[n][n_items] -- score_rank_kernel where score_row_fits_lds, the WideRanker otherwise; keep_scores
// leaves the filtered rows in h->scores.  The caller has reserved the rows and the lists.
void rank_rows_enqueue(ScorerHandle *h, const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                       bool keep_scores);
// ease.hip: the weights W = P / (-diag P) of an inverted matrix where they stand in HBM (n x n floats, row pitch *ld), scaled now if
// they were not yet; returns with the handle's stream drained.  MI355REC_E_INVALID without a successful invert.
void ease_weights_device(mi355rec_ease *h, const float **W, int64_t *ld, int *n);

// Host check of a candidate CSR: monotone indptr starting at 0, ids inside [0, n_items) and strictly ascending in every row
// (MI355REC_E_INVALID), no row longer than CAND_MAX (MI355REC_E_UNSUPPORTED).  Returns the length of the longest row.
int check_candidate_rows(const int32_t *indptr, const int32_t *indices, int n_rows, int n_items);
void check_candidate_cutoff(int cutoff);    // a list wider than MAX_TOPK (topk.cuh) is MI355REC_E_UNSUPPORTED: the one place that says so

// what cand.hip takes from score.hip (host functions): whether a score row of n_items floats is ranked in LDS at this cutoff, and
// mi355rec_spscorer::enqueue's accumulation of rows that are not -- h->scores[b][n_items] = A[users[b], :] . B, zeroed first,
// unfiltered, not ranked; the caller has reserved h->scores.
bool score_row_fits_lds(int n_items, int cutoff);
void spscorer_enqueue_wide_rows(mi355rec_spscorer_t h, const int *users, int n);
// spexact.hip: what mi355rec_spscorer's two enqueues do in exact mode (h->exact) -- the rows bit for bit SciPy's, written to
// h->scores without an atomic, then rank_rows_enqueue, or the candidates gathered from them.
Ranking spexact_enqueue(mi355rec_spscorer_t h, const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                        bool keep_scores);
Ranking spexact_enqueue_candidates(mi355rec_spscorer_t h, const int *users, int n, int cutoff, int remove_seen,
                                   const unsigned char *allowed, const CandidateRows &rows);
// spexact.hip: the pass of exact mode over a B on the device (b_ptr, b_idx: the live buffers, or the spare ones of a B that is about to
// be swapped in), queued on `s`: every row's ids strictly ascending inside [0, n_items) -- MI355REC_E_INVALID naming the first row that
// is not -- and, where `cuts` is given, the table of that B into it.  Returns with `s` drained.  The table is a function of B:
// whoever replaces B on an exact scorer calls this and swaps the table in together with B.
void spexact_check_and_cut(mi355rec_spscorer_t h, hipStream_t s, const int *b_ptr, const int *b_idx, DeviceBuffer<int> *cuts);
// cells of that table (0 when the scorer is not in exact mode): for the byte accounting of the calls that replace B
size_t spexact_table_cells(const mi355rec_spscorer *h);
// C[b][j] = A[rows[b]] . Bt[j] for b < n, j < m (A: rows of k floats, Bt: m x k, C: n x m, all row-major on the device): the scorer's
// f32 MFMA GEMM without biases, queued on `s`.  n <= 128 * 65535.
void gemm_rows_enqueue(const float *A, const int *rows, int n, int k, const float *Bt, int m, float *C, hipStream_t s);

// handoff.hip: what mi355rec_scorer_update_from_mf (mf.hip) and mi355rec_scorer_update_from_ials (ials.hip) share.
// out[i] = (float)in[i], round to nearest, for i < n; queued on `s`
void f64_to_f32_enqueue(const double *in, float *out, size_t n, hipStream_t s);
// the refusals: the shape and the biases of the `source` handle ("MF", "IALS") against the scorer's (MI355REC_E_INVALID)
void hand_off_check(const mi355rec_scorer *sc, const char *source, int n_users, int n_items, int k, int use_bias);
// Around the copy kernels, which the caller queues on the training handle's stream `source`, behind that handle's own work: begin
// drains the scorer's stream first (nothing reads the old model any more) and starts the scorer's call_timer on `source`; end stops
// it, waits for `source` -- neither handle's later work can race the copy -- and fills the scorer's stats.
void hand_off_begin(mi355rec_scorer *sc, hipStream_t source);
void hand_off_end(mi355rec_scorer *sc, hipStream_t source, double bytes, int launches);

// handoff.hip: a CSR that is already on the device (n_mid + 1 row pointers, at most `max_cells` ids and values; n_mid x n_items) becomes
// the sparse scorer's B.  What mi355rec_spscorer_update_from_slim (slim.hip) is made of, and what the next device-resident similarity
// model goes through:
//   begin   drains the scorer's stream (lists an evaluator queued there still read the old B) and starts the scorer's `timer` on
//           `source`, the stream of the handle that owns the CSR; the caller then queues whatever builds the CSR on `source`;
//   adopt   queues csr_adopt_kernel on `source` -- the CSR is copied into the spare buffers and checked in the same pass -- and waits.
//           A CSR that is not canonical (pointers from 0 upwards within max_cells, ids strictly ascending inside [0, n_items)) is a
//           bug of whoever built it: MI355REC_E_HIP naming the row, the scorer as it was.  In exact mode the table is rebuilt.  Then
//           the buffers are swapped, nnz_b follows, and the stats are call_ms = kernel_ms = begin .. here on `source`,
//           algorithmic_bytes = build_bytes (what building the CSR read) + the adopt pass's read and write + the exact table's,
//           n_launches = build_launches + the ones made here.
void spscorer_adopt_begin(mi355rec_spscorer *sc, hipStream_t source);
void spscorer_adopt(mi355rec_spscorer *sc, hipStream_t source, const int *indptr, const int *indices, const float *data, size_t max_cells,
                    double build_bytes, int build_launches);
// score.hip: room for a B of `cells` cells in the spare buffers (spscorer_plan.h's growth rule); the caller has drained h->stream
void spscorer_reserve_spare(mi355rec_spscorer *h, size_t cells);
// score.hip: the spare buffers, holding an accepted B of nnz cells (and `cuts`, its table, on an exact scorer), become the live ones
void spscorer_swap_in(mi355rec_spscorer *h, size_t nnz, DeviceBuffer<int> &cuts);

}  // namespace mi355rec
