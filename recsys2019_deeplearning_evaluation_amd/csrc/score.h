// score.h -- the "score + rank on the handle's stream" half of mi355rec_scorer_recommend / mi355rec_spscorer_recommend
// (score.hip), shared with the holdout evaluator (eval.hip), whose metric kernel reads the ranked lists where these leave them.
#pragma once

#include "common.h"

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
// C[b][j] = A[rows[b]] . Bt[j] for b < n, j < m (A: rows of k floats, Bt: m x k, C: n x m, all row-major on the device): the scorer's
// f32 MFMA GEMM without biases, queued on `s`.  n <= 128 * 65535.
void gemm_rows_enqueue(const float *A, const int *rows, int n, int k, const float *Bt, int m, float *C, hipStream_t s);
void scorer_info(mi355rec_scorer_t h, int *n_users, int *n_items, hipStream_t *stream);
void spscorer_info(mi355rec_spscorer_t h, int *n_users, int *n_items, hipStream_t *stream);

}  // namespace mi355rec
