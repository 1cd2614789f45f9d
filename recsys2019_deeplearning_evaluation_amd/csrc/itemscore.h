// itemscore.h -- the handle of the shared-vector scorer (itemscore.hip), a ScorerHandle (score.h) like the other three, for the holdout
// evaluators (eval.hip): every user is scored by the SAME vector of n_items floats -- the reference's non-personalized recommenders
// (Base/NonPersonalizedRecommender.py:30-43, 119-132) -- so a user's list is the head of one global order minus the user's seen items.
#pragma once

#include "score.h"

struct mi355rec_itemscorer final : mi355rec::ScorerHandle { // `timer`: everything one enqueue puts on the stream
    mi355rec::DeviceBuffer<float> vec;                      // the item scores, as given
    // the model's order: item ids by (score descending, id ascending), finite scores only; rank_of[item] = its position, -1 for an
    // item that is not in the order; length[0] = entries of the order (read by the kernels from device memory)
    mi355rec::DeviceBuffer<int> order, rank_of, length;
    mi355rec::DeviceBuffer<int> m_order, m_rank_of, m_length;   // the same three after an item mask: rebuilt by every masked call
    mi355rec::DeviceBuffer<uint32_t> keys, keys_sorted;         // sort keys of (re)building the order
    mi355rec::DeviceBuffer<int> ids;
    mi355rec::DeviceBuffer<unsigned char> tmp;                  // rocPRIM's temporary storage: the radix sort's or the selection's
    int n_order = 0;
    int window_bits = 0;                                        // W: positions of the order one pass of the ranking kernel covers

    mi355rec::Ranking enqueue(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed, bool keep_scores) override;
    mi355rec::Ranking enqueue_candidates(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                                         const mi355rec::CandidateRows &rows) override;
    [[noreturn]] void bad_user(int user) const override { cold_user(user); }
    void fill_recommend_stats(const int32_t *user_ids, int n) override;
    ~mi355rec_itemscorer() { shutdown(); }
};
