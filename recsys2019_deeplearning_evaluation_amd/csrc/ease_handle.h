// ease_handle.h -- the handle struct of the EASE_R closed form, shared by ease.hip (the unpivoted float32 elimination, weights and
// top-K) and ease_pivot.hip (the pivoted float64 elimination).  Host text only: no kernel lives here.
#pragma once

#include "common.h"

namespace mi355rec {

constexpr int EASE_TILE = 128;      // the matrix is padded to a multiple of it; its tail carries an identity block

enum { ST_EMPTY = 0, ST_MATRIX, ST_FAILED, ST_INVERTED, ST_WEIGHTS };

// What the pivoted inverse adds to a handle, allocated at the first mi355rec_ease_invert_pivoted and freed with the handle.
struct EasePivotWork {
    DeviceBuffer<double> A;             // the working matrix, npad x npad
    DeviceBuffer<double> panel;         // scratch copy of a block column for the pivot search, npad x block
    DeviceBuffer<double> D, Dt, R, Ct, ND;
    DeviceBuffer<double> part_val;      // per 64-row chunk: the largest |value| of the column searched next ...
    DeviceBuffer<int> part_pos;         // ... and its row
    DeviceBuffer<int> piv, inv_perm;    // piv[g]: the row swapped with row g; inv_perm[j]: the column of the result that holds column j
    DeviceBuffer<double> info;          // [0] smallest |pivot|, [1] swaps that moved a row
    std::vector<hipEvent_t> events;     // four per step: pivot search + swaps, then the update
    int moved = 0;
    double min_pivot = 0, pivot_ms = 0, update_ms = 0;
    bool valid = false;                 // the four figures above describe a pivoted inverse that ran
};

}  // namespace mi355rec

struct mi355rec_ease : mi355rec::Handle {     // `timer`: around the elimination; `call_timer`: around the weights + top-K kernels
    int n = 0, npad = 0, block = 0, steps = 0, failed_step = -1, state = mi355rec::ST_EMPTY;
    mi355rec::DeviceBuffer<float> A, D, R, Ct, ND, diag, out_val;
    mi355rec::DeviceBuffer<int> status, out_idx;
    double invert_ms = 0, gram_ms = 0, topk_ms = 0;
    int64_t launches = 0;
    mi355rec::EasePivotWork pivot;

    ~mi355rec_ease() {
        shutdown([&] {
            for (hipEvent_t e : pivot.events) (void)hipEventDestroy(e);
            pivot.events.clear();
        });
    }
};
