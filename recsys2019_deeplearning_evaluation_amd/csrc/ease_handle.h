// ease_handle.h -- the handle struct of the EASE_R closed form, shared by ease.hip (the unpivoted float32 elimination, weights and
// top-K) and ease_pivot.hip (the pivoted float64 elimination), and the head and tail both inverts run through.  Host text only: no
// kernel lives here; the arithmetic on the handle's shape is ease_plan.h.
#pragma once

#include "common.h"
#include "ease_plan.h"

namespace mi355rec {

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

// `timer`: around the elimination; `call_timer`: around the weights + top-K kernels (and the pivoted route's gather); n, npad, block, steps: EaseShape
struct mi355rec_ease : mi355rec::Handle, mi355rec::ease::EaseShape {
    int failed_step = -1, state = mi355rec::ST_EMPTY;
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

namespace mi355rec {

// ---- what mi355rec_ease_invert and mi355rec_ease_invert_pivoted share (defined in ease.hip) -----------------------------------------
// "<caller> needs a matrix that has been set and not yet inverted" unless one is there (then the device is bound).  Until begin_invert a
// route may still refuse the call with the matrix untouched (the pivoted route's workspace).
void require_invertible(const mi355rec_ease *h, const char *caller);
// The head: ST_FAILED until finish_invert says otherwise, the status word back to -1 (no step has failed), launches = 0, `timer` started.
void begin_invert(mi355rec_ease *h);
// After the last launch of the elimination: `timer` stopped and the download of the status word queued; a route queues its own
// downloads behind it, so that the one drain of await_elimination covers them all.
void stop_elimination(mi355rec_ease *h);
// Drains the stream; sets invert_ms and failed_step and returns the latter (-1: no step failed).
int await_elimination(mi355rec_ease *h);
// The tail: the stats of the call, then MI355REC_E_NUMERIC with `refusal` -- a format of the failed step, the steps and the block size
// -- where a step failed, ST_INVERTED where none did.
void finish_invert(mi355rec_ease *h, const ease::EaseAccounting &work, const char *refusal);

}  // namespace mi355rec
