// blocks.h -- what the PureSVD handle (svd.hip) and the NMF handle (nmf.hip) are both built on: the URM in both layouts and one dense
// float32 block per side resident on the device (BlockPair), the sparse x block product and the float64 Gram matrix as launchers on a
// caller's stream.  Bodies and kernels: blocks.hip / blocks_kernels.cuh; every number they launch with: blocks_plan.h.
#pragma once

#include "blocks_plan.h"
#include "common.h"

namespace mi355rec {

// one side of the product: the matrix whose rows are the output rows, cut into pieces of at most 512 cells (blocks::piece_plan)
struct Side {
    int n_rows = 0, n_pieces = 0, n_long = 0, n_slots = 0;
    DeviceBuffer<int> idx, p_row, p_begin, p_end, p_slot, l_row, l_first, l_count;
    DeviceBuffer<float> val;                           // empty for an all-ones matrix

    // uploads the layout and its piece tables; returns the bytes uploaded
    size_t build(int n, const int *row_ptr, const int *row_idx, const float *row_val, bool ones, hipStream_t s);
};

// Y[row] = sum_j val[j] * X[idx[j]] over the cells of the row, in cell order (val == nullptr: every value is 1); X and Y have r
// columns, `partial` holds n_slots rows of r floats.  Launches blocks::product_launches(sd.n_long) kernels.
void spmm_enqueue(const Side &sd, const float *val, const float *X, int r, float *Y, float *partial, hipStream_t s);

// G (r x r float64) = X^T X for X of n rows: slabs of rows, their partial tiles added in slab order (blocks::GRAM_LAUNCHES kernels)
void gram_enqueue(const float *X, int n, int r, const blocks::GramPlan &plan, double *part, double *G, hipStream_t s);

// "side 2: 0 (...) or 1 (...)" with the caller's words for the two sides (MI355REC_E_INVALID)
void require_side(int side, const char *zero, const char *one);

// what mi355rec_svd_create and mi355rec_nmf_create are handed
struct PairArgs {
    int n_users, n_items, width;
    const int *row_ptr, *row_idx;
    const float *row_val;
    const int *col_ptr, *col_idx;
    const float *col_val;
    size_t nnz() const { return (size_t)row_ptr[n_users]; }
};

struct BlockPair : Handle {
    int n_users = 0, n_items = 0, width = 0, ones = 0;   // width: the columns of both blocks (r of PureSVD, k of NMF)
    size_t nnz = 0;
    Side sides[2];                                     // [0]: rows = users (the CSR layout), [1]: rows = items (the CSC layout)
    DeviceBuffer<float> block[2], partial;
    DeviceBuffer<double> gram_part;
    DeviceBuffer<int> iota;                            // the identity row gather of gemm_rows_enqueue
    blocks::GramPlan gram_plan[2];
    int64_t launches = 0, calls = 0, create_bytes = 0, h2d_bytes = 0, d2h_bytes = 0;

    int rows_of(int s) const { return s == 0 ? n_users : n_items; }
    const float *values(int s) const { return ones ? nullptr : sides[s].val.ptr; }

    // The refusals of a create call that come before the device is touched, in the order both handles had them; `width_noun` is the
    // handle's word for the width ("block width r").  `out` is the create call's handle pointer.
    static void check_create(const void *out, const PairArgs &a, const char *width_noun);
    // Uploads both layouts and allocates what both handles hold; enqueues on `stream`, which the caller synchronises.
    blocks::PairSizes create_common(const PairArgs &a, bool all_ones);

    void set_block(int side, const float *X);          // host -> block[side], waits
    void get_block(int side, float *X);                // block[side] -> host, waits
    void product(int dst_side, const float *val, float *Y) {      // Y = layout[dst_side] . block[1 - dst_side]
        spmm_enqueue(sides[dst_side], val, block[1 - dst_side].ptr, width, Y, partial.ptr, stream);
    }
    void gram(int side, double *G) { gram_enqueue(block[side].ptr, rows_of(side), width, gram_plan[side], gram_part.ptr, G, stream); }
    // the five traffic counters and the all-ones flag, as both fit_info calls report them
    void traffic(int64_t *launches_, int64_t *calls_, int64_t *create_bytes_, int64_t *h2d_bytes_, int64_t *d2h_bytes_, int32_t *all_ones) const;

protected:
    ~BlockPair() = default;                            // (handle_destroy deletes through the exact type)
};

}  // namespace mi355rec
