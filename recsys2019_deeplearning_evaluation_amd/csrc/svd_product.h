// svd_product.h -- the sparse x block product and the float64 Gram of svd.hip, as launchers on a caller's stream: what the PureSVD
// handle (svd.hip) and the NMF handle (nmf.hip) share.  The kernels stay in svd.hip.
#pragma once

#include "common.h"

namespace mi355rec {

// refuses what the product's gather cannot take: pointers that decrease, an index outside the other side (MI355REC_E_INVALID)
void validate_layout(int n, int n_other, const int *ptr, const int *idx);

// one side of the product: the matrix whose rows are the output rows, cut into pieces of at most 512 cells
struct Side {
    int n_rows = 0, n_pieces = 0, n_long = 0, n_slots = 0;
    DeviceBuffer<int> idx, p_row, p_begin, p_end, p_slot, l_row, l_first, l_count;
    DeviceBuffer<float> val;                           // empty for an all-ones matrix

    // uploads the layout and its piece tables; returns the bytes uploaded
    size_t build(int n, const int *row_ptr, const int *row_idx, const float *row_val, bool ones, hipStream_t s);
};

// Y[row] = sum_j val[j] * X[idx[j]] over the cells of the row, in cell order (val == nullptr: every value is 1); X and Y have r
// columns, `partial` holds n_slots rows of r floats.  Returns the number of launches (1, or 2 with rows of more than one piece).
int spmm_enqueue(const Side &sd, const float *val, const float *X, int r, float *Y, float *partial, hipStream_t s);

// G (r x r float64) = X^T X for X of n rows: slabs of rows, their partial tiles added in slab order
struct GramPlan {
    int slabs = 0, rows = 0;
    size_t make(int n, int r);                         // returns the float64 cells `part` needs
};
void gram_enqueue(const float *X, int n, int r, const GramPlan &plan, double *part, double *G, hipStream_t s);

// out[i] = i: the identity row gather of gemm_rows_enqueue
void iota_enqueue(int *out, int n, hipStream_t s);

}  // namespace mi355rec
