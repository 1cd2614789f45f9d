// asy_estimate.h -- what asy_estimate.hip offers the rest of the library: AsySVD's user-factor estimate on arrays that are on the device.
#pragma once

#include "common.h"

namespace mi355rec {

// a CSR (n_rows + 1 pointers, ids, float32 values), Y (n_items x k float64, row-major), one divisor per row, the rows' order
// (asy_estimate_upload_order) and the n_rows x k output, all device pointers
struct AsyEstimateArrays {
    const int *indptr, *indices;
    const float *data;
    const double *Y, *divisor;
    const int *order;
    double *out;
};

// order <- the rows of the host pointers longest first (asy_estimate_plan.h: longest_first), uploaded on s; the pointers must climb from 0
void asy_estimate_upload_order(int n_rows, const int32_t *indptr_host, DeviceBuffer<int> &order, hipStream_t s);

// One launch on s: out[u, f] = (sum over row u, in storage order, of (double)data[t] * Y[indices[t], f]) / divisor[u], every product and
// every sum rounded to float64 on its own, one division at the end; a row whose divisor is not above 0 is left undivided (+0.0 for the
// empty profile that a zero divisor stands for).  e0 / e1: start / stop events the dispatch carries, or null.  The shape must have
// passed asy_estimate_plan::check_shape and the ids must be inside [0, n_items); nothing is allocated, copied or waited for.
void asy_estimate_enqueue(int n_rows, int k, const AsyEstimateArrays &a, hipStream_t s, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);

}  // namespace mi355rec
