// spscorer_plan.h -- the host arithmetic of replacing B in the sparse similarity scorer (score.hip: mi355rec_spscorer_update_b and
// mi355rec_spscorer_get_b; slim.hip + handoff.hip: mi355rec_spscorer_update_from_slim).  What is here: the check of a host CSR before
// anything is uploaded (it REPORTS the first bad row and why; score.hip words the refusal), the growth rule of the spare buffers the
// new B is written into, and the bytes each of the three calls accounts for.
// Plain C++17 on plain numbers and host arrays -- no HIP header, no common.h -- so g++ builds it alone and tests/test_slim_hand_off_spec.py
// runs tests/spscorer_plan_main.cpp under the host sanitizers without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace mi355rec {
namespace spscorer_plan {

// ---- the check of update_b ------------------------------------------------------------------------------------------------------------
// The row pointers are looked at first, all of them, and only then the ids: a pointer that decreases anywhere makes indptr[n_rows]
// meaningless as the length of `indices`, so no id is read before the pointers are known to climb from 0 to indptr[n_rows].  After
// that the ids are walked row by row and the first row with a finding wins.  `row` is -1 for START_NOT_ZERO (indptr[0] belongs to no
// row); `value` is the pointer or the id that was found.
struct CsrFinding {
    enum Kind { OK, START_NOT_ZERO, POINTERS_DECREASE, ID_OUTSIDE, NOT_ASCENDING } kind = OK;
    int row = -1;
    int64_t value = 0;
};

// ascending: the ids of a row must be strictly ascending (the exact mode: a column stored twice, or an unsorted row, cannot be served)
inline CsrFinding check_csr(int n_rows, int n_cols, const int32_t *indptr, const int32_t *indices, bool ascending) {
    if (indptr[0] != 0) return {CsrFinding::START_NOT_ZERO, -1, indptr[0]};
    for (int r = 0; r < n_rows; ++r)
        if (indptr[r + 1] < indptr[r]) return {CsrFinding::POINTERS_DECREASE, r, indptr[r + 1]};
    for (int r = 0; r < n_rows; ++r)
        for (int32_t t = indptr[r]; t < indptr[r + 1]; ++t) {
            const int32_t col = indices[t];
            if (col < 0 || col >= n_cols) return {CsrFinding::ID_OUTSIDE, r, col};
            if (ascending && t > indptr[r] && indices[t - 1] >= col) return {CsrFinding::NOT_ASCENDING, r, col};
        }
    return {};
}

// ---- the spare buffers ------------------------------------------------------------------------------------------------------------------
// A new B is written into spare buffers and swapped in once it has been accepted, so the buffers that come back as spares are the ones
// that held the B before.  Cells (ids and values alike) the spare buffer must hold for a B of `need` cells when it holds `have`: it is
// kept while it is large enough, and grows by at least a quarter beyond what it was, so a W whose nnz creeps up from one validation to
// the next does not allocate every time.  Never shrinks.  The row pointers are always n_rows + 1.
inline size_t spare_cells(size_t have, size_t need) {
    if (need <= have) return have;
    return std::max(need, have + have / 4);
}

// the most cells mi355rec_spscorer_update_from_slim can be handed: a W of topK slots per row (known before the launch, so the spare
// buffers are sized without waiting for the device to say how many cells W kept)
inline size_t slim_w_cells_bound(int n_items, int topK) { return (size_t)n_items * (size_t)std::min(topK, n_items); }

// ---- accounting: bytes read + written on the device -------------------------------------------------------------------------------------
inline double csr_bytes(int n_rows, size_t nnz) { return 4.0 * ((double)n_rows + 1) + 8.0 * (double)nnz; }
// exact mode's pass over a B that is already in place: the check reads pointers and ids, the table's binary searches read them again
// and write cuts_cells ints (0: the scorer is not in exact mode and nothing of this runs)
inline double exact_table_bytes(int n_rows, size_t nnz, size_t cuts_cells) {
    if (!cuts_cells) return 0.0;
    return 2.0 * (4.0 * ((double)n_rows + 1) + 4.0 * (double)nnz) + 4.0 * (double)cuts_cells;
}
// update_b: the copy writes the CSR
inline double update_b_bytes(int n_rows, size_t nnz, size_t cuts_cells) { return csr_bytes(n_rows, nnz) + exact_table_bytes(n_rows, nnz, cuts_cells); }
// get_b: the copy reads it
inline double get_b_bytes(int n_rows, size_t nnz, bool with_cells) { return with_cells ? csr_bytes(n_rows, nnz) : 4.0 * ((double)n_rows + 1); }
// update_from_slim: the row selection reads the weight store once (store_bytes: the dense n_items^2 cells or the packed triangle; the
// two sorts between it and the CSR work on n_items * topK slots and are not counted), the adopt pass reads W and writes it
inline double update_from_slim_bytes(double store_bytes, int n_items, size_t nnz, size_t cuts_cells) {
    return store_bytes + 2.0 * csr_bytes(n_items, nnz) + exact_table_bytes(n_items, nnz, cuts_cells);
}

}  // namespace spscorer_plan
}  // namespace mi355rec
