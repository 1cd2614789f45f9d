// extern "C" wrapper around csrc/spscorer_plan.h for tests/test_slim_hand_off_spec.py, which compiles it with g++ and calls it through
// ctypes: no GPU, no HIP runtime.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/spscorer_plan.h"

#include <cstring>

using namespace mi355rec::spscorer_plan;

// out[3]: what the check found (0 nothing, 1 the pointers do not start at 0, 2 they decrease, 3 an id outside, 4 ids not ascending),
// the row (-1 for kind 1), the pointer or id found
extern "C" void sp_check_csr(int n_rows, int n_cols, const int32_t *indptr, const int32_t *indices, int ascending, int64_t *out) {
    const CsrFinding f = check_csr(n_rows, n_cols, indptr, indices, ascending != 0);
    const int64_t v[3] = {f.kind, f.row, f.value};
    memcpy(out, v, sizeof(v));
}

extern "C" int64_t sp_spare_cells(int64_t have, int64_t need) { return (int64_t)spare_cells((size_t)have, (size_t)need); }
extern "C" int64_t sp_slim_w_cells_bound(int n_items, int topK) { return (int64_t)slim_w_cells_bound(n_items, topK); }

// out[4]: bytes of update_b, of get_b without and with the cells, of update_from_slim
extern "C" void sp_bytes(int n_rows, int64_t nnz, int64_t cuts_cells, double store_bytes, double *out) {
    out[0] = update_b_bytes(n_rows, (size_t)nnz, (size_t)cuts_cells);
    out[1] = get_b_bytes(n_rows, (size_t)nnz, false);
    out[2] = get_b_bytes(n_rows, (size_t)nnz, true);
    out[3] = update_from_slim_bytes(store_bytes, n_rows, (size_t)nnz, (size_t)cuts_cells);
}
