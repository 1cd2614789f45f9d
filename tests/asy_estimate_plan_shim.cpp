// extern "C" wrapper around csrc/asy_estimate_plan.h for tests/test_asysvd_estimate_spec.py, which compiles it with g++ and calls it
// through ctypes: no GPU, no HIP runtime.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/asy_estimate_plan.h"

#include <cstring>
#include <vector>

using namespace mi355rec::asy_estimate_plan;

// out[6]: factors per lane, lanes of a group, column tiles, items of a workgroup, items, grid
extern "C" void ae_layout(int64_t n_rows, int k, int64_t *out) {
    const Layout l = layout(n_rows, k);
    const int64_t v[6] = {l.vec, l.group, l.tiles, l.items_per_block, l.items, l.grid};
    memcpy(out, v, sizeof(v));
}

// out[4]: KMAX, THREADS, MAX_GROUP, DEPTH
extern "C" void ae_constants(int *out) {
    const int v[4] = {KMAX, THREADS, MAX_GROUP, DEPTH};
    memcpy(out, v, sizeof(v));
}

extern "C" int ae_check_shape(int64_t n_rows, int64_t n_items, int k) { return check_shape(n_rows, n_items, k); }

// out[3]: what the check found (0 nothing, 1 the pointers do not start at 0, 2 they decrease, 3 an id outside), the row, the value
extern "C" void ae_check_csr(int n_rows, int n_items, const int32_t *indptr, const int32_t *indices, int64_t *out) {
    const mi355rec::spscorer_plan::CsrFinding f = check_csr(n_rows, n_items, indptr, indices);
    const int64_t v[3] = {f.kind, f.row, f.value};
    memcpy(out, v, sizeof(v));
}

extern "C" void ae_longest_first(int n_rows, const int32_t *indptr, int32_t *order) {
    const int longest = longest_row(n_rows, indptr);
    std::vector<int32_t> count((size_t)longest + 2);
    longest_first(n_rows, indptr, longest, count.data(), order);
}

extern "C" double ae_bytes(int64_t nnz, int64_t n_rows, int k) { return bytes(nnz, n_rows, k); }
