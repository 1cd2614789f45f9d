// Stand-alone program around csrc/spscorer_plan.h: the CSR check of mi355rec_spscorer_update_b, the growth rule of the spare buffers and
// the byte accounting, straight through the header, on arrays that are exactly as long as the check may read -- the sanitizer sees a
// read past either.  tests/test_slim_hand_off_spec.py builds it with g++ -fsanitize=address,undefined and runs it as a child process;
// any finding or failed check ends it non-zero.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/spscorer_plan.h"

#include <cstdio>
#include <vector>

using namespace mi355rec::spscorer_plan;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++failures;                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
        }                                                                   \
    } while (0)

// heap arrays of exactly these entries (an empty vector's data() may be null: the check must not read it)
static CsrFinding check(int n_cols, const std::vector<int32_t> &indptr, const std::vector<int32_t> &indices, bool ascending) {
    return check_csr((int)indptr.size() - 1, n_cols, indptr.data(), indices.data(), ascending);
}

static void csr_checks() {
    // an empty CSR: rows without a cell, no id is read
    CHECK(check(5, {0, 0, 0, 0}, {}, true).kind == CsrFinding::OK);
    CHECK(check(5, {0, 0, 0, 0}, {}, false).kind == CsrFinding::OK);
    // a single row
    CHECK(check(5, {0, 3}, {0, 2, 4}, true).kind == CsrFinding::OK);
    CHECK(check(5, {0, 3}, {4, 2, 0}, false).kind == CsrFinding::OK);          // unsorted: the atomic mode takes it
    CsrFinding f = check(5, {0, 3}, {4, 2, 0}, true);
    CHECK(f.kind == CsrFinding::NOT_ASCENDING && f.row == 0 && f.value == 2);
    f = check(5, {0, 2}, {3, 3}, true);                                       // a column stored twice
    CHECK(f.kind == CsrFinding::NOT_ASCENDING && f.row == 0 && f.value == 3);
    CHECK(check(5, {0, 2}, {3, 3}, false).kind == CsrFinding::OK);
    // the last row is the bad one, its last id: nothing is read beyond it
    f = check(5, {0, 1, 1, 3}, {0, 1, 5}, false);
    CHECK(f.kind == CsrFinding::ID_OUTSIDE && f.row == 2 && f.value == 5);
    f = check(5, {0, 1, 1, 3}, {0, 1, -1}, true);
    CHECK(f.kind == CsrFinding::ID_OUTSIDE && f.row == 2 && f.value == -1);
    f = check(5, {0, 1, 1, 3}, {0, 4, 1}, true);
    CHECK(f.kind == CsrFinding::NOT_ASCENDING && f.row == 2 && f.value == 1);
    // the first row with a finding wins; an id outside before an order finding in the same row
    f = check(5, {0, 2, 4}, {2, 1, 7, 0}, true);
    CHECK(f.kind == CsrFinding::NOT_ASCENDING && f.row == 0);
    f = check(5, {0, 2, 4}, {1, 2, 7, 0}, true);
    CHECK(f.kind == CsrFinding::ID_OUTSIDE && f.row == 1 && f.value == 7);
    // the order inside a row is a matter of that row alone: a row may start below its predecessor's last id
    CHECK(check(5, {0, 2, 4}, {3, 4, 0, 1}, true).kind == CsrFinding::OK);
    // row pointers: the start, a decrease at the first and at the last row.  The ids are shorter than the pointers claim before the
    // decrease: no id may be read once the pointers are known to be bad
    f = check(5, {1, 2, 3}, {0, 1, 2}, false);
    CHECK(f.kind == CsrFinding::START_NOT_ZERO && f.row == -1 && f.value == 1);
    f = check(5, {0, -1, 2}, {0, 1}, false);
    CHECK(f.kind == CsrFinding::POINTERS_DECREASE && f.row == 0 && f.value == -1);
    f = check(5, {0, 1000000, 2}, {0, 1}, false);
    CHECK(f.kind == CsrFinding::POINTERS_DECREASE && f.row == 1 && f.value == 2);
    // row pointers that end one short of the ids there are: the cell past indptr[n_rows] is never looked at, bad as it is
    std::vector<int32_t> ids = {0, 1, 2, 99};
    ids.resize(3);
    ids.shrink_to_fit();
    CHECK(check(5, {0, 1, 3}, ids, true).kind == CsrFinding::OK);
    // ... and ids that are one short of what the pointers of the LAST row claim cannot be told from the outside: the caller's contract
    // is indptr[n_rows] entries, and the check reads exactly those
    const std::vector<int32_t> exact = {0, 1, 2};
    CHECK(check(3, {0, 1, 3}, exact, true).kind == CsrFinding::OK);
    f = check(2, {0, 1, 3}, exact, true);
    CHECK(f.kind == CsrFinding::ID_OUTSIDE && f.row == 1 && f.value == 2);
}

static void growth() {
    // from 0 cells: exactly what is needed, nothing for an empty B
    CHECK(spare_cells(0, 0) == 0 && spare_cells(0, 1) == 1 && spare_cells(0, 5348800) == 5348800);
    // kept while it is large enough -- a smaller B does not shrink it -- and a quarter of slack when it grows by less than that
    CHECK(spare_cells(100, 100) == 100 && spare_cells(100, 0) == 100 && spare_cells(100, 99) == 100);
    CHECK(spare_cells(100, 101) == 125 && spare_cells(100, 125) == 125 && spare_cells(100, 126) == 126 && spare_cells(3, 4) == 4);
    size_t have = 0;
    int allocations = 0;
    for (size_t need = 1000; need < 2000; need += 10) {                        // a W whose nnz creeps up: a handful of allocations, not 100
        const size_t room = spare_cells(have, need);
        CHECK(room >= need);
        allocations += room != have;
        have = room;
    }
    CHECK(allocations == 5);                                                  // 1000, 1250, 1562, 1952, 2440
    CHECK(slim_w_cells_bound(26744, 200) == (size_t)26744 * 200 && slim_w_cells_bound(200, 500) == 200 * 200 && slim_w_cells_bound(65535, 4096) < ((size_t)1 << 31));
}

static void accounting() {
    CHECK(csr_bytes(3, 0) == 16.0 && csr_bytes(3, 10) == 96.0);
    CHECK(update_b_bytes(3, 10, 0) == 96.0 && update_b_bytes(3, 10, 68) == 96.0 + 2 * (16.0 + 40.0) + 272.0);
    CHECK(get_b_bytes(3, 10, false) == 16.0 && get_b_bytes(3, 10, true) == 96.0);
    CHECK(update_from_slim_bytes(36.0, 3, 10, 0) == 36.0 + 192.0 && update_from_slim_bytes(36.0, 3, 0, 0) == 36.0 + 32.0);
    CHECK(exact_table_bytes(3, 10, 0) == 0.0);
}

int main() {
    csr_checks();
    growth();
    accounting();
    if (failures) {
        fprintf(stderr, "spscorer_plan_main: %d failed checks\n", failures);
        return 1;
    }
    puts("spscorer_plan_main: OK");
    return 0;
}
