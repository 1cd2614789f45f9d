// Stand-alone program around csrc/asy_estimate_plan.h: the lane layout, the longest-first order, the argument checks and the byte
// accounting of AsySVD's device estimate, straight through the header, on arrays that are exactly as long as the functions may read or
// write -- the sanitizer sees an access past either.  tests/test_asysvd_estimate_spec.py builds it with g++ -fsanitize=address,undefined
// and runs it as a child process; any finding or failed check ends it non-zero.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/asy_estimate_plan.h"

#include <cstdio>
#include <vector>

using namespace mi355rec::asy_estimate_plan;
using mi355rec::spscorer_plan::CsrFinding;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++failures;                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
        }                                                                   \
    } while (0)

static void layouts() {
    // every k an ASY_SVD handle takes: the tiles cover the factors exactly once, a group never leaves a wavefront, a workgroup is full
    for (int k = 1; k <= KMAX; ++k) {
        const Layout l = layout(1000, k);
        CHECK(l.vec == (k % 2 == 0 ? 2 : 1));
        CHECK(l.group >= 1 && l.group <= MAX_GROUP && (l.group & (l.group - 1)) == 0);
        CHECK(l.tiles * l.group * l.vec >= k && (l.tiles - 1) * l.group * l.vec < k);
        CHECK(l.tiles == 1 || l.group == MAX_GROUP);                // a second tile only when a wavefront is not enough
        CHECK(l.group == 1 || (l.group / 2) * l.vec < k);           // the narrowest group that holds the row
        CHECK(l.items_per_block * l.group == THREADS);
        CHECK(l.items == 1000LL * l.tiles && l.grid * l.items_per_block >= l.items && (l.grid - 1) * l.items_per_block < l.items);
    }
    const Layout a = layout(138493, 128), b = layout(138493, 256), c = layout(7, 1), d = layout(40, 65);
    CHECK(a.vec == 2 && a.group == 64 && a.tiles == 1 && a.items_per_block == 4 && a.grid == 34624);
    CHECK(b.vec == 2 && b.group == 64 && b.tiles == 2 && b.grid == 69247);
    CHECK(c.vec == 1 && c.group == 1 && c.tiles == 1 && c.items_per_block == 256 && c.grid == 1);
    CHECK(d.vec == 1 && d.group == 64 && d.tiles == 2 && d.items == 80 && d.grid == 20);
}

static void orders() {
    // lengths 2 0 5 2 0 1: longest first, rows of one length in their own order
    const std::vector<int32_t> indptr = {0, 2, 2, 7, 9, 9, 10};
    const int longest = longest_row(6, indptr.data());
    CHECK(longest == 5);
    std::vector<int32_t> count((size_t)longest + 2), order(6, -1);
    longest_first(6, indptr.data(), longest, count.data(), order.data());
    const std::vector<int32_t> want = {2, 0, 3, 5, 1, 4};
    CHECK(order == want);
    // nothing but empty rows; a single row
    const std::vector<int32_t> none = {0, 0, 0, 0};
    std::vector<int32_t> count0(2), order0(3, -1);
    CHECK(longest_row(3, none.data()) == 0);
    longest_first(3, none.data(), 0, count0.data(), order0.data());
    CHECK(order0[0] == 0 && order0[1] == 1 && order0[2] == 2);
    const std::vector<int32_t> one = {0, 4};
    std::vector<int32_t> count1(6), order1(1, -1);
    longest_first(1, one.data(), 4, count1.data(), order1.data());
    CHECK(order1[0] == 0);
}

static void checks() {
    CHECK(check_shape(10, 10, 1) == OK && check_shape(10, 10, KMAX) == OK);
    CHECK(check_shape(0, 10, 4) == EMPTY_SHAPE && check_shape(10, 0, 4) == EMPTY_SHAPE && check_shape(-1, 10, 4) == EMPTY_SHAPE);
    CHECK(check_shape(10, 10, 0) == K_RANGE && check_shape(10, 10, KMAX + 1) == K_RANGE && check_shape(10, 10, -3) == K_RANGE);
    for (int k = 1; k <= KMAX; ++k) CHECK(layout(2147483647LL, k).grid <= 2147483647LL);      // never more workgroups than rows
    // the CSR: unsorted rows and a column stored twice are taken as they are
    const std::vector<int32_t> indptr = {0, 3, 3, 5}, ids = {4, 0, 4, 2, 1};
    CHECK(check_csr(3, 5, indptr.data(), ids.data()).kind == CsrFinding::OK);
    CsrFinding f = check_csr(3, 4, indptr.data(), ids.data());
    CHECK(f.kind == CsrFinding::ID_OUTSIDE && f.row == 0 && f.value == 4);
    const std::vector<int32_t> negative = {4, 0, 4, 2, -1};
    f = check_csr(3, 5, indptr.data(), negative.data());
    CHECK(f.kind == CsrFinding::ID_OUTSIDE && f.row == 2 && f.value == -1);
    // bad pointers: no id is read (the ids are shorter than the pointers claim)
    const std::vector<int32_t> late = {1, 2, 3}, back = {0, 1000000, 2}, two = {0, 1};
    f = check_csr(2, 5, late.data(), two.data());
    CHECK(f.kind == CsrFinding::START_NOT_ZERO && f.value == 1);
    f = check_csr(2, 5, back.data(), two.data());
    CHECK(f.kind == CsrFinding::POINTERS_DECREASE && f.row == 1 && f.value == 2);
    // no cells at all: an empty id array is never looked at
    const std::vector<int32_t> empty_rows = {0, 0, 0};
    const std::vector<int32_t> no_ids;
    CHECK(check_csr(2, 5, empty_rows.data(), no_ids.data()).kind == CsrFinding::OK);
}

static void accounting() {
    CHECK(bytes(0, 3, 4) == 96.0 && bytes(10, 3, 4) == 10 * 40.0 + 96.0);
    CHECK(bytes(20000263, 138493, 128) == 20000263.0 * 1032.0 + 138493.0 * 1024.0);
}

int main() {
    layouts();
    orders();
    checks();
    accounting();
    if (failures) {
        fprintf(stderr, "asy_estimate_plan_main: %d failed checks\n", failures);
        return 1;
    }
    puts("asy_estimate_plan_main: OK");
    return 0;
}
