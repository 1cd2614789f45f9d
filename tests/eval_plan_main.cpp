// Stand-alone program around csrc/eval_plan.h: the shell and run arithmetic of DIVERSITY_SIMILARITY straight through the header, on
// arrays of exactly the size the kernel's LDS arrays and buffers have for the list at hand -- every index a run hands out stays inside
// them.  tests/test_evaluation_diversity_cpu.py builds it with g++ -fsanitize=address,undefined and runs it as a child process; any
// finding or failed check ends it non-zero.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/eval_plan.h"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace mi355rec::evalplan;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++failures;                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
        }                                                                   \
    } while (0)

static const int CUTOFF_LISTS[][5] = {{2, 3, 5, 0, 0}, {10, 2, 65, 64, 130}, {1, 1024, 70, 69, 71}};

// a list of `len` distinct items of a matrix of n_items x n_items cells, item q = (q * 7 + 3) % n_items
static void one_list(int len, int n_items) {
    std::vector<int> items(len);
    for (int q = 0; q < len; ++q) items[q] = (q * 7 + 3) % n_items;
    std::vector<double> D((size_t)n_items * n_items);
    for (size_t i = 0; i < D.size(); ++i) D[i] = (double)((i * 2654435761u) % 1025) / 1024.0;
    const int n_runs = div_run_count(len);
    CHECK(n_runs == (len >= 2 ? 2 * (len - 1) : 0));
    std::vector<double> run_sums(n_runs);
    std::vector<int> seen((size_t)len * len, 0);
    for (int w = 0; w < n_runs; ++w) {
        const DivRun r = div_run(w);
        CHECK(r.shell >= 1 && r.shell <= len - 1 && r.fixed >= 0 && r.fixed < len && r.count >= 0 && r.count <= len - 1);
        double s = 0.0;
        for (int q = 0; q < r.count; ++q) {
            const int i = r.column ? q : r.fixed, j = r.column ? r.fixed : q;
            CHECK(i != j && i <= len - 2 && div_shell(i, j) == r.shell);
            ++seen[(size_t)i * len + j];
            const uint64_t at = div_run_cell(r, items.data(), q, n_items);
            CHECK(at == (uint64_t)items[i] * n_items + items[j] && at < D.size());
            s += D.at(at);
        }
        run_sums.at(w) = s;
    }
    for (int i = 0; i < len; ++i)                               // every cell of the reference's loop once, nothing else
        for (int j = 0; j < len; ++j) CHECK(seen[(size_t)i * len + j] == (i != j && i <= len - 2));
    for (const auto &cuts : CUTOFF_LISTS)
        for (int cutoff : cuts) {
            if (cutoff == 0) continue;
            const int l = div_cutoff_length(cutoff, len), shells = div_cutoff_shells(cutoff, len);
            CHECK(l == (cutoff < len ? cutoff : len) && shells == (l >= 2 ? l - 1 : -1));
            if (shells < 0) continue;
            CHECK(2 * shells <= n_runs && div_denominator(cutoff, len) == (double)l * (l - 1));
            double numerator = 0.0, brute = 0.0;
            for (int k = 1; k <= shells; ++k) numerator += run_sums.at(2 * (k - 1)) + run_sums.at(2 * (k - 1) + 1);
            for (int i = 0; i + 1 < l; ++i)
                for (int j = 0; j < l; ++j)
                    if (j != i) brute += D[(size_t)items[i] * n_items + items[j]];
            CHECK(numerator == brute);                          // (multiples of 2^-10 below 2^11: every sum is exact)
        }
}

int main() {
    for (int len = 0; len <= 70; ++len) one_list(len, 97);
    one_list(DIV_MAX_WIDTH, DIV_MAX_WIDTH + 5);
    // the cell offset where int arithmetic ends
    CHECK(div_cell_offset(46339, 46339, 46340) == 2147395599ull);
    CHECK(div_cell_offset(46340, 46340, 46341) == 2147488280ull);
    CHECK(div_cell_offset(1999999, 1999999, 2000000) == 3999999999999ull);
    CHECK(div_matrix_bytes(26744, 8) == 5721932288ull && div_matrix_bytes(2000000, 8) == 32000000000000ull);
    CHECK(div_value_cells(2147483647, 64) == 137438953408ull);
    CHECK(div_upload_chunks(0) == 0 && div_upload_chunks(1) == 1 && div_upload_chunks(DIV_UPLOAD_CHUNK) == 1 &&
          div_upload_chunks(DIV_UPLOAD_CHUNK + 1) == 2);
    CHECK(div_range_blocks(0) == 1 && div_range_blocks(2048) == 1 && div_range_blocks(2049) == 2 && div_range_blocks(1ull << 40) == 4096);
    CHECK(div_width_ok(1) && div_width_ok(1024) && !div_width_ok(1025) && !div_width_ok(0));
    CHECK(div_threads(64) == 64 && div_threads(65) == 256);
    CHECK(div_elem_ok(4) && div_elem_ok(8) && !div_elem_ok(2) && !div_elem_ok(0));
    if (failures) {
        fprintf(stderr, "eval_plan_main: %d checks failed\n", failures);
        return 1;
    }
    printf("eval_plan_main: OK\n");
    return 0;
}
