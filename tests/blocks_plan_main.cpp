// Stand-alone program around csrc/blocks_plan.h: the tables of tests/test_blocks_plan.py once more, straight through the header, with
// the properties that are about memory -- every index a plan hands to the kernels stays inside the array or buffer the plan sizes for
// it.  The test builds it with g++ -fsanitize=address,undefined and runs it as a child process; any finding or failed check ends it
// non-zero.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/blocks_plan.h"

#include <cmath>
#include <cstdio>
#include <limits>

using namespace mi355rec::blocks;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++failures;                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
        }                                                                   \
    } while (0)

static const int WIDTHS[] = {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129, 3072, 3073, 4096};
static const int ROWS[] = {1, 15, 16, 17, 63, 64, 65, 1000, 138493, GEMM_MAX_ROWS, GEMM_MAX_ROWS + 1};

// row pointers of exactly n + 1 entries, indices of exactly nnz: the sanitizer sees a read past either
static void pieces(const std::vector<int> &lengths) {
    std::vector<int> ptr(1, 0);
    for (int n : lengths) ptr.push_back(ptr.back() + n);
    const int n = (int)lengths.size(), nnz = ptr.back();
    const PiecePlan p = piece_plan(ptr.data(), n);
    std::vector<char> cell(nnz, 0), slot_used(p.n_slots, 0);
    CHECK(p.begin.size() == p.row.size() && p.end.size() == p.row.size() && p.slot.size() == p.row.size());
    for (int i = 0; i < p.n_pieces(); ++i) {
        CHECK(p.row[i] >= 0 && p.row[i] < n && p.end[i] - p.begin[i] <= SPLIT && p.begin[i] >= ptr[p.row[i]] && p.end[i] <= ptr[p.row[i] + 1]);
        for (int j = p.begin[i]; j < p.end[i]; ++j) CHECK(!cell.at(j)++);                 // every cell in exactly one piece
        if (p.slot[i] >= 0) CHECK(!slot_used.at(p.slot[i])++);                              // a partial row is written by one piece
    }
    for (char c : cell) CHECK(c == 1);
    CHECK(p.long_first.size() == p.long_row.size() && p.long_count.size() == p.long_row.size());
    for (int l = 0; l < p.n_long(); ++l) {                                                  // the long-rows kernel reads first .. first + count - 1
        CHECK(p.long_row[l] >= 0 && p.long_row[l] < n && p.long_count[l] >= 2);
        for (int q = 0; q < p.long_count[l]; ++q) CHECK(slot_used.at(p.long_first[l] + q) == 1);
    }
    for (char c : slot_used) CHECK(c == 1);
    CHECK(side_upload_bytes(nnz, false, p.row.size(), p.long_row.size()) == 4 * (2 * (size_t)nnz + 4 * p.row.size() + 3 * p.long_row.size()));
    CHECK(product_launches(p.n_long()) == (p.n_long() ? 2 : 1));
}

static void layouts() {
    const int ok_ptr[] = {0, 2, 2, 3}, ok_idx[] = {0, 3, 1};
    CHECK(check_layout(3, 4, ok_ptr, ok_idx).kind == LayoutFinding::OK);
    const int none_ptr[] = {0, 0, 0};
    CHECK(check_layout(2, 5, none_ptr, nullptr).kind == LayoutFinding::OK);                  // no cell: the indices are never read
    const int start[] = {1, 2, 3};
    CHECK(check_layout(2, 4, start, ok_idx).kind == LayoutFinding::START_NOT_ZERO);
    // pointers that decrease end the check before an index is read: the indices here are shorter than ptr[1] claims
    const int down[] = {0, 1000000, 2};
    LayoutFinding f = check_layout(2, 4, down, ok_idx);
    CHECK(f.kind == LayoutFinding::POINTERS_DECREASE && f.at == 1);
    const int bad_idx[] = {0, 4, -1};
    f = check_layout(3, 4, ok_ptr, bad_idx);
    CHECK(f.kind == LayoutFinding::INDEX_OUTSIDE && f.index == 4);
}

static void values() {
    const float eps = std::numeric_limits<float>::epsilon();
    CHECK(EPS32 == eps);
    const std::vector<float> ones(5, 1.f), above = {1.f, 1.f, 1.0000001f, 1.f}, first = {-1.f, 2.f, 3.f}, last = {1.f, 1.f, 1.f, -0.5f};
    const std::vector<float> zeros = {0.f, 0.f, 1.f, 0.f}, at_eps = {eps, 1.f, eps}, over = {std::nextafter(eps, 1.f), 1.f, 0.5f}, nan = {1.f, NAN};
    CHECK(all_ones(nullptr, 0) && scan_values(nullptr, 0).ones && !scan_values(nullptr, 0).negative);
    CHECK(all_ones(ones.data(), ones.size()) && scan_values(ones.data(), ones.size()).ones && scan_values(ones.data(), ones.size()).norm_x == 5.0);
    CHECK(!all_ones(above.data(), above.size()) && !scan_values(above.data(), above.size()).ones);
    ValueScan s = scan_values(first.data(), first.size());
    CHECK(s.negative && s.negative_at == 0 && s.negative_value == -1.f);
    s = scan_values(last.data(), last.size());
    CHECK(s.negative && s.negative_at == 3 && s.negative_value == -0.5f);
    s = scan_values(nan.data(), nan.size());
    CHECK(s.negative && s.negative_at == 1);
    s = scan_values(zeros.data(), zeros.size());
    CHECK(!s.negative && !s.ones && s.norm_x == 1.0 && s.sum_x == 1.0);
    CHECK(scan_values(at_eps.data(), at_eps.size()).sum_x == 1.0);
    CHECK(scan_values(over.data(), over.size()).sum_x == (double)over[0] + 1.0 + 0.5);
}

static void plans() {
    for (int r : WIDTHS) {
        const int shift = group_shift(r);
        CHECK(shift == (r <= 16 ? 4 : r <= 32 ? 5 : 6) && width_in_range(r) && gram_tiles(r) * GT >= r && (int64_t)gram_reduce_grid(r) * NT >= (int64_t)r * r);
        for (int n : ROWS) {
            GramPlan g;
            const size_t cells = g.make(n, r);
            CHECK(g.slabs >= 1 && g.rows % GR == 0 && (int64_t)g.slabs * g.rows >= n && (int64_t)(g.slabs - 1) * g.rows < n && cells == (size_t)g.slabs * r * r);
            const ColsumPlan c = colsum_plan(n);
            CHECK(c.used >= 1 && c.used <= c.slabs && c.slabs <= CS_SLABS && (int64_t)c.used * c.rows >= n && (int64_t)(c.used - 1) * c.rows < n);
            const SweepPlan p = sweep_plan(n, r);
            CHECK((int64_t)p.blocks * p.rows_per_block >= n && (int64_t)(p.blocks - 1) * p.rows_per_block < n && p.rows_per_block << p.shift == NT);
            // a thread's columns sub + q * lanes, q < ceil(r / lanes), are the floats [q * NT + tid] of the dynamic LDS
            CHECK(p.lds_bytes >= ((size_t)((r - 1) >> p.shift) * NT + NT) * sizeof(float) && p.lds_bytes <= 64 * 1024 && p.raise_attribute == (p.lds_bytes > 48 * 1024));
            for (int pieces : {0, 1, n, n + n / 512}) {
                const size_t red = red_part_cells(pieces, n, n, r);
                CHECK(red >= (size_t)p.blocks && red >= (size_t)sddmm_grid(pieces, r) && red >= (size_t)sddmm_grid(n, r) && red >= (size_t)RED_BLOCKS);
                CHECK((int64_t)product_grid(pieces, r) * SPMM_THREADS >= (int64_t)pieces << shift);
            }
            CHECK(dot_blocks((size_t)n * r) >= 1 && dot_blocks((size_t)n * r) <= RED_BLOCKS && (int64_t)cell_grid((size_t)n * 64) * NT >= (int64_t)n * 64);
            GramPlan both[2];
            const PairSizes z = pair_sizes(n, 17, r, 3, 0, both);
            CHECK(z.n_max == std::max(n, 17) && z.cap == (size_t)z.n_max * r && z.partial_rows == 3 && z.gram_part_cells >= (size_t)both[0].slabs * r * r);
        }
    }
    CHECK(!width_in_range(0) && !width_in_range(4097) && rows_in_range(GEMM_MAX_ROWS, 1) && !rows_in_range(1, GEMM_MAX_ROWS + 1));
    CHECK(!sweep_plan(5, 3072).raise_attribute && sweep_plan(5, 3073).raise_attribute);
}

static void accounting() {
    for (int n_long : {0, 3}) {
        const int product = product_launches(n_long);
        CHECK(prepare_frobenius_launches(n_long) == 3 + product && sweep_launches(false, n_long) == 5 + product && sweep_launches(true, n_long) == 2);
        CHECK(mu_step_launches(0, false, n_long) == 5 + product && mu_step_launches(0, true, n_long) == 2);
        CHECK(mu_step_launches(1, false, n_long) == 4 + product && mu_step_launches(1, true, n_long) == 2 + product);
        CHECK(divergence_launches(0, n_long) == 9 + product && divergence_launches(1, n_long) == 9);
    }
    CHECK(block_bytes(GEMM_MAX_ROWS, 4096) == (int64_t)GEMM_MAX_ROWS * 4096 * 4 && gram_download_bytes(4096) == 8ll * 4096 * 4096);
    CHECK(product_figures(0, 5).bytes == 0.0 && fill_figures(10).flops == 0.0 && sweep_figures(7, 3).flops == 126.0);
}

int main() {
    pieces({0, 1, 511, 512, 513, 1023, 1024, 1025, 1537});
    pieces(std::vector<int>(1537, 3));
    pieces({0, 0, 0});
    pieces({});
    layouts();
    values();
    plans();
    accounting();
    if (failures) {
        fprintf(stderr, "blocks_plan_main: %d failed checks\n", failures);
        return 1;
    }
    puts("blocks_plan_main: OK");
    return 0;
}
