// Stand-alone program around csrc/ease_plan.h: the tables of tests/test_ease_plan.py once more, straight through the header, with the
// properties that are about memory -- every workgroup a plan launches stays inside the panel and the buffers ease_pivot.hip sizes for
// it, and the permutation writes every cell of its two arrays once.  The test builds it with g++ -fsanitize=address,undefined and runs
// it as a child process; any finding or failed check ends it non-zero.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/ease_plan.h"

#include <cstdio>
#include <numeric>
#include <string>

using namespace mi355rec::ease;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++failures;                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
        }                                                                   \
    } while (0)

static const int SIZES[] = {1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200, 255, 256, 257, 3706, 17770, 26744};
static const int BLOCKS[] = {64, 128};

static void knobs() {
    unsetenv("MI355REC_EASE_BLOCK");
    unsetenv("MI355REC_EASE_PIVOT_MAX_BYTES");
    EaseKnobs k = read_ease_knobs();
    CHECK(k.block == EASE_TILE && ease_block_valid(k.block) && !k.pivot_max_bytes);
    for (const char *v : {"", "0", "32", "abc", "-64"}) {
        setenv("MI355REC_EASE_BLOCK", v, 1);
        CHECK(!ease_block_valid(read_ease_knobs().block));
    }
    setenv("MI355REC_EASE_BLOCK", "64", 1);
    setenv("MI355REC_EASE_PIVOT_MAX_BYTES", "", 1);
    k = read_ease_knobs();
    CHECK(k.block == 64 && ease_block_valid(k.block) && k.pivot_max_bytes && *k.pivot_max_bytes == 0);
    setenv("MI355REC_EASE_PIVOT_MAX_BYTES", "99999999999999999999999", 1);
    CHECK(*read_ease_knobs().pivot_max_bytes == ULLONG_MAX);
    unsetenv("MI355REC_EASE_BLOCK");
    unsetenv("MI355REC_EASE_PIVOT_MAX_BYTES");
    char text[96];
    snprintf(text, sizeof(text), EASE_BLOCK_MESSAGE, 32);
    CHECK(std::string(text) == "MI355REC_EASE_BLOCK must be 64 or 128, got 32");
}

static void fits() {
    const size_t need = pivot_bytes(*ease_shape(26744, 128));
    CHECK(pivot_fit(need, need + PIVOT_RESERVE, std::nullopt) == EaseFit::FITS && pivot_fit(need, need + PIVOT_RESERVE - 1, std::nullopt) == EaseFit::NO_ROOM);
    CHECK(pivot_fit(need, 0, need - 1) == EaseFit::OVER_CAP && pivot_fit(need, 0, need) == EaseFit::NO_ROOM && pivot_fit(need, SIZE_MAX, need) == EaseFit::FITS);
    CHECK(pivot_fit(need, SIZE_MAX, 0) == EaseFit::OVER_CAP && pivot_fit(0, PIVOT_RESERVE, 0) == EaseFit::FITS);
    const size_t mine = ease_bytes(*ease_shape(26744, 128));
    CHECK(ease_fit(mine, mine + EASE_RESERVE) == EaseFit::FITS && ease_fit(mine, mine + EASE_RESERVE - 1) == EaseFit::NO_ROOM && ease_fit(mine, 0) == EaseFit::NO_ROOM);
    CHECK(!ease_shape(INT32_MAX, 64) && !ease_shape(INT32_MAX - 126, 128) && ease_shape(INT32_MAX - 127, 128)->npad == INT32_MAX - 127);
}

// every workgroup of a pivoted step against the buffers ensure_work allocates: part_val / part_pos hold npad / CHUNK candidates, the
// scratch panel npad rows; the block step's grids tile the padded matrix exactly
static void pivoted(const EaseShape &s) {
    std::vector<char> part((size_t)s.npad / CHUNK, 0), panel_row((size_t)s.npad, 0);
    int64_t launches = PIVOT_FRONT_LAUNCHES;
    int searched = 0;
    for (int step = 0; step < s.steps; ++step) {
        const PivotStep p = pivot_step(s, step);
        CHECK(p.k0 == step * s.block && p.cols == std::min(s.block, s.n - p.k0) && p.k0 + s.block <= s.npad);
        CHECK(p.transpose_grid * TRANSPOSE_W == s.npad && p.panel_grid_long * SMALL_T == s.npad && p.panel_grid_short * SMALL_T == s.block);
        CHECK(p.update_tiles * EASE_TILE == s.npad && p.writeback_grid * PANEL_W == s.npad);
        int count = PIVOT_BLOCK_LAUNCHES;
        if (p.cols <= 0) {
            CHECK(p.load_grid == 0 && p.swap_grid == 0 && p.k0 >= s.n);
        } else {
            CHECK(p.load_grid >= 1 && p.swap_grid * SWAP_W == s.npad);
            for (int b = 0; b < p.load_grid; ++b) {                  // the load kernel: chunk k0 / CHUNK + b, rows of that chunk
                part.at((size_t)(p.k0 / CHUNK + b)) = 1;
                panel_row.at((size_t)(p.k0 / CHUNK + b) * CHUNK + CHUNK - 1) = 1;
            }
            CHECK((p.k0 / CHUNK + p.load_grid - 1) == (s.n - 1) / CHUNK);
            count += 2 + p.cols;
            for (int j = 0; j < p.cols; ++j) {
                const int g = p.k0 + j, grid = pivot_elim_grid(s, p.k0, j);
                ++searched;
                CHECK(grid >= 0 && (grid == 0) == (j + 1 == s.block || g + 1 == s.n));
                for (int b = 0; b < grid; ++b) {                     // the elimination kernel: chunk (g + 1) / CHUNK + b
                    part.at((size_t)((g + 1) / CHUNK + b)) = 1;
                    panel_row.at((size_t)((g + 1) / CHUNK + b) * CHUNK + CHUNK - 1) = 1;
                }
                if (grid) CHECK(((g + 1) / CHUNK + grid - 1) == (s.n - 1) / CHUNK);
                count += grid > 0;
            }
        }
        CHECK(p.launches == count);
        launches += count;
    }
    CHECK(searched == s.n);
    CHECK(pivot_launches(s, false) == launches && pivot_launches(s, true) == launches + PIVOT_GATHER_LAUNCHES);
    const int full = s.n / s.block, ragged = s.n % s.block;
    CHECK(launches == 2 + 6 * (int64_t)s.steps + (int64_t)full * (2 * s.block + 1) + (ragged ? 2 * ragged + 1 : 0));
}

static void shapes() {
    for (int n : SIZES)
        for (int block : BLOCKS) {
            const EaseShape s = *ease_shape(n, block);
            CHECK(s.n == n && s.block == block && s.npad % EASE_TILE == 0 && s.npad >= n && s.npad - n < EASE_TILE && s.steps * block == s.npad);
            CHECK(ease_bytes(s) >= (size_t)s.npad * s.npad * sizeof(float) && pivot_bytes(s) >= (size_t)s.npad * s.npad * sizeof(double));
            CHECK((s.npad == n) == (ease_bytes(s) == ((size_t)s.npad * s.npad + 3 * (size_t)s.npad * block + (size_t)block * block) * sizeof(float)));
            CHECK(panel_lds_bytes(block) <= 160 * 1024);
            for (int step = 0; step < s.steps; ++step) {
                const EaseStep p = ease_step(s, step);
                CHECK(p.k0 == step * block && p.k0 + block <= s.npad && p.diag_grid == 1);
                CHECK(p.panel_grid * PANEL_W == s.npad && p.update_tiles * EASE_TILE == s.npad && p.writeback_grid * PANEL_W == s.npad);
            }
            CHECK(ease_launches(s) == 4 * (int64_t)s.steps);
            pivoted(s);
            const EaseAccounting f = invert_accounting(s, sizeof(float)), d = invert_accounting(s, sizeof(double));
            CHECK(f.flops == 2.0 * n * (double)n * n && f.bytes == 8.0 * (double)n * n * s.steps && d.bytes == 2 * f.bytes && f.units == s.steps && d.flops == f.flops);
        }
}

// vectors of exactly npad entries: the sanitizer sees a read or write past either
static void permutation(std::vector<int> piv, int n) {
    const int npad = (int)piv.size();
    const std::vector<int> inv_perm = inverse_column_permutation(piv.data(), n, npad);
    CHECK((int)inv_perm.size() == npad);
    std::vector<int> order((size_t)npad);
    std::iota(order.begin(), order.end(), 0);
    for (int g = 0; g < n; ++g) std::swap(order.at((size_t)g), order.at((size_t)piv[g]));
    std::vector<char> hit((size_t)npad, 0);
    for (int l = 0; l < npad; ++l) {
        CHECK(inv_perm.at((size_t)order[l]) == l);
        CHECK(!hit.at((size_t)inv_perm[l])++);
    }
    for (int j = n; j < npad; ++j) CHECK(inv_perm[j] == j);
}

static void permutations() {
    for (int n : {1, 128, 129, 200, 26744}) {
        const int npad = ease_shape(n, 64)->npad;
        std::vector<int> identity((size_t)npad);
        std::iota(identity.begin(), identity.end(), 0);
        permutation(identity, n);
        std::vector<int> last = identity, next = identity, first_and_last = identity;
        for (int g = 0; g < n; ++g) last[g] = n - 1;                  // every swap reaches for the last row of the matrix
        for (int g = 0; g + 1 < n; ++g) next[g] = g + 1;
        first_and_last[0] = n - 1;
        permutation(last, n);
        permutation(next, n);
        permutation(first_and_last, n);
    }
}

int main() {
    knobs();
    fits();
    shapes();
    permutations();
    if (failures) {
        fprintf(stderr, "ease_plan_main: %d failed checks\n", failures);
        return 1;
    }
    puts("ease_plan_main: OK");
    return 0;
}
