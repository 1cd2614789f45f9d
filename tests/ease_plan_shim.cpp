// extern "C" wrapper around csrc/ease_plan.h for tests/test_ease_plan.py, which compiles it with g++ and calls it through ctypes: no GPU,
// no HIP runtime.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/ease_plan.h"

#include <cstdio>
#include <cstring>

using namespace mi355rec::ease;

static EaseShape shape_of(int n, int block) { return *ease_shape(n, block); }

extern "C" void ep_constants(int64_t *out) {
    const int64_t v[7] = {EASE_TILE, TK, PANEL_W, CHUNK, GK, (int64_t)EASE_RESERVE, (int64_t)PIVOT_RESERVE};
    memcpy(out, v, sizeof(v));
}

// out[4]: the block as read, whether create takes it, whether a cap is set, the cap; message: what create says of the block
extern "C" void ep_read_knobs(uint64_t *out, char *message, int room) {
    const EaseKnobs k = read_ease_knobs();
    const uint64_t v[4] = {(uint64_t)(int64_t)k.block, ease_block_valid(k.block), k.pivot_max_bytes.has_value(), k.pivot_max_bytes.value_or(0)};
    memcpy(out, v, sizeof(v));
    snprintf(message, room, EASE_BLOCK_MESSAGE, k.block);
}

// 0 where the padded matrix has too many rows; out[5]: npad, steps, bytes of the handle, of the pivoted workspace, LDS of the panel kernel
extern "C" int ep_shape(int n, int block, int64_t *out) {
    const std::optional<EaseShape> s = ease_shape(n, block);
    if (!s) return 0;
    const int64_t v[5] = {s->npad, s->steps, (int64_t)ease_bytes(*s), (int64_t)pivot_bytes(*s), (int64_t)panel_lds_bytes(block)};
    memcpy(out, v, sizeof(v));
    return s->n == n && s->block == block;
}

// verdicts: 0 fits, 1 no room, 2 over the cap
extern "C" int ep_ease_fit(uint64_t need, uint64_t free_bytes) { return (int)ease_fit(need, free_bytes); }
extern "C" int ep_pivot_fit(uint64_t need, uint64_t free_bytes, int has_cap, uint64_t cap) {
    return (int)pivot_fit(need, free_bytes, has_cap ? std::optional<unsigned long long>(cap) : std::nullopt);
}

// out[5]: k0 and the grids of diag, panel, update (a side), write-back
extern "C" void ep_ease_step(int n, int block, int step, int64_t *out) {
    const EaseStep p = ease_step(shape_of(n, block), step);
    const int64_t v[5] = {p.k0, p.diag_grid, p.panel_grid, p.update_tiles, p.writeback_grid};
    memcpy(out, v, sizeof(v));
}
extern "C" int64_t ep_ease_launches(int n, int block) { return ease_launches(shape_of(n, block)); }

// out[10]: k0, cols, the grids of load, swap, transpose, the panel products' long and short side, update (a side), write-back; launches.
// elim[block]: per column j < cols the grid of the elimination launch after its pick, 0 where none follows (-1 from cols on)
extern "C" void ep_pivot_step(int n, int block, int step, int64_t *out, int *elim) {
    const EaseShape s = shape_of(n, block);
    const PivotStep p = pivot_step(s, step);
    const int64_t v[10] = {p.k0, p.cols, p.load_grid, p.swap_grid, p.transpose_grid, p.panel_grid_long, p.panel_grid_short, p.update_tiles, p.writeback_grid,
                           p.launches};
    memcpy(out, v, sizeof(v));
    for (int j = 0; j < block; ++j) elim[j] = j < p.cols ? pivot_elim_grid(s, p.k0, j) : -1;
}
extern "C" int64_t ep_pivot_launches(int n, int block, int gathered) { return pivot_launches(shape_of(n, block), gathered != 0); }

extern "C" void ep_inverse_permutation(const int *piv, int n, int npad, int *out) {
    const std::vector<int> p = inverse_column_permutation(piv, n, npad);
    memcpy(out, p.data(), p.size() * sizeof(int));
}

// out[3]: flops, bytes, units
extern "C" void ep_accounting(int n, int block, int cell_bytes, double *out) {
    const EaseAccounting a = invert_accounting(shape_of(n, block), (size_t)cell_bytes);
    const double v[3] = {a.flops, a.bytes, (double)a.units};
    memcpy(out, v, sizeof(v));
}
