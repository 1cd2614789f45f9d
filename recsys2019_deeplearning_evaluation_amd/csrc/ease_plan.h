// ease_plan.h -- the host arithmetic of the EASE_R closed form: the environment's knobs (EaseKnobs, parsed in ONE place), the padded
// shape, the bytes of the handle and of the pivoted route's workspace with the verdicts "does it fit", the launch geometry of every
// elimination step of both routes and their launch counts, the permutation that undoes the pivoted route's row swaps, the accounting
// -- and the constants the kernels share with it.
// Plain C++17 on plain numbers -- no HIP call; the free memory of the device comes in as an argument -- so g++ builds it and
// tests/test_ease_plan.py runs it without a GPU.  Included by ease.hip and ease_pivot.hip (through ease_handle.h).
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <optional>
#include <utility>
#include <vector>

namespace mi355rec {
namespace ease {

// ---- constants shared with the kernels -------------------------------------------------------------------------------------------
constexpr int EASE_TILE = 128;      // cells of a side of the update kernels' tile; the matrix is padded to a multiple of it, its tail carries an identity block
constexpr int TK = 32;              // K chunk of ease_update_kernel staged in LDS
constexpr int PANEL_W = 64;         // columns (rows) one workgroup of ease_panel_kernel and of the write-backs handles
constexpr int CHUNK = 64;           // rows of the panel one workgroup of the pivot search handles
constexpr int GK = 16;              // K chunk of ease_gemm64_kernel staged in LDS
// NOT shared: three kernels of ease_pivot_kernels.cuh keep literals of their own, and these host-side names for the grids below MUST
// MIRROR them (ease_pivot.hip asserts the tile sides against the TS it instantiates; the other two have no name to assert against)
constexpr int SWAP_W = 128;         // ease_pivot_swap_kernel: `blockIdx.x * 128`, __launch_bounds__(128) -- also the launch's block size
constexpr int TRANSPOSE_W = 32;     // ease_transpose64_kernel: `blockIdx.x * 32`, t[32][NB + 1]
constexpr int SMALL_T = 64;         // ease_gemm64_kernel<2, .>: T = 32 * TS, the tile that forms the panels R and ND

// ---- the environment ------------------------------------------------------------------------------------------------------------
// MI355REC_EASE_BLOCK as atoi reads it (an empty or non-numeric value is a 0, which is refused); MI355REC_EASE_PIVOT_MAX_BYTES, the
// cap a process that shares the device puts on the pivoted route's workspace, as strtoull reads it (an empty or non-numeric value is
// a cap of 0 bytes).  The create call uses `block` of its reading, the first allocation of a handle's workspace `pivot_max_bytes` of its own.
struct EaseKnobs {
    int block = EASE_TILE;
    std::optional<unsigned long long> pivot_max_bytes;
};
constexpr const char *EASE_BLOCK_MESSAGE = "MI355REC_EASE_BLOCK must be 64 or 128, got %d";
inline bool ease_block_valid(int block) { return block == 64 || block == 128; }

// the only place of ease.hip, ease_pivot.hip and their headers that reads the environment
inline EaseKnobs read_ease_knobs() {
    EaseKnobs k;
    if (const char *v = getenv("MI355REC_EASE_BLOCK")) k.block = atoi(v);
    if (const char *v = getenv("MI355REC_EASE_PIVOT_MAX_BYTES")) k.pivot_max_bytes = strtoull(v, nullptr, 10);
    return k;
}

// ---- the shape ------------------------------------------------------------------------------------------------------------------
// n items in an npad x npad buffer, npad = n rounded up to EASE_TILE; one elimination step per block column of `block` cells.
struct EaseShape {
    int n = 0, npad = 0, block = 0, steps = 0;
};
// nothing where npad does not fit an int ("too many items")
inline std::optional<EaseShape> ease_shape(int n_items, int block) {
    const int64_t npad = ((int64_t)n_items + EASE_TILE - 1) / EASE_TILE * EASE_TILE;
    if (npad > INT32_MAX) return std::nullopt;
    return EaseShape{n_items, (int)npad, block, (int)(npad / block)};
}

// ---- bytes, and whether they fit --------------------------------------------------------------------------------------------------
// the matrix, the three panels and the diagonal block, and -- where n is not a multiple of the tile -- the slab in which
// mi355rec_sim_compute_dense_device builds its unpadded columns before it copies them to the pitch of the matrix
inline size_t ease_bytes(const EaseShape &s) {
    const int64_t n = s.n, npad = s.npad;
    return (size_t)(npad * npad + 3 * npad * s.block + (int64_t)s.block * s.block + (npad != n ? n * n : 0)) * sizeof(float);
}
// the pivoted route's float64 workspace: the working matrix, the scratch panel and the three panels, D and its transpose
inline size_t pivot_bytes(const EaseShape &s) {
    const int64_t npad = s.npad;
    return (size_t)(npad * npad + 4 * npad * s.block + 2 * (int64_t)s.block * s.block) * sizeof(double);
}
constexpr size_t EASE_RESERVE = (size_t)256 << 20;      // next to the handle: outputs and the runtime
constexpr size_t PIVOT_RESERVE = (size_t)64 << 20;      // next to the workspace: the small buffers' rounding and the runtime

enum class EaseFit { FITS, NO_ROOM, OVER_CAP };
inline EaseFit ease_fit(size_t need, size_t free_bytes) { return need + EASE_RESERVE <= free_bytes ? EaseFit::FITS : EaseFit::NO_ROOM; }
// the cap is looked at first: a workspace above it is refused however much memory is free
inline EaseFit pivot_fit(size_t need, size_t free_bytes, const std::optional<unsigned long long> &cap) {
    if (cap && need > *cap) return EaseFit::OVER_CAP;
    return need + PIVOT_RESERVE > free_bytes ? EaseFit::NO_ROOM : EaseFit::FITS;
}

// dynamic LDS of ease_panel_kernel<NB>: Ds[NB][NB + 4], Xs[NB][PANEL_W], Ys[PANEL_W][NB + 4]
inline size_t panel_lds_bytes(int block) { return (size_t)(block * (block + 4) + block * PANEL_W + PANEL_W * (block + 4)) * sizeof(float); }

// ---- the steps of the unpivoted route ---------------------------------------------------------------------------------------------
// diag, panel, update (a square grid of `update_tiles` a side), write-back: every tile and every panel is whole
struct EaseStep {
    int k0, diag_grid, panel_grid, update_tiles, writeback_grid;
};
constexpr int EASE_STEP_LAUNCHES = 4;
inline EaseStep ease_step(const EaseShape &s, int step) { return {step * s.block, 1, s.npad / PANEL_W, s.npad / EASE_TILE, s.npad / PANEL_W}; }
inline int64_t ease_launches(const EaseShape &s) { return EASE_STEP_LAUNCHES * (int64_t)s.steps; }
constexpr int WEIGHTS_LAUNCHES = 2, TOPK_LAUNCHES = 1;      // get-diagonal + weights, once per inverse; every top-K call

// ---- the steps of the pivoted route -----------------------------------------------------------------------------------------------
// The pivot search of step k runs over the rows k0 .. n - 1 in chunks of CHUNK rows, last_chunk = (n - 1) / CHUNK: the load kernel
// over the chunks from k0's on; per column j < cols one pick (one workgroup) and -- unless it is the last column of a full panel
// (nothing to its right) or row g = k0 + j is the last row (nothing below) -- one elimination launch over the chunks from row g + 1's on.
struct PivotStep {
    int k0, cols;                       // cols <= 0: the block lies in the identity tail, nothing is searched or swapped
    int load_grid, swap_grid;           // (0 where cols <= 0)
    int transpose_grid, panel_grid_long, panel_grid_short, update_tiles, writeback_grid;      // the block step: R is (long, short), ND (short, long)
    int launches;
};
constexpr int PIVOT_BLOCK_LAUNCHES = 6, PIVOT_FRONT_LAUNCHES = 2, PIVOT_GATHER_LAUNCHES = 1;      // diag .. write-back; init + widen; gather

// workgroups of the elimination launch after the pick of column j of the panel at k0; 0: no launch follows
inline int pivot_elim_grid(const EaseShape &s, int k0, int j) {
    const int g = k0 + j, last_chunk = (s.n - 1) / CHUNK;
    if (!(j + 1 < s.block && g + 1 < s.n)) return 0;
    return last_chunk - (g + 1) / CHUNK + 1;
}

inline PivotStep pivot_step(const EaseShape &s, int step) {
    PivotStep p{};
    p.k0 = step * s.block;
    p.cols = std::min(s.block, s.n - p.k0);
    p.transpose_grid = s.npad / TRANSPOSE_W;
    p.panel_grid_long = s.npad / SMALL_T;
    p.panel_grid_short = s.block / SMALL_T;
    p.update_tiles = s.npad / EASE_TILE;
    p.writeback_grid = s.npad / PANEL_W;
    p.launches = PIVOT_BLOCK_LAUNCHES;
    if (p.cols > 0) {
        p.load_grid = (s.n - 1) / CHUNK - p.k0 / CHUNK + 1;
        p.swap_grid = s.npad / SWAP_W;
        p.launches += 2 + p.cols;                              // load, swap, a pick per column
        for (int j = 0; j < p.cols; ++j) p.launches += pivot_elim_grid(s, p.k0, j) > 0;
    }
    return p;
}

// launches of a whole pivoted inverse: init and widen in front, every step, and the gather when no step failed
inline int64_t pivot_launches(const EaseShape &s, bool gathered) {
    int64_t total = PIVOT_FRONT_LAUNCHES + (gathered ? PIVOT_GATHER_LAUNCHES : 0);
    for (int step = 0; step < s.steps; ++step) total += pivot_step(s, step).launches;
    return total;
}

// ---- the permutation ----------------------------------------------------------------------------------------------------------------
// piv[g], g < n: the row swapped with row g, in order.  Row g of the permuted matrix is row order[g] of the original; (P G)^-1 = G^-1
// P^T, so column order[l] of G^-1 is column l of what was computed: the swaps undone on the columns, last first.  inv_perm[j]: the
// column of the result that holds column j of the inverse.
inline std::vector<int> inverse_column_permutation(const int *piv, int n, int npad) {
    std::vector<int> order((size_t)npad), inv_perm((size_t)npad);
    for (int i = 0; i < npad; ++i) order[i] = i;
    for (int g = 0; g < n; ++g)
        if (piv[g] != g) std::swap(order[g], order[piv[g]]);
    for (int l = 0; l < npad; ++l) inv_perm[order[l]] = l;
    return inv_perm;
}

// ---- accounting -----------------------------------------------------------------------------------------------------------------
// ALGORITHMIC work of an inverse: 2 n^3 flop; every step reads and writes the matrix once, 4 bytes a cell (the float64 working
// matrix of the pivoted route: 8)
struct EaseAccounting {
    double flops, bytes;
    int units;
};
inline EaseAccounting invert_accounting(const EaseShape &s, size_t cell_bytes) {
    return {2.0 * (double)s.n * s.n * s.n, 2.0 * (double)cell_bytes * (double)s.n * s.n * s.steps, s.steps};
}

}  // namespace ease
}  // namespace mi355rec
