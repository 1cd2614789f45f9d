// asy_estimate_plan.h -- the host arithmetic of AsySVD's user-factor estimate on the device (asy_estimate.hip: asy_estimate_kernel behind
// mi355rec_mf_asy_user_factors and mi355rec_asy_user_factors).  What is here: how the n_rows x k output cells are laid over lanes (factors
// per lane, the width of the lane group that shares a row, column tiles, rows per workgroup, the grid), the order the rows are handed out
// in, the argument checks of the stateless entry and the bytes a call accounts for.
// Plain C++17 on plain numbers and host arrays -- no HIP header, no common.h -- so g++ builds it alone and tests/test_asysvd_estimate_spec.py
// runs tests/asy_estimate_plan_main.cpp under the host sanitizers without a GPU.
#pragma once

#include <cstddef>
#include <cstdint>

#include "spscorer_plan.h"      // check_csr: the check of a host CSR that reports the first bad row

namespace mi355rec {
namespace asy_estimate_plan {

constexpr int KMAX = 256;            // the most factors an ASY_SVD handle takes (mf_plan.h: ASY_KMAX; mf.hip asserts they are one number)
constexpr int THREADS = 256;         // lanes of a workgroup
constexpr int MAX_GROUP = 64;        // lanes of the widest group: one wavefront
constexpr int DEPTH = 8;             // rows of Y a lane requests before the first of them is added (8 x 16 bytes per lane in flight)

// ---- the lane mapping -------------------------------------------------------------------------------------------------------------------
// The parallelism is the output cells: a cell's additions are one chain in storage order, so a row is never split and nothing is reduced
// across lanes.  A lane owns `vec` adjacent factors of one row: two (one 16-byte load per row of Y) where k is even -- every row of Y
// and of the output then starts on a 16-byte boundary -- and one otherwise.  `group` lanes, a power of two up to a wavefront, share a row:
// they read its ids and values coalesced, `group` cells a step and one cell per lane, and hand them round with __shfl.  A k beyond
// group x vec factors is cut into `tiles` column tiles, each an item of work of its own (it walks the row again: 8 bytes per cell
// beside group x vec x 8 of Y).  A workgroup holds THREADS / group items; item i is tile i % tiles of the (i / tiles)-th longest row.
struct Layout {
    int vec = 0, group = 0, tiles = 0, items_per_block = 0;
    long long items = 0, grid = 0;
};

inline int factors_per_lane(int k) { return k % 2 == 0 ? 2 : 1; }

inline int group_width(int k) {
    const int slots = (k + factors_per_lane(k) - 1) / factors_per_lane(k);
    int g = 1;
    while (g < slots && g < MAX_GROUP) g *= 2;
    return g;
}

inline Layout layout(long long n_rows, int k) {
    Layout l;
    l.vec = factors_per_lane(k);
    l.group = group_width(k);
    const int tile = l.group * l.vec;
    l.tiles = (k + tile - 1) / tile;
    l.items_per_block = THREADS / l.group;
    l.items = n_rows * l.tiles;
    l.grid = (l.items + l.items_per_block - 1) / l.items_per_block;
    return l;
}

// ---- the order of the rows ----------------------------------------------------------------------------------------------------------------
// Rows are handed out longest first (workgroups start in grid order), so that one profile of thousands of cells does not end the launch
// alone, and the groups that share a wavefront walk rows of nearly one length.  A counting sort on the length, stable: rows of one length
// keep their order.  `order` has n_rows entries; `count` is scratch of max_length + 2 entries (max_length: the longest row, what
// longest_row returns).  The pointers must have passed check_csr.
inline int longest_row(int n_rows, const int32_t *indptr) {
    int longest = 0;
    for (int r = 0; r < n_rows; ++r) longest = indptr[r + 1] - indptr[r] > longest ? indptr[r + 1] - indptr[r] : longest;
    return longest;
}

inline void longest_first(int n_rows, const int32_t *indptr, int max_length, int32_t *count, int32_t *order) {
    for (int l = 0; l <= max_length + 1; ++l) count[l] = 0;
    for (int r = 0; r < n_rows; ++r) ++count[indptr[r + 1] - indptr[r]];
    // count[l] <- the position of the first row of length l: the rows longer than l come before it
    int32_t before = 0;
    for (int l = max_length; l >= 0; --l) {
        const int32_t here = count[l];
        count[l] = before;
        before += here;
    }
    for (int r = 0; r < n_rows; ++r) order[count[indptr[r + 1] - indptr[r]]++] = r;
}

// ---- the argument checks ----------------------------------------------------------------------------------------------------------------
// (the grid needs no check of its own: a second tile comes with 64-lane groups only, KMAX is four tiles and such a workgroup holds
// four items, so a launch never has more workgroups than the matrix has rows -- an int32)
enum Refusal { OK, EMPTY_SHAPE, K_RANGE };

inline Refusal check_shape(long long n_rows, long long n_items, int k) {
    if (n_rows <= 0 || n_items <= 0) return EMPTY_SHAPE;
    if (k < 1 || k > KMAX) return K_RANGE;
    return OK;
}

// the stateless entry's CSR: pointers that climb from 0 and ids inside [0, n_items); the rows are taken as they are stored, sorted or not
inline spscorer_plan::CsrFinding check_csr(int n_rows, int n_items, const int32_t *indptr, const int32_t *indices) {
    return spscorer_plan::check_csr(n_rows, n_items, indptr, indices, false);
}

// ---- accounting: bytes read + written on the device ---------------------------------------------------------------------------------------
// every stored cell reads one row of Y (k float64), its id and its value; every output cell is written once
inline double bytes(long long nnz, long long n_rows, int k) { return (double)nnz * (8.0 * k + 8.0) + 8.0 * (double)n_rows * k; }

}  // namespace asy_estimate_plan
}  // namespace mi355rec
