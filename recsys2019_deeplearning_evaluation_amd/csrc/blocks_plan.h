// blocks_plan.h -- the host arithmetic of the two handles that keep a URM in both layouts and one dense block per side resident: PureSVD
// (svd.hip) and NMF (nmf.hip), on top of blocks.h / blocks.hip.  What is here: the constants the kernels share with the host, the
// lane-group width, the piece plan of a layout, the layout and value checks (they REPORT what they found; the .hip side words the
// refusal), every grid and buffer size, and the accounting of every step-wise call.
// Plain C++17 on plain numbers and host arrays -- no HIP header, no common.h -- so g++ builds it alone and tests/test_blocks_plan.py
// runs it without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mi355rec {
namespace blocks {

constexpr int SPLIT = 512;                 // nonzeros of the longest piece of a row
constexpr int SPMM_THREADS = 256;          // threads of the product kernel
constexpr int GT = 64;                     // side of a Gram tile
constexpr int GR = 16;                     // block rows staged per step of the Gram kernel
constexpr int NT = 256;                    // threads of every NMF kernel, of the Gram kernels and of the iota kernel
constexpr int RED_BLOCKS = 1024;           // workgroups of a grid-wide reduction, at most
constexpr int CS_SLABS = 512;              // row slabs of a column sum, at most
constexpr float EPS32 = 1.1920929e-07f;    // sklearn's EPSILON = np.finfo(np.float32).eps
constexpr int MIN_WIDTH = 1, MAX_WIDTH = 4096;                    // columns of a block (r of PureSVD, k of NMF)
// block * matrix is score.hip's gemm_rows_enqueue: 128 rows per workgroup, at most 65535 workgroups along that grid axis
constexpr int GEMM_ROWS_PER_BLOCK = 128, GEMM_MAX_BLOCKS = 65535;
constexpr int GEMM_MAX_ROWS = GEMM_ROWS_PER_BLOCK * GEMM_MAX_BLOCKS;   // 8 388 480: "more than 8 M rows on a side" is refused
constexpr size_t SWEEP_LDS_DEFAULT = 48 * 1024;                   // dynamic LDS a kernel may ask for without raising its attribute

inline int ceil_div(int64_t a, int64_t b) { return static_cast<int>((a + b - 1) / b); }

inline bool width_in_range(int r) { return r >= MIN_WIDTH && r <= MAX_WIDTH; }
inline bool rows_in_range(int n_users, int n_items) { return ceil_div(std::max(n_users, n_items), GEMM_ROWS_PER_BLOCK) <= GEMM_MAX_BLOCKS; }

// ---- the lane group ---------------------------------------------------------------------------------------------------------------
// A piece of a row (product, SDDMM) or a row of the block (sweep) belongs to a group of 16 / 32 / 64 lanes, chosen from the width so
// that narrow blocks pack 4 or 2 groups into a wavefront.  This is the only place the rule is written: the product grid, the SDDMM
// grid, the sweep's rows per workgroup and LDS bytes, and the cells of red_part all come from it.
inline int group_shift(int r) { return r <= 16 ? 4 : (r <= 32 ? 5 : 6); }

// workgroups of `threads` threads for n groups of 1 << group_shift(r) lanes
inline int group_grid(int n, int r, int threads) { return ceil_div((int64_t)n << group_shift(r), threads); }
inline int product_grid(int n_pieces, int r) { return group_grid(n_pieces, r, SPMM_THREADS); }
inline int sddmm_grid(int n_pieces, int k) { return group_grid(n_pieces, k, NT); }

// ---- the piece plan of one layout ---------------------------------------------------------------------------------------------------
// A row of the layout is cut into pieces of at most SPLIT cells, in cell order; an empty row is one empty piece.  A one-piece row
// writes its output row directly (slot -1); the pieces of a longer row write the partial rows first, first + 1, ... of its slots,
// which the long-rows kernel adds in that order.
struct PiecePlan {
    std::vector<int> row, begin, end, slot;                  // per piece
    std::vector<int> long_row, long_first, long_count;       // per row of more than one piece
    int n_slots = 0;
    int n_pieces() const { return (int)row.size(); }
    int n_long() const { return (int)long_row.size(); }
};

inline PiecePlan piece_plan(const int *row_ptr, int n) {
    PiecePlan p;
    p.row.reserve(n);
    for (int i = 0; i < n; ++i) {
        const int b = row_ptr[i], e = row_ptr[i + 1], len = e - b;
        const int parts = std::max(1, ceil_div(len, SPLIT));
        if (parts > 1) {
            p.long_row.push_back(i);
            p.long_first.push_back(p.n_slots);
            p.long_count.push_back(parts);
        }
        for (int q = 0; q < parts; ++q) {
            p.row.push_back(i);
            p.begin.push_back(b + q * SPLIT);
            p.end.push_back(std::min(e, b + (q + 1) * SPLIT));
            p.slot.push_back(parts > 1 ? p.n_slots++ : -1);
        }
    }
    return p;
}

// bytes a side uploads at create: the indices (and the values unless all are 1), four piece tables, three long-row tables
inline size_t side_upload_bytes(size_t nnz, bool ones, size_t n_pieces, size_t n_long) {
    return 4 * (nnz * (ones ? 1 : 2) + 4 * n_pieces + 3 * n_long);
}
inline int product_launches(int n_long) { return n_long ? 2 : 1; }      // the long-rows kernel runs only where a row has two pieces

// ---- what create looks at before it touches the device ------------------------------------------------------------------------------
// The product gathers block rows by the indices of a layout: pointers that decrease or an index outside the other side are refused.
struct LayoutFinding {
    enum Kind { OK, START_NOT_ZERO, POINTERS_DECREASE, INDEX_OUTSIDE } kind = OK;
    int at = 0;          // POINTERS_DECREASE: the row
    int index = 0;       // INDEX_OUTSIDE: the index found
};

inline LayoutFinding check_layout(int n, int n_other, const int *ptr, const int *idx) {
    if (ptr[0] != 0) return {LayoutFinding::START_NOT_ZERO, 0, 0};
    for (int i = 0; i < n; ++i)
        if (ptr[i] > ptr[i + 1]) return {LayoutFinding::POINTERS_DECREASE, i, 0};
    for (int j = 0, e = ptr[n]; j < e; ++j)
        if (idx[j] < 0 || idx[j] >= n_other) return {LayoutFinding::INDEX_OUTSIDE, j, idx[j]};
    return {};
}

// all-ones URMs skip the value stream of the product
inline bool all_ones(const float *val, size_t nnz) {
    bool ones = true;
    for (size_t i = 0; i < nnz && ones; ++i) ones = val[i] == 1.0f;
    return ones;
}

// NMF's scan: stops at the first negative value (the figures are then those of the cells before it); the float64 sums are taken in
// storage order.  norm_x = sum of x^2, sum_x = sum of the x above eps32 (what the Kullback-Leibler divergence counts).
struct ValueScan {
    bool ones = true, negative = false;
    size_t negative_at = 0;
    float negative_value = 0.f;
    double norm_x = 0.0, sum_x = 0.0;
};

inline ValueScan scan_values(const float *val, size_t nnz) {
    ValueScan s;
    for (size_t i = 0; i < nnz; ++i) {
        if (!(val[i] >= 0.f)) {
            s.negative = true;
            s.negative_at = i;
            s.negative_value = val[i];
            return s;
        }
        s.ones = s.ones && val[i] == 1.0f;
        s.norm_x += (double)val[i] * val[i];
        if (val[i] > EPS32) s.sum_x += val[i];
    }
    return s;
}

// ---- the float64 Gram matrix G = X^T X of a block of n rows -------------------------------------------------------------------------
// 64 x 64 tiles of the upper triangle, a slab of `rows` rows per workgroup, the slabs' partial tiles added in slab order.
struct GramPlan {
    int slabs = 0, rows = 0;
    size_t make(int n, int r) {                          // returns the float64 cells `gram_part` needs
        const int nt = ceil_div(r, GT), pairs = nt * (nt + 1) / 2;
        slabs = std::max(1, std::min(ceil_div(n, 4 * GR), 1024 / pairs));
        rows = ceil_div(ceil_div(n, slabs), GR) * GR;
        slabs = ceil_div(n, rows);
        return (size_t)slabs * r * r;
    }
};
inline int gram_tiles(int r) { return ceil_div(r, GT); }                       // the Gram grid is (tiles, tiles, slabs)
inline int gram_reduce_grid(int r) { return ceil_div((int64_t)r * r, NT); }
constexpr int GRAM_LAUNCHES = 2;

// ---- NMF's float64 reductions ---------------------------------------------------------------------------------------------------------
// column sums: `used` slabs of `rows` rows; colsum_part holds CS_SLABS rows of k cells
struct ColsumPlan {
    int slabs = 0, rows = 0, used = 0;
};
inline ColsumPlan colsum_plan(int n) {
    ColsumPlan p;
    p.slabs = std::min(CS_SLABS, ceil_div(n, 64));
    p.rows = ceil_div(n, p.slabs);
    p.used = ceil_div(n, p.rows);
    return p;
}
inline int column_grid(int k) { return ceil_div(k, NT); }                     // one thread per column
inline int cell_grid(size_t cells) { return ceil_div((int64_t)cells, NT); }   // one thread per cell (scale, fill, to_float)
constexpr int COLSUM_LAUNCHES = 2;

// a dot product of `len` cells: every workgroup a contiguous share, one float64 sum per workgroup into red_part
inline int dot_blocks(size_t len) { return std::max(1, std::min<int>(RED_BLOCKS, ceil_div((int64_t)len, 4 * NT))); }
constexpr int DOT_LAUNCHES = 2;

// ---- one half-sweep of coordinate descent over a block of n rows ----------------------------------------------------------------------
// A row per lane group; the rows of a workgroup sit in dynamic LDS, ceil(k / lanes) floats per thread: at most 64 KiB (k = 4096),
// next to 2 KiB of static LDS.  Above SWEEP_LDS_DEFAULT the kernel's attribute must be raised before the launch.
struct SweepPlan {
    int shift = 0, rows_per_block = 0, blocks = 0;
    size_t lds_bytes = 0;
    bool raise_attribute = false;
};
inline SweepPlan sweep_plan(int n, int k) {
    SweepPlan p;
    p.shift = group_shift(k);
    p.rows_per_block = NT >> p.shift;
    p.blocks = ceil_div(n, p.rows_per_block);
    p.lds_bytes = (size_t)ceil_div(k, 1 << p.shift) * NT * sizeof(float);
    p.raise_attribute = p.lds_bytes > SWEEP_LDS_DEFAULT;
    return p;
}

// red_part holds one float64 per workgroup of whichever launch last wrote it at blockIdx.x.  INVARIANT: its cells cover the grid of
// every such launch -- the sweep on either side (sweep_plan(n, k).blocks = ceil(n << shift / NT), n <= n_max), the SDDMM on either
// side (sddmm_grid(n_pieces, k)) and the dot products (dot_blocks(len) <= RED_BLOCKS).  tests/test_blocks_plan.py checks it.
inline size_t red_part_cells(int n_pieces_users, int n_pieces_items, int n_max, int k) {
    const int64_t most = std::max<int64_t>(std::max(n_pieces_users, n_pieces_items), n_max);
    return (size_t)std::max<int64_t>(RED_BLOCKS, ceil_div(most << group_shift(k), NT));
}

// ---- the buffers both handles allocate at create ----------------------------------------------------------------------------------------
struct PairSizes {
    int n_max = 0;
    size_t cap = 0;              // cells of a block (and of every buffer that stands in for one): the longer side
    size_t partial_rows = 0;     // rows of `partial`: the slots of the side with more of them, at least 1
    size_t gram_part_cells = 0;  // the larger of the two sides' Gram plans, at least 1
};
inline PairSizes pair_sizes(int n_users, int n_items, int r, int n_slots_users, int n_slots_items, GramPlan gram_plan[2]) {
    PairSizes z;
    z.n_max = std::max(n_users, n_items);
    z.cap = (size_t)z.n_max * r;
    z.partial_rows = (size_t)std::max(1, std::max(n_slots_users, n_slots_items));
    z.gram_part_cells = std::max<size_t>(1, std::max(gram_plan[0].make(n_users, r), gram_plan[1].make(n_items, r)));
    return z;
}

// ---- accounting -----------------------------------------------------------------------------------------------------------------------
// bytes over PCIe of the step-wise calls
inline int64_t block_bytes(int rows, int r) { return (int64_t)((size_t)rows * r * sizeof(float)); }      // set_block, get_block
inline int64_t gram_download_bytes(int r) { return (int64_t)r * r * sizeof(double); }
inline int64_t apply_upload_bytes(int r) { return (int64_t)r * r * sizeof(float); }
inline int64_t permutation_bytes(int k) { return (int64_t)k * sizeof(int); }
constexpr int64_t SCALAR_BYTES = sizeof(double);                  // a violation or a divergence coming back

// launches a call adds to the handle's count
constexpr int APPLY_LAUNCHES = 1, FILL_LAUNCHES = 1;
inline int prepare_frobenius_launches(int n_long) { return GRAM_LAUNCHES + 1 + product_launches(n_long); }     // Gram, to_float, product
inline int sweep_launches(bool reuse, int n_long) { return (reuse ? 0 : prepare_frobenius_launches(n_long)) + 2; }   // sweep, sum
inline int mu_step_launches(int loss, bool reuse, int n_long) {
    if (loss == 0) return (reuse ? 0 : prepare_frobenius_launches(n_long)) + 2;                          // GEMM, scale
    return (reuse ? 0 : COLSUM_LAUNCHES) + 1 + product_launches(n_long) + 1;                             // SDDMM, product, scale
}
inline int divergence_launches(int loss, int n_long_users) {
    if (loss == 0) return 2 * GRAM_LAUNCHES + DOT_LAUNCHES + product_launches(n_long_users) + DOT_LAUNCHES + 1;
    return 1 + 1 + 2 * COLSUM_LAUNCHES + DOT_LAUNCHES + 1;                                              // SDDMM, sum, ..., divergence
}

// algorithmic bytes and flops of a call (n_units is nnz for every one of them)
struct CallFigures {
    double bytes = 0.0, flops = 0.0;
};
// a gathered row of the block, an index and a value per cell
inline CallFigures product_figures(size_t nnz, int r) { return {(double)nnz * (4.0 * r + 8.0), 2.0 * (double)nnz * r}; }
// the sweep reads a row of HHt per row and step from the cache: its traffic is the block twice and XHt once
inline CallFigures sweep_figures(int n, int k) { return {12.0 * n * k, 2.0 * (double)n * k * k}; }
inline CallFigures mu_frobenius_figures(size_t cells, int k) { return {16.0 * cells, 2.0 * (double)cells * k}; }
inline CallFigures mu_kl_figures(size_t nnz, int k) { return {(double)nnz * (4.0 * k + 12.0), 2.0 * (double)nnz * k}; }
inline CallFigures fill_figures(size_t cells) { return {4.0 * cells, 0.0}; }
inline CallFigures divergence_figures(size_t nnz, int k) { return product_figures(nnz, k); }

}  // namespace blocks
}  // namespace mi355rec
