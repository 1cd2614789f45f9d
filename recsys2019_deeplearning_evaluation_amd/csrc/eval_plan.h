// eval_plan.h -- the index arithmetic of DIVERSITY_SIMILARITY (Base/Evaluation/metrics.py:641-694 Diversity_similarity) that can be
// wrong without a GPU: where a cell of the item diversity matrix lies, which shell of a list a cell belongs to, how the shells are cut
// into the runs the kernel's threads walk, how many shells a cutoff sums for a list of a given length, the byte sizes and the width
// limit.  Plain C++ on plain numbers, host and device: eval_diversity.cuh and mi355rec_eval_set_diversity use it, g++ builds it and
// tests/test_evaluation_diversity_cpu.py runs it without a GPU.
//
// The reference's value of one list `items` of length L (the first min(cutoff, list length) entries):
//     ( sum over i = 0 .. L-2, j = 0 .. L-1, j != i of D[items[i], items[j]] ) / (L (L - 1))
// The last position never gives a row, j != i is by position, D is indexed [row = items[i], column = items[j]].  Cell (i, j) is part of
// every L >= max(i + 2, j + 1), so it is given to shell k = max(i + 1, j), 1 <= k <= L - 1: a list of length L sums the shells 1 .. L-1.
// Shell k holds 2k - 1 cells, as two runs:
//     column run  (i, k) for i = 0 .. k-1      k cells      run 2 (k - 1)
//     row run     (k-1, j) for j = 0 .. k-2    k - 1 cells  run 2 (k - 1) + 1
#pragma once

#include <cstddef>
#include <cstdint>

#ifndef MI355REC_HD
#if defined(__HIPCC__)
#define MI355REC_HD __host__ __device__
#else
#define MI355REC_HD
#endif
#endif

namespace mi355rec {
namespace evalplan {

constexpr int DIV_MAX_WIDTH = 1024;                     // the list's ids and its run sums live in LDS; the work is L^2 gathers per user
constexpr int DIV_SMALL_WIDTH = 64;                     // up to here one wavefront per user, above it four
constexpr size_t DIV_UPLOAD_CHUNK = (size_t)256 << 20;  // bytes per host-to-device copy of the matrix

MI355REC_HD inline bool div_width_ok(int width) { return width >= 1 && width <= DIV_MAX_WIDTH; }
MI355REC_HD inline bool div_elem_ok(int elem_bytes) { return elem_bytes == 4 || elem_bytes == 8; }
MI355REC_HD inline int div_threads(int width) { return width <= DIV_SMALL_WIDTH ? 64 : 256; }

// cells, not bytes: row_item * n_items passes 2^31 from 46 341 items on
MI355REC_HD inline uint64_t div_cell_offset(int row_item, int col_item, int n_items) {
    return (uint64_t)(uint32_t)row_item * (uint64_t)(uint32_t)n_items + (uint64_t)(uint32_t)col_item;
}

MI355REC_HD inline int div_shell(int i, int j) { return i + 1 > j ? i + 1 : j; }    // of cell (i, j), i != j

// One run of a shell: `count` cells, cell q of it is (q, fixed) in a column run and (fixed, q) in a row run.
struct DivRun {
    int shell, fixed, count;
    bool column;
};
MI355REC_HD inline int div_run_count(int len) { return len >= 2 ? 2 * (len - 1) : 0; }     // runs of a list of `len` items
MI355REC_HD inline DivRun div_run(int w) {
    const int k = w / 2 + 1;
    return (w & 1) ? DivRun{k, k - 1, k - 1, false} : DivRun{k, k, k, true};
}
MI355REC_HD inline uint64_t div_run_cell(const DivRun &r, const int *items, int q, int n_items) {
    return r.column ? div_cell_offset(items[q], items[r.fixed], n_items) : div_cell_offset(items[r.fixed], items[q], n_items);
}

// What a cutoff sees of a list of `len` items: its length, and the shells 1 .. div_cutoff_shells() it sums (-1: fewer than two
// items, the reference divides by zero there).
MI355REC_HD inline int div_cutoff_length(int cutoff, int len) { return cutoff < len ? cutoff : len; }
MI355REC_HD inline int div_cutoff_shells(int cutoff, int len) {
    const int l = div_cutoff_length(cutoff, len);
    return l >= 2 ? l - 1 : -1;
}
MI355REC_HD inline double div_denominator(int cutoff, int len) {
    const int l = div_cutoff_length(cutoff, len);
    return (double)((int64_t)l * (l - 1));
}

// ---- sizes ------------------------------------------------------------------------------------------------------------------------
MI355REC_HD inline uint64_t div_matrix_cells(int n_items) { return (uint64_t)(uint32_t)n_items * (uint64_t)(uint32_t)n_items; }
MI355REC_HD inline uint64_t div_matrix_bytes(int n_items, int elem_bytes) { return div_matrix_cells(n_items) * (uint64_t)elem_bytes; }
MI355REC_HD inline uint64_t div_value_cells(int n_eval, int n_cut) { return (uint64_t)(uint32_t)n_eval * (uint64_t)(uint32_t)n_cut; }
MI355REC_HD inline uint64_t div_upload_chunks(uint64_t bytes) { return (bytes + DIV_UPLOAD_CHUNK - 1) / DIV_UPLOAD_CHUNK; }
// grid of the range check: 256 threads a block, at most 4096 blocks, each thread strides over the cells
MI355REC_HD inline int div_range_blocks(uint64_t cells) {
    const uint64_t blocks = (cells + 256 * 8 - 1) / (256 * 8);
    return blocks < 1 ? 1 : (blocks > 4096 ? 4096 : (int)blocks);
}

}  // namespace evalplan
}  // namespace mi355rec
