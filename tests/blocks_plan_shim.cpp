// extern "C" wrapper around csrc/blocks_plan.h for tests/test_blocks_plan.py and tests/test_block_pair_gpu.py, which compile it with
// g++ and call it through ctypes: no GPU, no HIP runtime.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/blocks_plan.h"

#include <cstring>

using namespace mi355rec::blocks;

extern "C" void bp_constants(int64_t *out) {
    const int64_t v[11] = {SPLIT, SPMM_THREADS, GT, GR, NT, RED_BLOCKS, CS_SLABS, MIN_WIDTH, MAX_WIDTH, GEMM_MAX_ROWS, (int64_t)SWEEP_LDS_DEFAULT};
    memcpy(out, v, sizeof(v));
}

// out[5]: the group shift of a width, whether create takes the width, Gram tiles per side, grid of the Gram reduction, of a per-column kernel
extern "C" void bp_width(int r, int64_t *out) {
    const int64_t v[5] = {group_shift(r), width_in_range(r), gram_tiles(r), gram_reduce_grid(r), column_grid(r)};
    memcpy(out, v, sizeof(v));
}

extern "C" int bp_rows_in_range(int n_users, int n_items) { return rows_in_range(n_users, n_items); }

// The piece plan of a layout of n rows.  The arrays hold `room` entries each; counts[4]: pieces, long rows, slots, upload bytes of the
// side with real values.  Returns 0 where the arrays are too short (nothing is written then).
extern "C" int bp_pieces(const int *row_ptr, int n, int room, int *row, int *begin, int *end, int *slot, int *long_row, int *long_first,
                         int *long_count, int64_t *counts) {
    const PiecePlan p = piece_plan(row_ptr, n);
    if (p.n_pieces() > room || p.n_long() > room) return 0;
    const size_t pb = p.row.size() * sizeof(int), lb = p.long_row.size() * sizeof(int);
    if (pb) memcpy(row, p.row.data(), pb), memcpy(begin, p.begin.data(), pb), memcpy(end, p.end.data(), pb), memcpy(slot, p.slot.data(), pb);
    if (lb) memcpy(long_row, p.long_row.data(), lb), memcpy(long_first, p.long_first.data(), lb), memcpy(long_count, p.long_count.data(), lb);
    const int64_t v[4] = {p.n_pieces(), p.n_long(), p.n_slots, (int64_t)side_upload_bytes((size_t)row_ptr[n], false, p.row.size(), p.long_row.size())};
    memcpy(counts, v, sizeof(v));
    return 1;
}

extern "C" int64_t bp_upload_bytes(int64_t nnz, int ones, int64_t n_pieces, int64_t n_long) {
    return (int64_t)side_upload_bytes((size_t)nnz, ones != 0, (size_t)n_pieces, (size_t)n_long);
}

// out[3]: what the layout check found (0 nothing, 1 the pointers do not start at 0, 2 they decrease, 3 an index outside), the row of
// the decrease, the index found outside
extern "C" void bp_layout(int n, int n_other, const int *ptr, const int *idx, int64_t *out) {
    const LayoutFinding f = check_layout(n, n_other, ptr, idx);
    const int64_t v[3] = {f.kind, f.kind == LayoutFinding::POINTERS_DECREASE ? f.at : 0, f.kind == LayoutFinding::INDEX_OUTSIDE ? f.index : 0};
    memcpy(out, v, sizeof(v));
}

// flags[4]: PureSVD's all-ones scan, NMF's all-ones, whether NMF found a negative value, its position; sums[3]: that value, norm_x, sum_x
extern "C" void bp_values(const float *val, int64_t nnz, int64_t *flags, double *sums) {
    const ValueScan s = scan_values(val, (size_t)nnz);
    const int64_t v[4] = {all_ones(val, (size_t)nnz), s.negative ? 0 : s.ones, s.negative, s.negative ? (int64_t)s.negative_at : 0};
    const double d[3] = {s.negative ? (double)s.negative_value : 0.0, s.negative ? 0.0 : s.norm_x, s.negative ? 0.0 : s.sum_x};
    memcpy(flags, v, sizeof(v));
    memcpy(sums, d, sizeof(d));
}

// out[3]: slabs, rows per slab, float64 cells of the partial tiles
extern "C" void bp_gram(int n, int r, int64_t *out) {
    GramPlan g;
    const size_t cells = g.make(n, r);
    const int64_t v[3] = {g.slabs, g.rows, (int64_t)cells};
    memcpy(out, v, sizeof(v));
}

// out[3]: slabs, rows per slab, slabs used
extern "C" void bp_colsum(int n, int64_t *out) {
    const ColsumPlan p = colsum_plan(n);
    const int64_t v[3] = {p.slabs, p.rows, p.used};
    memcpy(out, v, sizeof(v));
}

extern "C" int bp_dot_blocks(int64_t len) { return dot_blocks((size_t)len); }
extern "C" int bp_cell_grid(int64_t cells) { return cell_grid((size_t)cells); }

// out[5]: group shift, rows per workgroup, workgroups, dynamic LDS bytes, whether the kernel's attribute must be raised
extern "C" void bp_sweep(int n, int k, int64_t *out) {
    const SweepPlan p = sweep_plan(n, k);
    const int64_t v[5] = {p.shift, p.rows_per_block, p.blocks, (int64_t)p.lds_bytes, p.raise_attribute};
    memcpy(out, v, sizeof(v));
}

// out[2]: grid of the product, grid of the SDDMM
extern "C" void bp_piece_grids(int n_pieces, int r, int64_t *out) {
    const int64_t v[2] = {product_grid(n_pieces, r), sddmm_grid(n_pieces, r)};
    memcpy(out, v, sizeof(v));
}

extern "C" int64_t bp_red_part_cells(int n_pieces_users, int n_pieces_items, int n_max, int k) {
    return (int64_t)red_part_cells(n_pieces_users, n_pieces_items, n_max, k);
}

// out[6]: rows of the longer side, cells of a block buffer, rows of `partial`, cells of `gram_part`, Gram slabs of either side
extern "C" void bp_sizes(int n_users, int n_items, int r, int n_slots_users, int n_slots_items, int64_t *out) {
    GramPlan g[2];
    const PairSizes z = pair_sizes(n_users, n_items, r, n_slots_users, n_slots_items, g);
    const int64_t v[6] = {z.n_max, (int64_t)z.cap, (int64_t)z.partial_rows, (int64_t)z.gram_part_cells, g[0].slabs, g[1].slabs};
    memcpy(out, v, sizeof(v));
}

// The accounting of every call at one shape; long[2]: rows of more than one piece on the users' and on the items' layout.
// counts[25]: PCIe bytes of set_block / get_block per side, of a Gram download, an apply upload, a permutation, a scalar;
//             launches of product per side, gram, apply, fill; of a sweep per (reuse, side); of a MU step per (loss, reuse, side); of a
//             divergence per loss
// figures[18]: bytes and flops of product, sweep per side, MU frobenius per side, MU Kullback-Leibler, fill per side, divergence
extern "C" void bp_accounting(int n_users, int n_items, int64_t nnz, int r, const int *n_long, int64_t *counts, double *figures) {
    const int rows[2] = {n_users, n_items};
    int c = 0;
    for (int s = 0; s < 2; ++s) counts[c++] = block_bytes(rows[s], r);
    counts[c++] = gram_download_bytes(r);
    counts[c++] = apply_upload_bytes(r);
    counts[c++] = permutation_bytes(r);
    counts[c++] = SCALAR_BYTES;
    for (int s = 0; s < 2; ++s) counts[c++] = product_launches(n_long[s]);
    counts[c++] = GRAM_LAUNCHES;
    counts[c++] = APPLY_LAUNCHES;
    counts[c++] = FILL_LAUNCHES;
    for (int reuse = 0; reuse < 2; ++reuse)
        for (int s = 0; s < 2; ++s) counts[c++] = sweep_launches(reuse != 0, n_long[s]);
    for (int loss = 0; loss < 2; ++loss)
        for (int reuse = 0; reuse < 2; ++reuse)
            for (int s = 0; s < 2; ++s) counts[c++] = mu_step_launches(loss, reuse != 0, n_long[s]);
    for (int loss = 0; loss < 2; ++loss) counts[c++] = divergence_launches(loss, n_long[0]);
    int f = 0;
    const auto put = [&](CallFigures x) { figures[f++] = x.bytes, figures[f++] = x.flops; };
    put(product_figures((size_t)nnz, r));
    for (int s = 0; s < 2; ++s) put(sweep_figures(rows[s], r));
    for (int s = 0; s < 2; ++s) put(mu_frobenius_figures((size_t)rows[s] * r, r));
    put(mu_kl_figures((size_t)nnz, r));
    for (int s = 0; s < 2; ++s) put(fill_figures((size_t)rows[s] * r));
    put(divergence_figures((size_t)nnz, r));
}
