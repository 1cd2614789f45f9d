// blocks.hip -- the translation unit of blocks.h: the product, Gram and iota kernels (blocks_kernels.cuh) with their launchers, and the
// bodies of BlockPair, the base of the PureSVD handle (svd.hip) and the NMF handle (nmf.hip)  [DESIGN.md sections 11 and 12].
// Every grid, buffer size and byte count comes from blocks_plan.h.
#include "blocks.h"
#include "blocks_kernels.cuh"

using namespace mi355rec::blocks;

namespace mi355rec {

namespace {

// the product gathers block rows by the indices of a layout: what check_layout found, in the words of the refusal
void require_layout(int n, int n_other, const int *ptr, const int *idx) {
    const LayoutFinding f = check_layout(n, n_other, ptr, idx);
    MI_REQUIRE(f.kind != LayoutFinding::START_NOT_ZERO, "row pointers do not start at 0");
    MI_REQUIRE(f.kind != LayoutFinding::POINTERS_DECREASE, "row pointers decrease at %d", f.at);
    MI_REQUIRE(f.kind != LayoutFinding::INDEX_OUTSIDE, "index %d outside [0, %d)", f.index, n_other);
}

void iota_enqueue(int *out, int n, hipStream_t s) {
    hipLaunchKernelGGL(svd_iota_kernel, dim3(ceil_div(n, NT)), dim3(NT), 0, s, out, n);
    MI_HIP(hipGetLastError());
}

}  // namespace

size_t Side::build(int n, const int *row_ptr, const int *row_idx, const float *row_val, bool ones, hipStream_t s) {
    const PiecePlan p = piece_plan(row_ptr, n);
    n_rows = n;
    n_pieces = p.n_pieces();
    n_long = p.n_long();
    n_slots = p.n_slots;
    const size_t nnz = (size_t)row_ptr[n];
    idx.alloc(std::max<size_t>(nnz, 1));
    if (nnz) MI_HIP(hipMemcpyAsync(idx.ptr, row_idx, nnz * sizeof(int), hipMemcpyHostToDevice, s));
    if (!ones) {
        val.alloc(std::max<size_t>(nnz, 1));
        if (nnz) MI_HIP(hipMemcpyAsync(val.ptr, row_val, nnz * sizeof(float), hipMemcpyHostToDevice, s));
    }
    p_row.upload(p.row.data(), p.row.size(), s);
    p_begin.upload(p.begin.data(), p.begin.size(), s);
    p_end.upload(p.end.data(), p.end.size(), s);
    p_slot.upload(p.slot.data(), p.slot.size(), s);
    if (n_long) {
        l_row.upload(p.long_row.data(), p.long_row.size(), s);
        l_first.upload(p.long_first.data(), p.long_first.size(), s);
        l_count.upload(p.long_count.data(), p.long_count.size(), s);
    }
    MI_HIP(hipStreamSynchronize(s));              // the plan's vectors go out of scope
    return side_upload_bytes(nnz, ones, p.row.size(), p.long_row.size());
}

void spmm_enqueue(const Side &sd, const float *val, const float *X, int r, float *Y, float *partial, hipStream_t s) {
    const int lp_shift = group_shift(r), grid = product_grid(sd.n_pieces, r);
    if (!val)
        hipLaunchKernelGGL(svd_spmm_kernel<true>, dim3(grid), dim3(SPMM_THREADS), 0, s, sd.p_row.ptr, sd.p_begin.ptr, sd.p_end.ptr,
                           sd.p_slot.ptr, sd.n_pieces, sd.idx.ptr, (const float *)nullptr, X, r, lp_shift, Y, partial);
    else
        hipLaunchKernelGGL(svd_spmm_kernel<false>, dim3(grid), dim3(SPMM_THREADS), 0, s, sd.p_row.ptr, sd.p_begin.ptr, sd.p_end.ptr,
                           sd.p_slot.ptr, sd.n_pieces, sd.idx.ptr, val, X, r, lp_shift, Y, partial);
    MI_HIP(hipGetLastError());
    if (sd.n_long) {
        hipLaunchKernelGGL(svd_long_rows_kernel, dim3(sd.n_long), dim3(256), 0, s, sd.l_row.ptr, sd.l_first.ptr, sd.l_count.ptr, partial, r, Y);
        MI_HIP(hipGetLastError());
    }
}

void gram_enqueue(const float *X, int n, int r, const GramPlan &plan, double *part, double *G, hipStream_t s) {
    const int nt = gram_tiles(r);
    hipLaunchKernelGGL(svd_gram_kernel, dim3(nt, nt, plan.slabs), dim3(NT), 0, s, X, n, r, plan.rows, part);
    MI_HIP(hipGetLastError());
    hipLaunchKernelGGL(svd_gram_reduce_kernel, dim3(gram_reduce_grid(r)), dim3(NT), 0, s, part, plan.slabs, r, G);
    MI_HIP(hipGetLastError());
}

void require_side(int side, const char *zero, const char *one) { MI_REQUIRE(side == 0 || side == 1, "side %d: 0 (%s) or 1 (%s)", side, zero, one); }

void BlockPair::check_create(const void *out, const PairArgs &a, const char *width_noun) {
    MI_REQUIRE(out && a.row_ptr && a.col_ptr, "NULL argument");
    MI_REQUIRE(a.n_users > 0 && a.n_items > 0, "empty URM (%d x %d)", a.n_users, a.n_items);
    MI_REQUIRE(width_in_range(a.width), "%s = %d outside [%d, %d]", width_noun, a.width, MIN_WIDTH, MAX_WIDTH);
    MI_REQUIRE(a.row_ptr[a.n_users] == a.col_ptr[a.n_items], "the two layouts hold %d and %d cells", a.row_ptr[a.n_users], a.col_ptr[a.n_items]);
    MI_REQUIRE(a.nnz() == 0 || (a.row_idx && a.col_idx && a.row_val && a.col_val), "NULL argument");
    MI_REQUIRE(rows_in_range(a.n_users, a.n_items), "more than 8 M rows on a side");
    require_layout(a.n_users, a.n_items, a.row_ptr, a.row_idx);
    require_layout(a.n_items, a.n_users, a.col_ptr, a.col_idx);
}

PairSizes BlockPair::create_common(const PairArgs &a, bool all_ones) {
    n_users = a.n_users;
    n_items = a.n_items;
    width = a.width;
    nnz = a.nnz();
    ones = all_ones ? 1 : 0;
    hipStream_t s = stream;
    create_bytes += (int64_t)sides[0].build(n_users, a.row_ptr, a.row_idx, a.row_val, all_ones, s);
    create_bytes += (int64_t)sides[1].build(n_items, a.col_ptr, a.col_idx, a.col_val, all_ones, s);
    const PairSizes z = pair_sizes(n_users, n_items, width, sides[0].n_slots, sides[1].n_slots, gram_plan);
    block[0].alloc_zero(z.cap, s);
    block[1].alloc_zero(z.cap, s);
    partial.alloc(z.partial_rows * width);
    gram_part.alloc(z.gram_part_cells);
    iota.alloc(z.n_max);
    iota_enqueue(iota.ptr, z.n_max, s);
    return z;
}

void BlockPair::set_block(int side, const float *X) {
    const int64_t bytes = block_bytes(rows_of(side), width);
    MI_HIP(hipMemcpyAsync(block[side].ptr, X, (size_t)bytes, hipMemcpyHostToDevice, stream));
    MI_HIP(hipStreamSynchronize(stream));
    h2d_bytes += bytes;
    ++calls;
}

void BlockPair::get_block(int side, float *X) {
    const int64_t bytes = block_bytes(rows_of(side), width);
    MI_HIP(hipMemcpyAsync(X, block[side].ptr, (size_t)bytes, hipMemcpyDeviceToHost, stream));
    MI_HIP(hipStreamSynchronize(stream));
    d2h_bytes += bytes;
    ++calls;
}

void BlockPair::traffic(int64_t *launches_, int64_t *calls_, int64_t *create_bytes_, int64_t *h2d_bytes_, int64_t *d2h_bytes_, int32_t *all_ones) const {
    *launches_ = launches;
    *calls_ = calls;
    *create_bytes_ = create_bytes;
    *h2d_bytes_ = h2d_bytes;
    *d2h_bytes_ = d2h_bytes;
    *all_ones = ones;
}

}  // namespace mi355rec
