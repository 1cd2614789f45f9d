// svd.hip -- the device half of PureSVD's randomized SVD on MI355X (gfx950)  [DESIGN.md section 11].
//
// The reference (MatrixFactorization/PureSVDRecommender.py:34-47) calls sklearn's randomized_svd: sixteen products of the URM or
// its transpose with a tall, thin dense block, a normalisation of the block after each, and a small dense SVD.  The handle keeps
// the URM in both layouts and one block per side (users x r, items x r) resident -- the BlockPair of blocks.h, which the NMF handle
// (nmf.hip) is built on, too; the loop is driven from Python through the step-wise entry points below, because the r x r
// factorisations (Cholesky, eigh) belong to LAPACK on the host.
//
//   product             blocks.hip's svd_spmm_kernel (+ svd_long_rows_kernel): bitwise repeatable, all-ones URMs skip the value stream
//   gram                blocks.hip's svd_gram_kernel + svd_gram_reduce_kernel: G = X^T X in float64
//   block * matrix      X <- X T is score.hip's f32 MFMA GEMM (gemm_rows_enqueue) with the identity as its row gather.
// This file holds the handle, its launches and its C ABI; there is no kernel in it.
#include "blocks.h"
#include "score.h"

using namespace mi355rec;
using namespace mi355rec::blocks;

struct mi355rec_svd : BlockPair {
    DeviceBuffer<float> tmp, T;
    DeviceBuffer<double> G;
    double phase_ms[3] = {0, 0, 0};                   // products, Gram, apply

    ~mi355rec_svd() { shutdown(); }
};

namespace {

void require_block_side(int side) { require_side(side, "users x r", "items x r"); }

}  // namespace

extern "C" int mi355rec_svd_create(mi355rec_svd_t *out, int32_t n_users, int32_t n_items, int32_t r, const int32_t *row_ptr,
                                   const int32_t *row_idx, const float *row_val, const int32_t *col_ptr, const int32_t *col_idx,
                                   const float *col_val) {
    return guarded([&] {
        const PairArgs a{n_users, n_items, r, row_ptr, row_idx, row_val, col_ptr, col_idx, col_val};
        BlockPair::check_create(out, a, "block width r");
        *out = nullptr;
        auto h = open_handle<mi355rec_svd>(1);
        ReleaseScope scope(h->stream);
        const PairSizes z = h->create_common(a, all_ones(row_val, a.nnz()));
        h->tmp.alloc(z.cap);
        h->G.alloc((size_t)r * r);
        h->T.alloc((size_t)r * r);
        MI_HIP(hipStreamSynchronize(h->stream));
        *out = h.release();
    });
}

extern "C" int mi355rec_svd_set_block(mi355rec_svd_t h, int32_t side, const float *X) {
    return guarded([&] {
        MI_REQUIRE(h && X, "NULL argument");
        require_block_side(side);
        ensure_device();
        h->set_block(side, X);
    });
}

extern "C" int mi355rec_svd_get_block(mi355rec_svd_t h, int32_t side, float *X) {
    return guarded([&] {
        MI_REQUIRE(h && X, "NULL argument");
        require_block_side(side);
        ensure_device();
        h->get_block(side, X);
    });
}

extern "C" int mi355rec_svd_product(mi355rec_svd_t h, int32_t dst_side) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL argument");
        require_side(dst_side, "users = URM . items", "items = URM^T . users");
        ensure_device();
        hipStream_t s = h->stream;
        h->timer.start(s);
        h->product(dst_side, h->values(dst_side), h->block[dst_side].ptr);
        h->timer.stop(s);
        MI_HIP(hipStreamSynchronize(s));
        const double ms = h->timer.elapsed_ms();
        const CallFigures f = product_figures(h->nnz, h->width);
        h->phase_ms[0] += ms;
        h->launches += product_launches(h->sides[dst_side].n_long);
        ++h->calls;
        h->stats = mi355rec_stats{};
        h->stats.call_ms = h->stats.kernel_ms = ms;
        h->stats.n_launches = h->stats.n_timed = 1;
        h->stats.n_units = (int64_t)h->nnz;
        h->stats.algorithmic_bytes = f.bytes;
        h->stats.algorithmic_flops = f.flops;
    });
}

extern "C" int mi355rec_svd_gram(mi355rec_svd_t h, int32_t side, double *G) {
    return guarded([&] {
        MI_REQUIRE(h && G, "NULL argument");
        require_block_side(side);
        ensure_device();
        hipStream_t s = h->stream;
        const int r = h->width;
        h->timer.start(s);
        h->gram(side, h->G.ptr);
        h->timer.stop(s);
        h->G.download(G, (size_t)r * r, s);
        MI_HIP(hipStreamSynchronize(s));
        h->phase_ms[1] += h->timer.elapsed_ms();
        h->launches += GRAM_LAUNCHES;
        h->d2h_bytes += gram_download_bytes(r);
        ++h->calls;
    });
}

extern "C" int mi355rec_svd_apply(mi355rec_svd_t h, int32_t side, const float *T) {
    return guarded([&] {
        MI_REQUIRE(h && T, "NULL argument");
        require_block_side(side);
        ensure_device();
        hipStream_t s = h->stream;
        const int r = h->width, n = h->rows_of(side);
        std::vector<float> Tt((size_t)r * r);          // the GEMM multiplies by the rows of its second operand
        for (int i = 0; i < r; ++i)
            for (int j = 0; j < r; ++j) Tt[(size_t)j * r + i] = T[(size_t)i * r + j];
        MI_HIP(hipMemcpyAsync(h->T.ptr, Tt.data(), Tt.size() * sizeof(float), hipMemcpyHostToDevice, s));
        h->timer.start(s);
        gemm_rows_enqueue(h->block[side].ptr, h->iota.ptr, n, r, h->T.ptr, r, h->tmp.ptr, s);
        h->timer.stop(s);
        MI_HIP(hipStreamSynchronize(s));
        h->block[side].swap(h->tmp);
        h->phase_ms[2] += h->timer.elapsed_ms();
        h->launches += APPLY_LAUNCHES;
        h->h2d_bytes += apply_upload_bytes(r);
        ++h->calls;
    });
}

extern "C" int mi355rec_svd_get_stats(mi355rec_svd_t h, mi355rec_stats *stats) { return handle_get_stats(h, stats); }

extern "C" int mi355rec_svd_fit_info(mi355rec_svd_t h, double *product_ms, double *gram_ms, double *apply_ms, int64_t *launches,
                                     int64_t *calls, int64_t *create_bytes, int64_t *h2d_bytes, int64_t *d2h_bytes, int32_t *all_ones) {
    return guarded([&] {
        MI_REQUIRE(h && product_ms && gram_ms && apply_ms && launches && calls && create_bytes && h2d_bytes && d2h_bytes && all_ones,
                   "NULL argument");
        *product_ms = h->phase_ms[0];
        *gram_ms = h->phase_ms[1];
        *apply_ms = h->phase_ms[2];
        h->traffic(launches, calls, create_bytes, h2d_bytes, d2h_bytes, all_ones);
    });
}

extern "C" void mi355rec_svd_destroy(mi355rec_svd_t h) { handle_destroy(h); }
