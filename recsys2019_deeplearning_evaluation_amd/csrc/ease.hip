// ease.hip -- the closed form of EASE_R on MI355X (gfx950): P = G^-1 in place in HBM, the weights W = P / (-diag P) and their
// column-wise top-K  [EASE_R/EASE_R_Recommender.py:40-82; DESIGN.md section 13].
//
// The inverse is a blocked Gauss-Jordan elimination WITHOUT pivoting, valid for symmetric positive-definite input only (every
// diagonal block met on the way is a Schur complement of an SPD matrix, hence SPD).  One step per block column k of NB cells:
//   ease_diag_kernel    one workgroup: D = A[k,k]^-1 by an unpivoted Gauss-Jordan sweep in float64; its pivots are the squares
//                       of the Cholesky factor's diagonal.  A pivot that is <= 0 or NaN writes the step into the status word
//   ease_panel_kernel   the panels the update overwrites go to the workspace: Ct = A[:,k]^T, R = D A[k,:], ND = -A[:,k] D
//   ease_update_kernel  the hot kernel: A[i,j] -= A[i,k] D A[k,j] = Ct^T R, an n x n x NB read-modify-write GEMM on
//                       v_mfma_f32_32x32x2_f32 (128 x 128 tiles, operands staged in LDS as score_gemm_kernel does)
//   ease_writeback_kernel  block row k <- R, block column k <- ND, the block itself <- D (replacing what the update left there)
// Every dependency is a kernel boundary on the handle's stream; a set status word turns every later kernel into an empty launch.
// Matrices that are not positive definite: ease_pivot.hip inverts them on the same handle (ease_handle.h) with pivoting, in float64.
//
// Edges: the matrix lives in an npad x npad buffer, npad = n rounded up to 128, whose tail carries an identity block.  The padded
// matrix is block diagonal, so the leading n x n cells of its inverse are G^-1 exactly and no kernel forms an address outside the
// buffer: every tile and every panel is whole.
//
// The kernels: ease_kernels.cuh.  The shape, the bytes, the grids of a step, the launch counts and the accounting: ease_plan.h.  Here:
// the launches, the head and tail both inverts share (ease_handle.h) and the C ABI.
#include "common.h"
#include "ease_handle.h"
#include "score.h"
#include "ease_kernels.cuh"

#include <algorithm>
#include <chrono>

using namespace mi355rec;
using namespace mi355rec::ease;

namespace {        // (the handle struct: ease_handle.h)

void clear_and_pad(mi355rec_ease *h) {
    hipStream_t s = h->stream;
    if (h->npad != h->n) {
        MI_HIP(hipMemsetAsync(h->A.ptr, 0, (size_t)h->npad * h->npad * sizeof(float), s));
        hipLaunchKernelGGL(ease_pad_kernel, dim3(1), dim3(TILE), 0, s, h->A.ptr, (int64_t)h->npad, h->n, h->npad);
        MI_HIP(hipGetLastError());
    }
    h->failed_step = -1;
    h->pivot.valid = false;
}

template <int NB>
void enqueue_elimination(mi355rec_ease *h) {
    hipStream_t s = h->stream;
    const int64_t ld = h->npad;
    const size_t lds_panel = panel_lds_bytes(NB);
    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ease_panel_kernel<NB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_panel));
    for (int step = 0; step < h->steps; ++step) {
        const EaseStep p = ease_step(*h, step);
        hipLaunchKernelGGL(ease_diag_kernel<NB>, dim3(p.diag_grid), dim3(1024), 0, s, h->A.ptr, ld, p.k0, step, h->status.ptr, h->D.ptr);
        hipLaunchKernelGGL(ease_panel_kernel<NB>, dim3(p.panel_grid), dim3(256), lds_panel, s, h->A.ptr, ld, p.k0, h->status.ptr, h->D.ptr,
                           h->R.ptr, h->Ct.ptr, h->ND.ptr);
        hipLaunchKernelGGL(ease_update_kernel<NB>, dim3(p.update_tiles, p.update_tiles), dim3(256), 0, s, h->A.ptr, ld, h->status.ptr, h->R.ptr, h->Ct.ptr);
        hipLaunchKernelGGL(ease_writeback_kernel<NB>, dim3(p.writeback_grid), dim3(256), 0, s, h->A.ptr, ld, p.k0, h->status.ptr, h->D.ptr,
                           h->R.ptr, h->ND.ptr);
    }
    MI_HIP(hipGetLastError());
    h->launches += ease_launches(*h);
}

// W in place of P, once; true when this call did it
bool ensure_weights(mi355rec_ease *h) {
    MI_REQUIRE(h->state == ST_INVERTED || h->state == ST_WEIGHTS, "the weights need a successful mi355rec_ease_invert first");
    if (h->state == ST_WEIGHTS) return false;
    hipStream_t s = h->stream;
    hipLaunchKernelGGL(ease_get_diagonal_kernel, dim3(div_up(h->n, 256)), dim3(256), 0, s, h->A.ptr, (int64_t)h->npad, h->n, h->diag.ptr);
    hipLaunchKernelGGL(ease_weights_kernel, dim3(std::min(div_up(h->n, 256), 64), std::min(h->n, 65535)), dim3(256), 0, s, h->A.ptr, (int64_t)h->npad, h->n,
                       h->diag.ptr);
    MI_HIP(hipGetLastError());
    h->launches += WEIGHTS_LAUNCHES;
    h->state = ST_WEIGHTS;
    return true;
}

// ensure_weights between the marks of `call_timer`; once the stream has drained the caller notes the time where this returned true
bool timed_ensure_weights(mi355rec_ease *h) {
    h->call_timer.start(h->stream);
    const bool scaled = ensure_weights(h);
    h->call_timer.stop(h->stream);
    return scaled;
}

}  // namespace

void mi355rec::require_invertible(const mi355rec_ease *h, const char *caller) {
    MI_REQUIRE(h->state == ST_MATRIX, "%s needs a matrix that has been set and not yet inverted", caller);
    ensure_device();
}

void mi355rec::begin_invert(mi355rec_ease *h) {
    hipStream_t s = h->stream;
    h->state = ST_FAILED;                                   // until the status word says otherwise
    MI_HIP(hipMemsetAsync(h->status.ptr, 0xFF, sizeof(int), s));      // -1: no step has failed
    h->launches = 0;
    h->timer.start(s);
}

void mi355rec::stop_elimination(mi355rec_ease *h) {
    h->timer.stop(h->stream);
    MI_HIP(hipMemcpyAsync(&h->failed_step, h->status.ptr, sizeof(int), hipMemcpyDeviceToHost, h->stream));
}

int mi355rec::await_elimination(mi355rec_ease *h) {
    MI_HIP(hipStreamSynchronize(h->stream));
    h->invert_ms = h->timer.elapsed_ms();
    return h->failed_step;
}

void mi355rec::finish_invert(mi355rec_ease *h, const EaseAccounting &work, const char *refusal) {
    h->stats = mi355rec_stats{};
    h->stats.kernel_ms = h->stats.call_ms = h->invert_ms;
    h->stats.n_launches = h->launches;
    h->stats.n_timed = 1;
    h->stats.n_units = work.units;
    h->stats.algorithmic_flops = work.flops;
    h->stats.algorithmic_bytes = work.bytes;
    if (h->failed_step >= 0) fail(MI355REC_E_NUMERIC, refusal, h->failed_step, h->steps, h->block);
    h->state = ST_INVERTED;
}

extern "C" int mi355rec_ease_create(mi355rec_ease_t *out, int32_t n_items) {
    return guarded([&] {
        MI_REQUIRE(out, "NULL argument");
        MI_REQUIRE(n_items > 0, "empty matrix (%d items)", n_items);
        *out = nullptr;
        const int block = read_ease_knobs().block;
        MI_REQUIRE(ease_block_valid(block), EASE_BLOCK_MESSAGE, block);
        const std::optional<EaseShape> shape = ease_shape(n_items, block);
        MI_REQUIRE(shape, "%d items: too many", n_items);
        ensure_device();
        size_t free_b = 0, total_b = 0;
        MI_HIP(hipMemGetInfo(&free_b, &total_b));
        const size_t need = ease_bytes(*shape);
        MI_REQUIRE(ease_fit(need, free_b) == EaseFit::FITS, "the matrix of %d items and its workspace (%.2f GB) do not fit the device's free memory (%.2f GB)",
                   n_items, (need + EASE_RESERVE) / 1e9, free_b / 1e9);
        auto h = open_handle<mi355rec_ease>(2);
        static_cast<EaseShape &>(*h) = *shape;
        const size_t npad = (size_t)h->npad;
        h->A.alloc(npad * npad);
        h->D.alloc((size_t)block * block);
        h->R.alloc((size_t)block * npad);
        h->Ct.alloc((size_t)block * npad);
        h->ND.alloc((size_t)block * npad);
        h->diag.alloc((size_t)n_items);
        h->status.alloc(1);
        *out = h.release();
    });
}

extern "C" int mi355rec_ease_set_gram_from_sim(mi355rec_ease_t h, mi355rec_sim_t sim) {
    return guarded([&] {
        MI_REQUIRE(h && sim, "NULL argument");
        int n_cols = 0, topK = 0;
        sim_shape(sim, &n_cols, &topK);
        MI_REQUIRE(topK == 0, "the similarity handle must be a dense one (topK == 0), its topK is %d", topK);
        MI_REQUIRE(n_cols == h->n, "the similarity handle has %d columns, the matrix %d items", n_cols, h->n);
        ensure_device();
        ReleaseScope scope(h->stream);
        hipStream_t s = h->stream;
        const auto t0 = std::chrono::steady_clock::now();
        h->state = ST_EMPTY;
        clear_and_pad(h);
        MI_HIP(hipStreamSynchronize(s));
        // the Gram matrix is symmetric: column c of the build, contiguous, is row c of the matrix (pitch npad)
        const int rc = mi355rec_sim_compute_dense_device(sim, 0, h->n, h->A.ptr, h->npad);
        if (rc != MI355REC_OK) throw Error(rc, mi355rec_last_error());
        h->gram_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        h->state = ST_MATRIX;
    });
}

extern "C" int mi355rec_ease_set_matrix(mi355rec_ease_t h, const float *G, int64_t ld) {
    return guarded([&] {
        MI_REQUIRE(h && G, "NULL argument");
        MI_REQUIRE(ld >= h->n, "ld (%lld) < number of items (%d)", (long long)ld, h->n);
        ensure_device();
        hipStream_t s = h->stream;
        h->state = ST_EMPTY;
        clear_and_pad(h);
        MI_HIP(hipMemcpy2DAsync(h->A.ptr, (size_t)h->npad * sizeof(float), G, (size_t)ld * sizeof(float), (size_t)h->n * sizeof(float), (size_t)h->n,
                                hipMemcpyHostToDevice, s));
        MI_HIP(hipStreamSynchronize(s));
        h->state = ST_MATRIX;
    });
}

extern "C" int mi355rec_ease_get_matrix(mi355rec_ease_t h, float *G, int64_t ld) {
    return guarded([&] {
        MI_REQUIRE(h && G, "NULL argument");
        MI_REQUIRE(ld >= h->n, "ld (%lld) < number of items (%d)", (long long)ld, h->n);
        MI_REQUIRE(h->state != ST_EMPTY, "no matrix has been set");
        ensure_device();
        MI_HIP(hipMemcpy2DAsync(G, (size_t)ld * sizeof(float), h->A.ptr, (size_t)h->npad * sizeof(float), (size_t)h->n * sizeof(float), (size_t)h->n,
                                hipMemcpyDeviceToHost, h->stream));
        MI_HIP(hipStreamSynchronize(h->stream));
    });
}

extern "C" int mi355rec_ease_set_diagonal(mi355rec_ease_t h, const float *diag) {
    return guarded([&] {
        MI_REQUIRE(h && diag, "NULL argument");
        MI_REQUIRE(h->state == ST_MATRIX, "set_diagonal needs a matrix that has been set and not yet inverted");
        ensure_device();
        hipStream_t s = h->stream;
        MI_HIP(hipMemcpyAsync(h->diag.ptr, diag, (size_t)h->n * sizeof(float), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(ease_set_diagonal_kernel, dim3(div_up(h->n, 256)), dim3(256), 0, s, h->A.ptr, (int64_t)h->npad, h->n, h->diag.ptr);
        MI_HIP(hipGetLastError());
        MI_HIP(hipStreamSynchronize(s));
    });
}

extern "C" int mi355rec_ease_invert(mi355rec_ease_t h) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL argument");
        require_invertible(h, "invert");
        begin_invert(h);
        if (h->block == 64) enqueue_elimination<64>(h);
        else enqueue_elimination<128>(h);
        stop_elimination(h);
        await_elimination(h);
        finish_invert(h, invert_accounting(*h, sizeof(float)),
                      "the matrix is not positive definite: a pivot <= 0 (or NaN) in elimination step %d of %d (block size %d)");
    });
}

extern "C" int mi355rec_ease_get_dense(mi355rec_ease_t h, float *W, int64_t ld) {
    return guarded([&] {
        MI_REQUIRE(h && W, "NULL argument");
        MI_REQUIRE(ld >= h->n, "ld (%lld) < number of items (%d)", (long long)ld, h->n);
        ensure_device();
        hipStream_t s = h->stream;
        const bool scaled = timed_ensure_weights(h);
        MI_HIP(hipMemcpy2DAsync(W, (size_t)ld * sizeof(float), h->A.ptr, (size_t)h->npad * sizeof(float), (size_t)h->n * sizeof(float), (size_t)h->n,
                                hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
        if (scaled) h->topk_ms = h->call_timer.elapsed_ms();
    });
}

// what the dense scorer (densescore.hip) copies its weights from, device to device: the cells mi355rec_ease_get_dense downloads
void mi355rec::ease_weights_device(mi355rec_ease *h, const float **W, int64_t *ld, int *n) {
    const bool scaled = timed_ensure_weights(h);
    MI_HIP(hipStreamSynchronize(h->stream));
    if (scaled) h->topk_ms = h->call_timer.elapsed_ms();
    *W = h->A.ptr;
    *ld = h->npad;
    *n = h->n;
}

extern "C" int mi355rec_ease_get_topk(mi355rec_ease_t h, int32_t topK, int32_t *idx, float *val) {
    return guarded([&] {
        MI_REQUIRE(h && idx && val, "NULL argument");
        MI_REQUIRE(topK >= 1, "topK must be at least 1, got %d", topK);
        MI_REQUIRE(h->state == ST_INVERTED || h->state == ST_WEIGHTS, "the weights need a successful mi355rec_ease_invert first");
        if (topK > MAX_TOPK || !score_row_fits_lds(h->n, topK))
            fail(MI355REC_E_UNSUPPORTED, "top-%d of columns of %d cells is beyond the in-LDS selection (at most %d of about 30 000 cells)", topK, h->n,
                 MAX_TOPK);
        ensure_device();
        ReleaseScope scope(h->stream);
        hipStream_t s = h->stream;
        const size_t cells = (size_t)h->n * topK;
        if (h->out_idx.count < cells) {
            h->out_idx.alloc(cells);
            h->out_val.alloc(cells);
        }
        h->call_timer.start(s);
        ensure_weights(h);
        const int n_pad = (h->n + 3) & ~3;
        const size_t lds = (size_t)n_pad * 4 + (size_t)AUX_WORDS * 4;
        auto k = ease_topk_kernel<1024>;
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, dim3(h->n), dim3(1024), lds, s, h->A.ptr, (int64_t)h->npad, h->n, n_pad, topK, h->out_idx.ptr, h->out_val.ptr);
        MI_HIP(hipGetLastError());
        h->launches += TOPK_LAUNCHES;
        h->call_timer.stop(s);
        h->out_idx.download(idx, cells, s);
        h->out_val.download(val, cells, s);
        MI_HIP(hipStreamSynchronize(s));
        h->topk_ms = h->call_timer.elapsed_ms();
    });
}

extern "C" int mi355rec_ease_fit_info(mi355rec_ease_t h, int32_t *block, int32_t *steps, int32_t *failed_step, double *invert_ms, double *gram_ms,
                                      double *topk_ms, int64_t *launches) {
    return guarded([&] {
        MI_REQUIRE(h && block && steps && failed_step && invert_ms && gram_ms && topk_ms && launches, "NULL argument");
        *block = h->block;
        *steps = h->steps;
        *failed_step = h->failed_step;
        *invert_ms = h->invert_ms;
        *gram_ms = h->gram_ms;
        *topk_ms = h->topk_ms;
        *launches = h->launches;
    });
}

extern "C" int mi355rec_ease_get_stats(mi355rec_ease_t h, mi355rec_stats *stats) { return handle_get_stats(h, stats); }

extern "C" void mi355rec_ease_destroy(mi355rec_ease_t h) { handle_destroy(h); }
