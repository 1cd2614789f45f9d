// ease_pivot.hip -- the inverse of EASE_R for matrices that are NOT positive definite (explicit ratings: counts, not sums of squares,
// on the diagonal make the matrix symmetric indefinite) on MI355X (gfx950): blocked Gauss-Jordan elimination with partial (row)
// pivoting, float64 throughout  [DESIGN.md section 13].  ease.hip keeps the unpivoted float32 route; this unit shares its handle
// (ease_handle.h) and leaves the result where that route leaves it -- the handle's float32 matrix, state ST_INVERTED -- so weights,
// top-K and the dense scorer's hand-off follow unchanged.
//
// The working matrix is a float64 npad x npad copy of the handle's matrix (same identity tail).  One step per block column k of NB cells:
//   pivot search   LU elimination with partial pivoting on a scratch copy of the panel A[k0 .. n, k0 .. k0 + NB]: ease_pivot_load_kernel
//                  copies it; per column ease_pivot_pick_kernel (one workgroup) reduces the per-chunk candidates to the pivot row
//                  -- the largest |value|, ties to the lowest row, a NaN counts as the largest -- and swaps it up inside the scratch,
//                  ease_pivot_elim_kernel eliminates the column below it and leaves the next column's candidates.  Rows >= n (the
//                  identity tail) are never candidates; a pivot that is 0 or NaN writes the step into the status word
//   ease_pivot_swap_kernel   the NB swaps, in order, on whole rows of the working matrix (converted block columns included)
//   ease_diag64_kernel       D = A[k,k]^-1 by the unpivoted sweep of ease_diag_kernel on doubles (the swaps made the block factorable)
//   ease_transpose64_kernel  Ct = A[:,k]^T
//   ease_gemm64_kernel       R = D A[k,:], ND = -A[:,k] D, and the hot one: A -= Ct^T R, an npad x npad x NB read-modify-write GEMM on
//                            v_mfma_f64_16x16x4_f64 (128 x 128 tiles, operands staged in LDS as ease_update_kernel does)
//   ease_writeback64_kernel  block row k <- R, block column k <- ND, the block itself <- D
// After the last step the row swaps are undone on the COLUMNS, last swap first: the swap list is composed into one permutation on the
// host and ease_gather32_kernel gathers the float32 result from the permuted column while it converts.
// Every dependency is a kernel boundary on the handle's stream; a set status word turns every later kernel into an empty launch; no
// atomics, fixed reduction orders: two runs give the same bits.
//
// The kernels: ease_pivot_kernels.cuh.  The bytes of the workspace and whether they fit, the grids and launches of a step, the
// permutation and the accounting: ease_plan.h.  Here: the workspace, the launches and the C ABI.
#include "common.h"
#include "ease_handle.h"
#include "ease_pivot_kernels.cuh"

#include <algorithm>

using namespace mi355rec;
using namespace mi355rec::ease;

namespace {

// Is there room for the workspace?  Decided before anything is allocated, from the device's free memory (asked again after the cache
// of released blocks has gone back to the driver) and from MI355REC_EASE_PIVOT_MAX_BYTES (read at every first allocation).
void require_room(const mi355rec_ease *h, size_t need) {
    const std::optional<unsigned long long> cap = read_ease_knobs().pivot_max_bytes;
    size_t free_b = 0, total_b = 0;
    MI_HIP(hipMemGetInfo(&free_b, &total_b));
    EaseFit fit = pivot_fit(need, free_b, cap);
    if (fit == EaseFit::NO_ROOM) {
        uint64_t freed = 0;
        (void)mi355rec_device_trim(&freed);
        MI_HIP(hipMemGetInfo(&free_b, &total_b));
        fit = pivot_fit(need, free_b, cap);
    }
    if (fit == EaseFit::OVER_CAP)
        fail(MI355REC_E_UNSUPPORTED, "no device memory for the float64 working matrix of the pivoted inverse (%.2f GB for %d items): "
             "MI355REC_EASE_PIVOT_MAX_BYTES allows %llu bytes", need / 1e9, h->n, *cap);
    if (fit == EaseFit::NO_ROOM)
        fail(MI355REC_E_UNSUPPORTED, "no device memory for the float64 working matrix of the pivoted inverse (%.2f GB for %d items): %.2f GB are free",
             need / 1e9, h->n, free_b / 1e9);
}

// The workspace, once per handle.  No memory is not an abort: MI355REC_E_UNSUPPORTED with the handle's matrix untouched (require_room).
// A hipMalloc that fails all the same is turned into the same code, and the error it leaves in the runtime is taken out, so that the
// next launch check of the handle does not report it.
void ensure_work(mi355rec_ease *h) {
    EasePivotWork &w = h->pivot;
    while ((int)w.events.size() < 4 * h->steps) {           // (a failure here is an ordinary MI355REC_E_HIP)
        hipEvent_t e;
        MI_HIP(hipEventCreate(&e));
        w.events.push_back(e);
    }
    if (w.A.ptr) return;
    const size_t npad = (size_t)h->npad, block = (size_t)h->block, need = pivot_bytes(*h);
    require_room(h, need);
    try {
        w.A.alloc(npad * npad);
        w.panel.alloc(npad * block);
        w.D.alloc(block * block);
        w.Dt.alloc(block * block);
        w.R.alloc(block * npad);
        w.Ct.alloc(block * npad);
        w.ND.alloc(block * npad);
        w.part_val.alloc(npad / CHUNK);
        w.part_pos.alloc(npad / CHUNK);
        w.piv.alloc(npad);
        w.inv_perm.alloc(npad);
        w.info.alloc(2);
    } catch (const Error &e) {
        const std::string why = e.what();
        (void)hipGetLastError();
        ReleaseScope scope(h->stream);
        for (DeviceBuffer<double> *b : {&w.A, &w.panel, &w.D, &w.Dt, &w.R, &w.Ct, &w.ND, &w.part_val, &w.info}) b->release();
        for (DeviceBuffer<int> *b : {&w.part_pos, &w.piv, &w.inv_perm}) b->release();
        fail(MI355REC_E_UNSUPPORTED, "no device memory for the float64 working matrix of the pivoted inverse (%.2f GB for %d items): %s", need / 1e9, h->n,
             why.c_str());
    }
}

// the pivot search of one step on the scratch panel, then its swaps on whole rows of the working matrix
template <int NB>
void enqueue_pivot_search(mi355rec_ease *h, int step, const PivotStep &p) {
    EasePivotWork &w = h->pivot;
    hipStream_t s = h->stream;
    const int64_t ld = h->npad;
    const int n = h->n;
    int *status = h->status.ptr;
    hipLaunchKernelGGL(ease_pivot_load_kernel<NB>, dim3(p.load_grid), dim3(256), 0, s, w.A.ptr, ld, p.k0, n, status, w.panel.ptr, w.part_val.ptr,
                       w.part_pos.ptr);
    for (int j = 0; j < p.cols; ++j) {
        hipLaunchKernelGGL(ease_pivot_pick_kernel<NB>, dim3(1), dim3(256), 0, s, w.panel.ptr, p.k0, j, n, step, status, w.part_val.ptr, w.part_pos.ptr,
                           w.piv.ptr, w.info.ptr);
        if (const int grid = pivot_elim_grid(*h, p.k0, j))
            hipLaunchKernelGGL(ease_pivot_elim_kernel<NB>, dim3(grid), dim3(256), 0, s, w.panel.ptr, p.k0, j, n, status, w.part_val.ptr, w.part_pos.ptr);
    }
    hipLaunchKernelGGL(ease_pivot_swap_kernel, dim3(p.swap_grid), dim3(SWAP_W), 0, s, w.A.ptr, ld, p.k0, p.cols, w.piv.ptr, status);
}

template <int NB>
void enqueue_pivoted_elimination(mi355rec_ease *h) {
    EasePivotWork &w = h->pivot;
    hipStream_t s = h->stream;
    const int64_t ld = h->npad;
    int *status = h->status.ptr;
    for (int step = 0; step < h->steps; ++step) {
        const PivotStep p = pivot_step(*h, step);
        const int k0 = p.k0;
        MI_HIP(hipEventRecord(w.events[4 * step], s));
        if (p.cols > 0) enqueue_pivot_search<NB>(h, step, p);
        MI_HIP(hipEventRecord(w.events[4 * step + 1], s));
        hipLaunchKernelGGL(ease_diag64_kernel<NB>, dim3(1), dim3(1024), 0, s, w.A.ptr, ld, k0, step, status, w.D.ptr, w.Dt.ptr);
        hipLaunchKernelGGL(ease_transpose64_kernel<NB>, dim3(p.transpose_grid), dim3(256), 0, s, w.A.ptr, ld, k0, status, w.Ct.ptr);
        // R = D A[k,:]: X[m][c] = sum_q Dt[q][m] A[k0 + q][c];  ND = -A[:,k] D: X[r][m] = sum_q Ct[q][r] D[q][m]
        static_assert(SMALL_T == 32 * 2 && EASE_TILE == 32 * 4, "the plan's grids are for the tiles of ease_gemm64_kernel<2, .> and <4, 2>");
        hipLaunchKernelGGL((ease_gemm64_kernel<2, 0>), dim3(p.panel_grid_long, p.panel_grid_short), dim3(256), 0, s, w.R.ptr, ld, w.Dt.ptr, (int64_t)NB,
                           w.A.ptr + (int64_t)k0 * ld, ld, NB, status);
        hipLaunchKernelGGL((ease_gemm64_kernel<2, 1>), dim3(p.panel_grid_short, p.panel_grid_long), dim3(256), 0, s, w.ND.ptr, (int64_t)NB, w.Ct.ptr, ld,
                           w.D.ptr, (int64_t)NB, NB, status);
        MI_HIP(hipEventRecord(w.events[4 * step + 2], s));
        hipLaunchKernelGGL((ease_gemm64_kernel<4, 2>), dim3(p.update_tiles, p.update_tiles), dim3(256), 0, s, w.A.ptr, ld, w.Ct.ptr, ld, w.R.ptr, ld, NB, status);
        MI_HIP(hipEventRecord(w.events[4 * step + 3], s));
        hipLaunchKernelGGL(ease_writeback64_kernel<NB>, dim3(p.writeback_grid), dim3(256), 0, s, w.A.ptr, ld, k0, status, w.D.ptr, w.R.ptr, w.ND.ptr);
        h->launches += p.launches;
    }
    MI_HIP(hipGetLastError());
}

// the two figures the pick kernel keeps and the device time of the steps' two timed spans: what mi355rec_ease_pivot_info reports
void note_pivot_figures(mi355rec_ease *h, const double info[2]) {
    EasePivotWork &w = h->pivot;
    w.pivot_ms = w.update_ms = 0;
    for (int step = 0; step < h->steps; ++step) {
        float a = 0.f, b = 0.f;
        MI_HIP(hipEventElapsedTime(&a, w.events[4 * step], w.events[4 * step + 1]));
        MI_HIP(hipEventElapsedTime(&b, w.events[4 * step + 2], w.events[4 * step + 3]));
        w.pivot_ms += a;
        w.update_ms += b;
    }
    w.min_pivot = info[0];
    w.moved = (int)info[1];
    w.valid = true;
}

// the handle's float32 matrix <- the working matrix, its columns permuted back; timed by `call_timer` and added to invert_ms
void gather_result(mi355rec_ease *h, const std::vector<int> &piv) {
    EasePivotWork &w = h->pivot;
    hipStream_t s = h->stream;
    const int npad = h->npad;
    const std::vector<int> inv_perm = inverse_column_permutation(piv.data(), h->n, npad);
    MI_HIP(hipMemcpyAsync(w.inv_perm.ptr, inv_perm.data(), (size_t)npad * sizeof(int), hipMemcpyHostToDevice, s));
    h->call_timer.start(s);
    hipLaunchKernelGGL(ease_gather32_kernel, dim3(div_up(npad, 256), std::min(npad, 1024)), dim3(256), 0, s, w.A.ptr, h->A.ptr, (int64_t)npad, npad,
                       w.inv_perm.ptr);
    MI_HIP(hipGetLastError());
    h->call_timer.stop(s);
    h->launches += PIVOT_GATHER_LAUNCHES;
    MI_HIP(hipStreamSynchronize(s));
    h->invert_ms += h->call_timer.elapsed_ms();
}

}  // namespace

extern "C" int mi355rec_ease_invert_pivoted(mi355rec_ease_t h) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL argument");
        require_invertible(h, "invert_pivoted");
        ensure_work(h);                                         // (no memory: the matrix is still there, the state stays ST_MATRIX)
        begin_invert(h);
        EasePivotWork &w = h->pivot;
        hipStream_t s = h->stream;
        const int npad = h->npad;
        w.valid = false;
        hipLaunchKernelGGL(ease_pivot_init_kernel, dim3(div_up(npad, 256)), dim3(256), 0, s, w.piv.ptr, npad, w.info.ptr);
        hipLaunchKernelGGL(ease_widen64_kernel, dim3(std::min<int64_t>(((int64_t)npad * npad + 255) / 256, 65536)), dim3(256), 0, s, h->A.ptr, w.A.ptr,
                           (int64_t)npad * npad);
        h->launches += PIVOT_FRONT_LAUNCHES;
        if (h->block == 64) enqueue_pivoted_elimination<64>(h);
        else enqueue_pivoted_elimination<128>(h);
        stop_elimination(h);
        double info[2] = {0, 0};
        std::vector<int> piv((size_t)npad);
        MI_HIP(hipMemcpyAsync(info, w.info.ptr, sizeof(info), hipMemcpyDeviceToHost, s));
        MI_HIP(hipMemcpyAsync(piv.data(), w.piv.ptr, (size_t)npad * sizeof(int), hipMemcpyDeviceToHost, s));
        const int failed = await_elimination(h);
        note_pivot_figures(h, info);
        if (failed < 0) gather_result(h, piv);
        finish_invert(h, invert_accounting(*h, sizeof(double)),
                      "the matrix is singular: a pivot that is 0 (or NaN) in elimination step %d of %d (block size %d)");
    });
}

extern "C" int mi355rec_ease_pivot_info(mi355rec_ease_t h, int32_t *moved_rows, double *min_pivot, double *pivot_ms, double *update_ms) {
    return guarded([&] {
        MI_REQUIRE(h && moved_rows && min_pivot && pivot_ms && update_ms, "NULL argument");
        MI_REQUIRE(h->pivot.valid, "no pivoted inverse has run on the matrix that is set");
        *moved_rows = h->pivot.moved;
        *min_pivot = h->pivot.min_pivot;
        *pivot_ms = h->pivot.pivot_ms;
        *update_ms = h->pivot.update_ms;
    });
}
