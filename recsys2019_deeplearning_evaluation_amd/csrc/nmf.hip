// nmf.hip -- the device half of NMFRecommender on MI355X (gfx950)  [DESIGN.md section 12].
//
// The reference (MatrixFactorization/NMFRecommender.py:58-71) hands URM_train to sklearn.decomposition.NMF: coordinate descent or
// multiplicative updates on W (users x k) and H (k x items), then a second solve for W alone.  The handle keeps the URM in both
// layouts, W and Ht = H^T (items x k) -- the BlockPair of blocks.h -- and one value buffer per layout resident; an iteration is
// driven from Python through the step-wise entry points below, because it needs a fresh permutation and the stop statistic on the
// host anyway.  "Side" s is the block being updated (0: W from the CSR layout, 1: Ht from the CSC layout); the other block is held
// fixed, so both half-steps of an iteration are the same code.
//
// The kernels are in nmf_kernels.cuh; products and Gram matrices are blocks.hip's, block * matrix is score.hip's f32 MFMA GEMM
// (gemm_rows_enqueue); every grid, buffer size and accounting figure comes from blocks_plan.h.  This file holds the handle, its
// launches -- one function per timed step -- and its C ABI.
#include "blocks.h"
#include "nmf_kernels.cuh"
#include "score.h"

using namespace mi355rec;
using namespace mi355rec::blocks;

namespace {

enum Phase { PH_PRODUCT = 0, PH_GEMM, PH_SWEEP, PH_SCALE, PH_SDDMM, PH_REDUCE, N_PHASES };

}  // namespace

struct mi355rec_nmf : BlockPair {
    double norm_x = 0.0, sum_x = 0.0;                  // sum of x^2; sum of the x above eps32
    DeviceBuffer<float> num, den, q[2], Gf, colsum_f;
    DeviceBuffer<double> G[2], colsum_part, colsum[2], red_part, scal;
    DeviceBuffer<int> perm;
    int prepared_side = -1, prepared_loss = -1;        // what Gf and num, or colsum_f, currently hold
    double phase_ms[N_PHASES] = {0, 0, 0, 0, 0, 0};
    std::vector<int> phase_of;                         // of every event pair used in the current call

    void start_call() {                                // a call that failed half-way leaves event pairs behind
        dispatch_timers.reset();
        phase_of.clear();
    }
    // one timed step of a call: what `enqueue` launches, between an event pair booked to `phase`
    template <class F>
    void step(int phase, F &&enqueue) {
        hipEvent_t a, b;
        dispatch_timers.reserve(dispatch_timers.used + 1);
        dispatch_timers.next(a, b, 1 << 30);
        MI_HIP(hipEventRecord(a, stream));
        phase_of.push_back(phase);
        enqueue();
        MI_HIP(hipEventRecord(b, stream));
    }
    // waits for the call's work, books its phases and launches and leaves the figures of the call in `stats`
    void finish_call(int main_phase, int n_launches, CallFigures figures) {
        MI_HIP(hipStreamSynchronize(stream));
        stats = mi355rec_stats{};
        for (int i = 0; i < dispatch_timers.used; ++i) {
            float ms = 0.f;
            MI_HIP(hipEventElapsedTime(&ms, dispatch_timers.start[i], dispatch_timers.stop[i]));
            phase_ms[phase_of[i]] += ms;
            stats.call_ms += ms;
            if (phase_of[i] == main_phase) stats.kernel_ms += ms;
        }
        stats.n_launches = stats.n_timed = dispatch_timers.used;
        stats.n_units = (int64_t)nnz;
        stats.algorithmic_bytes = figures.bytes;
        stats.algorithmic_flops = figures.flops;
        dispatch_timers.reset();
        phase_of.clear();
        launches += n_launches;
        ++calls;
    }

    ~mi355rec_nmf() { shutdown(); }
};

namespace {

void require_block_side(int side) { require_side(side, "W, users x k", "Ht, items x k"); }
void require_loss(int loss) { MI_REQUIRE(loss == 0 || loss == 1, "loss %d: 0 (frobenius) or 1 (kullback-leibler)", loss); }

// ---- single launches --------------------------------------------------------------------------------------------------------------
void enqueue_colsum(mi355rec_nmf *h, int side, float *out_f) {
    const int n = h->rows_of(side), k = h->width;
    const ColsumPlan p = colsum_plan(n);
    hipLaunchKernelGGL(nmf_colsum_kernel, dim3(p.used, column_grid(k)), dim3(NT), 0, h->stream, h->block[side].ptr, n, k, p.rows, h->colsum_part.ptr);
    MI_HIP(hipGetLastError());
    hipLaunchKernelGGL(nmf_colsum_reduce_kernel, dim3(column_grid(k)), dim3(NT), 0, h->stream, h->colsum_part.ptr, p.used, k, h->colsum[side].ptr, out_f);
    MI_HIP(hipGetLastError());
}

// scal[scalar] (+)= red_part[0] + ... + red_part[n - 1]
void enqueue_sum(mi355rec_nmf *h, int n, int scalar, int accumulate) {
    hipLaunchKernelGGL(nmf_sum_kernel, dim3(1), dim3(NT), 0, h->stream, h->red_part.ptr, n, h->scal.ptr + scalar, accumulate);
    MI_HIP(hipGetLastError());
}

template <class T>
void enqueue_dot(mi355rec_nmf *h, const T *a, const T *b, size_t len, int scalar) {
    const int blocks = dot_blocks(len);
    hipLaunchKernelGGL(nmf_dot_kernel<T>, dim3(blocks), dim3(NT), 0, h->stream, a, b, len, h->red_part.ptr);
    MI_HIP(hipGetLastError());
    enqueue_sum(h, blocks, scalar, 0);
}

// q[side] = x / wh per cell, or (log_sum) x log(x / wh) into one red_part cell per workgroup; returns the workgroups
int enqueue_sddmm(mi355rec_nmf *h, int side, bool log_sum) {
    const Side &sd = h->sides[side];
    const int k = h->width, shift = group_shift(k), blocks = sddmm_grid(sd.n_pieces, k);
    if (log_sum)
        hipLaunchKernelGGL(nmf_sddmm_kernel<true>, dim3(blocks), dim3(NT), 0, h->stream, sd.p_row.ptr, sd.p_begin.ptr, sd.p_end.ptr, sd.n_pieces,
                           sd.idx.ptr, h->values(side), h->block[side].ptr, h->block[1 - side].ptr, k, shift, (float *)nullptr, h->red_part.ptr);
    else
        hipLaunchKernelGGL(nmf_sddmm_kernel<false>, dim3(blocks), dim3(NT), 0, h->stream, sd.p_row.ptr, sd.p_begin.ptr, sd.p_end.ptr, sd.n_pieces,
                           sd.idx.ptr, h->values(side), h->block[side].ptr, h->block[1 - side].ptr, k, shift, h->q[side].ptr, (double *)nullptr);
    MI_HIP(hipGetLastError());
    return blocks;
}

// block[side] *= num / den, den = den_m (a matrix) or den_v (one value per column)
void enqueue_scale(mi355rec_nmf *h, int side, const float *den_m, const float *den_v, float zero_to, int floor) {
    const size_t cells = (size_t)h->rows_of(side) * h->width;
    hipLaunchKernelGGL(nmf_scale_kernel, dim3(cell_grid(cells)), dim3(NT), 0, h->stream, h->block[side].ptr, h->num.ptr, den_m, den_v, cells,
                       h->width, zero_to, floor);
    MI_HIP(hipGetLastError());
}

// one half-sweep of block[side], its violation into one red_part cell per workgroup; returns the workgroups
int enqueue_sweep(mi355rec_nmf *h, int side) {
    const int n = h->rows_of(side), k = h->width;
    const SweepPlan p = sweep_plan(n, k);
    if (p.raise_attribute)
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(nmf_cd_sweep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
    hipLaunchKernelGGL(nmf_cd_sweep_kernel, dim3(p.blocks), dim3(NT), p.lds_bytes, h->stream, h->block[side].ptr, n, k, p.shift, h->Gf.ptr, h->num.ptr,
                       h->perm.ptr, h->red_part.ptr);
    MI_HIP(hipGetLastError());
    return p.blocks;
}

// ---- the steps of the calls ---------------------------------------------------------------------------------------------------------
// what a frobenius step on `side` reads of the other block: Gf = its Gram matrix (float32 of the float64 sum), num = URM . other
void prepare_frobenius(mi355rec_nmf *h, int side) {
    const int k = h->width;
    h->step(PH_REDUCE, [&] {
        h->gram(1 - side, h->G[1 - side].ptr);
        hipLaunchKernelGGL(nmf_to_float_kernel, dim3(cell_grid((size_t)k * k)), dim3(NT), 0, h->stream, h->G[1 - side].ptr, h->Gf.ptr, (size_t)k * k);
        MI_HIP(hipGetLastError());
    });
    h->step(PH_PRODUCT, [&] { h->product(side, h->values(side), h->num.ptr); });
    h->prepared_side = side;
    h->prepared_loss = 0;
}

void mu_frobenius(mi355rec_nmf *h, int side, bool reuse) {
    const int n = h->rows_of(side), k = h->width;
    if (!reuse) prepare_frobenius(h, side);
    h->step(PH_GEMM, [&] { gemm_rows_enqueue(h->block[side].ptr, h->iota.ptr, n, k, h->Gf.ptr, k, h->den.ptr, h->stream); });      // Gf is symmetric
    h->step(PH_SCALE, [&] { enqueue_scale(h, side, h->den.ptr, nullptr, EPS32, 0); });
    h->finish_call(PH_SCALE, mu_step_launches(0, reuse, h->sides[side].n_long), mu_frobenius_figures((size_t)n * k, k));
}

void mu_kullback_leibler(mi355rec_nmf *h, int side, bool reuse) {
    if (!reuse) {
        h->step(PH_REDUCE, [&] { enqueue_colsum(h, 1 - side, h->colsum_f.ptr); });
        h->prepared_side = side;
        h->prepared_loss = 1;
    }
    h->step(PH_SDDMM, [&] { enqueue_sddmm(h, side, false); });
    h->step(PH_PRODUCT, [&] { h->product(side, h->q[side].ptr, h->num.ptr); });
    // a zero sum of H's rows becomes eps32 under W; a zero sum of W's columns becomes 1 under H, and H is floored at eps64
    h->step(PH_SCALE, [&] { enqueue_scale(h, side, nullptr, h->colsum_f.ptr, side == 0 ? EPS32 : 1.0f, side == 1 ? 1 : 0); });
    h->finish_call(PH_SDDMM, mu_step_launches(1, reuse, h->sides[side].n_long), mu_kl_figures(h->nnz, h->width));
}

// scal[SC_A] = tr((W^T W)(H H^T)), scal[SC_B] = sum (X H^T) o W
void frobenius_sums(mi355rec_nmf *h) {
    const int k = h->width;
    h->step(PH_REDUCE, [&] {
        h->gram(0, h->G[0].ptr);
        h->gram(1, h->G[1].ptr);
        enqueue_dot<double>(h, h->G[0].ptr, h->G[1].ptr, (size_t)k * k, SC_A);
    });
    // X H^T into `den`: `num` may hold the products a later step reuses
    h->step(PH_PRODUCT, [&] { h->product(0, h->values(0), h->den.ptr); });
    h->step(PH_REDUCE, [&] { enqueue_dot<float>(h, h->den.ptr, h->block[0].ptr, (size_t)h->n_users * k, SC_B); });
}

// scal[SC_A] = sum x log(x / wh), scal[SC_B] = (sum W)(sum H)
void kullback_leibler_sums(mi355rec_nmf *h) {
    int blocks = 0;
    h->step(PH_SDDMM, [&] { blocks = enqueue_sddmm(h, 0, true); });
    h->step(PH_REDUCE, [&] {
        enqueue_sum(h, blocks, SC_A, 0);
        enqueue_colsum(h, 0, nullptr);
        enqueue_colsum(h, 1, nullptr);
        enqueue_dot<double>(h, h->colsum[0].ptr, h->colsum[1].ptr, (size_t)h->width, SC_B);
    });
}

void require_permutation(const int32_t *permutation, int k) {
    std::vector<char> seen(k, 0);
    for (int i = 0; i < k; ++i) {
        const int t = permutation[i];
        MI_REQUIRE(t >= 0 && t < k && !seen[t], "not a permutation of 0 .. %d: entry %d is %d", k - 1, i, t);
        seen[t] = 1;
    }
}

}  // namespace

extern "C" int mi355rec_nmf_create(mi355rec_nmf_t *out, int32_t n_users, int32_t n_items, int32_t k, const int32_t *row_ptr,
                                   const int32_t *row_idx, const float *row_val, const int32_t *col_ptr, const int32_t *col_idx,
                                   const float *col_val) {
    return guarded([&] {
        const PairArgs a{n_users, n_items, k, row_ptr, row_idx, row_val, col_ptr, col_idx, col_val};
        BlockPair::check_create(out, a, "number of components k");
        const ValueScan v = scan_values(row_val, a.nnz());
        MI_REQUIRE(!v.negative, "negative value %g in the URM", (double)v.negative_value);
        *out = nullptr;
        auto h = open_handle<mi355rec_nmf>(1);
        h->norm_x = v.norm_x;
        h->sum_x = v.sum_x;
        ReleaseScope scope(h->stream);
        hipStream_t s = h->stream;
        const PairSizes z = h->create_common(a, v.ones);
        h->num.alloc(z.cap);
        h->den.alloc(z.cap);
        for (int sd = 0; sd < 2; ++sd) {
            h->q[sd].alloc(std::max<size_t>(h->nnz, 1));
            h->G[sd].alloc((size_t)k * k);
            h->colsum[sd].alloc(k);
        }
        h->Gf.alloc((size_t)k * k);
        h->colsum_f.alloc(k);
        h->colsum_part.alloc((size_t)CS_SLABS * k);
        h->red_part.alloc(red_part_cells(h->sides[0].n_pieces, h->sides[1].n_pieces, z.n_max, k));
        h->scal.alloc_zero(N_SCALARS, s);
        h->perm.alloc(k);
        h->dispatch_timers.reserve(8);
        MI_HIP(hipStreamSynchronize(s));
        *out = h.release();
    });
}

extern "C" int mi355rec_nmf_set_block(mi355rec_nmf_t h, int32_t side, const float *X) {
    return guarded([&] {
        require_block_side(side);
        MI_REQUIRE(h && X, "NULL argument");
        ensure_device();
        h->set_block(side, X);
        h->prepared_side = -1;
    });
}

extern "C" int mi355rec_nmf_get_block(mi355rec_nmf_t h, int32_t side, float *X) {
    return guarded([&] {
        require_block_side(side);
        MI_REQUIRE(h && X, "NULL argument");
        ensure_device();
        h->get_block(side, X);
    });
}

extern "C" int mi355rec_nmf_fill_block(mi355rec_nmf_t h, int32_t side, float value) {
    return guarded([&] {
        require_block_side(side);
        MI_REQUIRE(h, "NULL argument");
        MI_REQUIRE(value >= 0.f, "fill value %g is negative", (double)value);
        ensure_device();
        h->start_call();
        const size_t cells = (size_t)h->rows_of(side) * h->width;
        h->step(PH_SCALE, [&] {
            hipLaunchKernelGGL(nmf_fill_kernel, dim3(cell_grid(cells)), dim3(NT), 0, h->stream, h->block[side].ptr, cells, value);
            MI_HIP(hipGetLastError());
        });
        h->prepared_side = -1;
        h->finish_call(PH_SCALE, FILL_LAUNCHES, fill_figures(cells));
    });
}

extern "C" int mi355rec_nmf_cd_sweep(mi355rec_nmf_t h, int32_t side, const int32_t *permutation, int32_t reuse, double *violation) {
    return guarded([&] {
        require_block_side(side);
        MI_REQUIRE(h && permutation, "NULL argument");
        const int k = h->width;
        require_permutation(permutation, k);
        MI_REQUIRE(!reuse || (h->prepared_side == side && h->prepared_loss == 0), "reuse: no frobenius products of side %d are held", side);
        ensure_device();
        h->start_call();
        hipStream_t s = h->stream;
        MI_HIP(hipMemcpyAsync(h->perm.ptr, permutation, k * sizeof(int), hipMemcpyHostToDevice, s));
        h->h2d_bytes += permutation_bytes(k);
        if (!reuse) prepare_frobenius(h, side);
        int blocks = 0;
        h->step(PH_SWEEP, [&] { blocks = enqueue_sweep(h, side); });
        h->step(PH_REDUCE, [&] { enqueue_sum(h, blocks, SC_VIOLATION, 1); });
        if (violation) {
            MI_HIP(hipMemcpyAsync(violation, h->scal.ptr + SC_VIOLATION, sizeof(double), hipMemcpyDeviceToHost, s));
            MI_HIP(hipMemsetAsync(h->scal.ptr + SC_VIOLATION, 0, sizeof(double), s));
            h->d2h_bytes += SCALAR_BYTES;
        }
        h->finish_call(PH_SWEEP, sweep_launches(reuse != 0, h->sides[side].n_long), sweep_figures(h->rows_of(side), k));
    });
}

extern "C" int mi355rec_nmf_mu_step(mi355rec_nmf_t h, int32_t side, int32_t loss, int32_t reuse) {
    return guarded([&] {
        require_block_side(side);
        require_loss(loss);
        MI_REQUIRE(h, "NULL argument");
        MI_REQUIRE(!reuse || (h->prepared_side == side && h->prepared_loss == loss), "reuse: nothing of side %d and loss %d is held", side, loss);
        ensure_device();
        h->start_call();
        if (loss == 0) mu_frobenius(h, side, reuse != 0);
        else mu_kullback_leibler(h, side, reuse != 0);
    });
}

extern "C" int mi355rec_nmf_divergence(mi355rec_nmf_t h, int32_t loss, double *divergence) {
    return guarded([&] {
        require_loss(loss);
        MI_REQUIRE(h && divergence, "NULL argument");
        ensure_device();
        h->start_call();
        if (loss == 0) frobenius_sums(h);
        else kullback_leibler_sums(h);
        h->step(PH_REDUCE, [&] {
            hipLaunchKernelGGL(nmf_divergence_kernel, dim3(1), dim3(64), 0, h->stream, h->scal.ptr, loss, h->norm_x, h->sum_x);
            MI_HIP(hipGetLastError());
        });
        MI_HIP(hipMemcpyAsync(divergence, h->scal.ptr + SC_OUT, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        h->d2h_bytes += SCALAR_BYTES;
        h->finish_call(loss == 0 ? PH_PRODUCT : PH_SDDMM, divergence_launches(loss, h->sides[0].n_long), divergence_figures(h->nnz, h->width));
    });
}

extern "C" int mi355rec_nmf_get_stats(mi355rec_nmf_t h, mi355rec_stats *stats) { return handle_get_stats(h, stats); }

extern "C" int mi355rec_nmf_fit_info(mi355rec_nmf_t h, double *phase_ms, int64_t *launches, int64_t *calls, int64_t *create_bytes,
                                     int64_t *h2d_bytes, int64_t *d2h_bytes, int32_t *all_ones) {
    return guarded([&] {
        MI_REQUIRE(h && phase_ms && launches && calls && create_bytes && h2d_bytes && d2h_bytes && all_ones, "NULL argument");
        for (int p = 0; p < N_PHASES; ++p) phase_ms[p] = h->phase_ms[p];
        h->traffic(launches, calls, create_bytes, h2d_bytes, d2h_bytes, all_ones);
    });
}

extern "C" void mi355rec_nmf_destroy(mi355rec_nmf_t h) { handle_destroy(h); }
