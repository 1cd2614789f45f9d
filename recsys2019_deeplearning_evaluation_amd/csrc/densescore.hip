// densescore.hip -- scoring with DENSE item-item weights on MI355X (gfx950): scores[u] = A[u, :] . B with A sparse (CSR) and B a
// dense n_mid x n_out float32 array in HBM -- BaseItemSimilarityMatrixRecommender._compute_item_score
// (Base/BaseSimilarityMatrixRecommender.py:73-92: URM_train[users].dot(W_sparse)) for a W_sparse that is an ndarray, which is what
// EASE_R_Recommender.fit leaves with its default topK=None (EASE_R/EASE_R_Recommender.py:40-82).  DESIGN.md section 16.
//
// The contract is SciPy's csr @ ndarray (csr_matvecs) bit for bit: every output cell starts at +0.0f and walks the user's stored
// cells IN CSR STORAGE ORDER with acc = acc + (a * B[i][j]) in float32, the product rounded before the add.  Nothing here may
// contract the two into a fused multiply-add (hipcc's default for device code): the pragma below switches contraction off for this
// translation unit and mul_add_rn spells the two roundings out.  The device scores are then the host scores, the lists follow by
// the ranking's tie rule, and two calls give the same bytes (no atomics anywhere).
//
//   dscore_rows_kernel   a workgroup takes one user and one tile of DSCORE_TILE columns; a lane keeps four adjacent columns'
//                        accumulators in registers and walks the profile in storage order: the ids and values are the same in every
//                        lane (scalar loads), UNROLL rows of B are requested (16 bytes per lane, 4 KiB per workgroup and row) before
//                        the first of them is added, the adds stay in order.  The grid runs users fastest, so the workgroups that
//                        are resident together share a column tile: its slab of B (n_mid x DSCORE_TILE x 4 B) is what L2 and the
//                        Infinity Cache serve to the other users of the block.
//   dscore_cand_kernel   candidate rows (EvaluatorNegativeItemSample): one workgroup per user, a candidate column per lane, the same
//                        recurrence per cell -- a candidate's score is bitwise the full row's cell -- then cand_filter_rank (cand.cuh).
// Ranking of full rows is the factor scorer's (score.hip: rank_rows_enqueue -- score_rank_kernel in LDS, WideRanker beyond).
// A non-finite B is scored as IEEE arithmetic gives it (0 * inf = NaN, as on the host); NaN scores are never listed.
// A translation unit of its own, as cand.hip and itemscore.hip: score.hip's device code does not depend on it.
#include "common.h"
#include "score.h"
#include "topk.cuh"
#include "cand.cuh"

#include <algorithm>
#include <cstdlib>

#pragma clang fp contract(off)

namespace mi355rec {
namespace {

constexpr int DSCORE_THREADS = 256;
constexpr int DSCORE_TILE = 1024;       // columns of a workgroup's tile: four per lane, one 16-byte load per lane and row of B
constexpr int DSCORE_UNROLL = 8;        // rows of B in flight per lane (the faster one of 4 and 8 at the ML-20M shape)
constexpr int CAND_UNROLL = 4;          // the same for the candidate kernel's 4-byte gathers
static_assert(DSCORE_TILE == 4 * DSCORE_THREADS, "four columns per lane");

// acc + (a * w): two float32 roundings, never one.  Written out under the pragma above: __fmul_rn / __fadd_rn are plain operators
// compiled where the HIP headers define them, under the default contraction, and the two fuse once inlined.
__device__ __forceinline__ float mul_add_rn(float acc, float a, float w) {
    const float product = a * w;
    return acc + product;
}

struct DScoreParams {
    int n_out;
    int64_t ldb;                    // floats between two rows of B: a multiple of 4, rows are 16-byte aligned
    const int *a_ptr, *a_idx;
    const float *a_val, *B;
    const int *users;
    float *scores;                  // [n_batch][n_out]
};

template <int UNROLL>
__global__ __launch_bounds__(DSCORE_THREADS) void dscore_rows_kernel(const DScoreParams p) {
    const int b = blockIdx.x, u = p.users[b];
    const int c0 = blockIdx.y * DSCORE_TILE + threadIdx.x * 4;
    if (c0 >= p.n_out) return;      // (no barrier below; c0 + 3 < ldb: the load of a row's last quad stays inside the row)
    const float *col = p.B + c0;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int q = p.a_ptr[u];
    const int end = p.a_ptr[u + 1];
    for (; q + UNROLL <= end; q += UNROLL) {
        float a[UNROLL];
        float4 w[UNROLL];
#pragma unroll
        for (int r = 0; r < UNROLL; ++r) {
            a[r] = p.a_val[q + r];
            w[r] = *reinterpret_cast<const float4 *>(col + (int64_t)p.a_idx[q + r] * p.ldb);
        }
#pragma unroll
        for (int r = 0; r < UNROLL; ++r) {
            acc.x = mul_add_rn(acc.x, a[r], w[r].x);
            acc.y = mul_add_rn(acc.y, a[r], w[r].y);
            acc.z = mul_add_rn(acc.z, a[r], w[r].z);
            acc.w = mul_add_rn(acc.w, a[r], w[r].w);
        }
    }
    for (; q < end; ++q) {
        const float a = p.a_val[q];
        const float4 w = *reinterpret_cast<const float4 *>(col + (int64_t)p.a_idx[q] * p.ldb);
        acc.x = mul_add_rn(acc.x, a, w.x);
        acc.y = mul_add_rn(acc.y, a, w.y);
        acc.z = mul_add_rn(acc.z, a, w.z);
        acc.w = mul_add_rn(acc.w, a, w.w);
    }
    float *out = p.scores + (size_t)b * p.n_out + c0;
    if ((p.n_out & 3) == 0) {       // every score row is 16-byte aligned
        *reinterpret_cast<float4 *>(out) = acc;
    } else {
        out[0] = acc.x;
        if (c0 + 1 < p.n_out) out[1] = acc.y;
        if (c0 + 2 < p.n_out) out[2] = acc.z;
        if (c0 + 3 < p.n_out) out[3] = acc.w;
    }
}

struct DCandParams {
    CandParams c;
    int64_t ldb;
    const int *a_ptr, *a_idx;
    const float *a_val, *B;
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void dscore_cand_kernel(const DCandParams p) {
    const CandParams &c = p.c;
    extern __shared__ __attribute__((aligned(16))) unsigned char cand_smem[];
    uint64_t *cand = reinterpret_cast<uint64_t *>(cand_smem);
    __shared__ SelectScratch sc;
    __shared__ uint32_t s_nfinite;
    const int tid = threadIdx.x;
    const int b = blockIdx.x, u = c.users[b];
    const int row = c.by_user ? u : b;
    const int k0 = c.cand_ptr[row], ncand = c.cand_ptr[row + 1] - k0;
    const int *items = c.cand_idx + k0;
    const int q0 = p.a_ptr[u], end = p.a_ptr[u + 1];
    if (tid == 0) { s_nfinite = 0; sc.out_count = 0; }
    for (int i = tid; i < ncand; i += THREADS) {
        const int item = items[i];
        const float *col = p.B + item;
        float acc = 0.f;
        int q = q0;
        for (; q + CAND_UNROLL <= end; q += CAND_UNROLL) {
            float a[CAND_UNROLL], w[CAND_UNROLL];
#pragma unroll
            for (int r = 0; r < CAND_UNROLL; ++r) {
                a[r] = p.a_val[q + r];
                w[r] = col[(int64_t)p.a_idx[q + r] * p.ldb];
            }
#pragma unroll
            for (int r = 0; r < CAND_UNROLL; ++r) acc = mul_add_rn(acc, a[r], w[r]);
        }
        for (; q < end; ++q) acc = mul_add_rn(acc, p.a_val[q], col[(int64_t)p.a_idx[q] * p.ldb]);
        cand[i] = cand_entry(c.allowed && !c.allowed[item] ? -INFINITY : acc, i);
    }
    cand_filter_rank<THREADS>(c, u, items, ncand, cand, sc, &s_nfinite, c.ranked + (size_t)b * c.cutoff);
}

int64_t padded_row(int n_out) { return ((int64_t)n_out + 3) & ~(int64_t)3; }

// monotone row pointers starting at 0 and column ids inside [0, n_cols): a stored id is an address (a row of B, a cell of a score row)
void check_csr(const char *what, const int32_t *indptr, const int32_t *indices, int n_rows, int n_cols) {
    MI_REQUIRE(indptr[0] == 0, "%s indptr must start at 0", what);
    for (int r = 0; r < n_rows; ++r) MI_REQUIRE(indptr[r] <= indptr[r + 1], "%s indptr is not monotone", what);
    const int64_t nnz = indptr[n_rows];
    for (int64_t q = 0; q < nnz; ++q)
        MI_REQUIRE(indices[q] >= 0 && indices[q] < n_cols, "%s column id %d outside [0, %d)", what, indices[q], n_cols);
}

void upload_weights(mi355rec_dscorer *h, const float *B) {
    hipStream_t s = h->stream;
    MI_HIP(hipStreamSynchronize(s));                    // (a scoring kernel still running reads the old weights)
    MI_HIP(hipMemcpy2DAsync(h->B.ptr, (size_t)h->ldb * sizeof(float), B, (size_t)h->n_items * sizeof(float), (size_t)h->n_items * sizeof(float),
                            (size_t)h->n_mid, hipMemcpyHostToDevice, s));
    MI_HIP(hipStreamSynchronize(s));
}

int unroll_depth() {
    // (MI355REC_DSCORE_UNROLL: the other instance, for the measurement of DESIGN.md section 16)
    if (const char *v = getenv("MI355REC_DSCORE_UNROLL")) {
        const int d = atoi(v);
        MI_REQUIRE(d == 4 || d == 8, "MI355REC_DSCORE_UNROLL must be 4 or 8, got %d", d);
        return d;
    }
    return DSCORE_UNROLL;
}

}  // namespace

}  // namespace mi355rec

using namespace mi355rec;

// The score + rank half of mi355rec_dscorer_recommend (see mi355rec_scorer::enqueue).  `timer`: the scoring dispatch; `call_timer`:
// scoring + ranking.
Ranking mi355rec_dscorer::enqueue(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed, bool keep_scores) {
    hipStream_t s = stream;
    const int tiles = div_up(n_items, DSCORE_TILE);
    if (tiles > 65535) fail(MI355REC_E_UNSUPPORTED, "score rows of %d items: at most %d", n_items, 65535 * DSCORE_TILE);
    const size_t cells = (size_t)n * n_items;
    reserve((size_t)n * cutoff, cells, score_row_fits_lds(n_items, cutoff) ? 0 : cells);
    call_timer.start(s);
    DScoreParams p{};
    p.n_out = n_items; p.ldb = ldb;
    p.a_ptr = a_ptr.ptr; p.a_idx = a_idx.ptr; p.a_val = a_val.ptr; p.B = B.ptr;
    p.users = users; p.scores = scores.ptr;
    if (unroll == 4) hipExtLaunchKernelGGL(dscore_rows_kernel<4>, dim3(n, tiles), dim3(DSCORE_THREADS), 0, s, timer.t0, timer.t1, 0, p);
    else hipExtLaunchKernelGGL(dscore_rows_kernel<8>, dim3(n, tiles), dim3(DSCORE_THREADS), 0, s, timer.t0, timer.t1, 0, p);
    MI_HIP(hipGetLastError());
    rank_rows_enqueue(this, users, n, cutoff, remove_seen, allowed, keep_scores);
    call_timer.stop(s);
    return Ranking{ranked.ptr, s};
}

Ranking mi355rec_dscorer::enqueue_candidates(const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                                             const CandidateRows &rows) {
    hipStream_t s = stream;
    check_candidate_cutoff(cutoff);
    reserve((size_t)n * cutoff, 0, 0);
    DCandParams p{};
    p.c = cand_params(this, users, cutoff, remove_seen, allowed, rows);
    p.ldb = ldb;
    p.a_ptr = a_ptr.ptr; p.a_idx = a_idx.ptr; p.a_val = a_val.ptr; p.B = B.ptr;
    const size_t lds = (size_t)cand_buffer_entries(rows.longest) * 8;
    auto k = dscore_cand_kernel<CAND_THREADS>;
    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipExtLaunchKernelGGL(k, dim3(n), dim3(CAND_THREADS), (unsigned)lds, s, timer.t0, timer.t1, 0, p);
    MI_HIP(hipGetLastError());
    return Ranking{ranked.ptr, s};
}

void mi355rec_dscorer::fill_recommend_stats(const int32_t *user_ids, int n) {
    double nnz = 0;                                     // stored cells of the batch's profiles: each one streams a row of B
    for (int i = 0; i < n; ++i) nnz += a_ptr_host[user_ids[i] + 1] - a_ptr_host[user_ids[i]];
    stats.call_ms = call_timer.elapsed_ms();
    stats.kernel_ms = timer.elapsed_ms();
    stats.algorithmic_flops = 2.0 * nnz * n_items;
    stats.algorithmic_bytes = 4.0 * nnz * n_items;
}

extern "C" int mi355rec_dscorer_create(mi355rec_dscorer_t *out, int32_t n_users, int32_t n_mid, int32_t n_out, const int32_t *a_indptr,
                                       const int32_t *a_indices, const float *a_data, const float *B, const int32_t *seen_indptr,
                                       const int32_t *seen_indices) {
    return guarded([&] {
        MI_REQUIRE(out && a_indptr && seen_indptr, "NULL argument");
        MI_REQUIRE(n_users > 0 && n_mid > 0 && n_out > 0, "empty model");
        *out = nullptr;
        const size_t na = (size_t)a_indptr[n_users], ns = (size_t)seen_indptr[n_users];
        MI_REQUIRE((a_indices && a_data) || na == 0, "NULL argument");
        MI_REQUIRE(seen_indices || ns == 0, "NULL argument");
        check_csr("profile", a_indptr, a_indices, n_users, n_mid);
        check_csr("seen", seen_indptr, seen_indices, n_users, n_out);
        const int64_t ldb = padded_row(n_out);
        ensure_device();
        size_t free_b = 0, total_b = 0;
        MI_HIP(hipMemGetInfo(&free_b, &total_b));
        const double need = (double)n_mid * (double)ldb * sizeof(float) + (double)((size_t)256 << 20);   // + 256 MiB for score rows and the runtime
        MI_REQUIRE(need <= (double)free_b, "the dense weights of %d x %d cells (%.2f GB) do not fit the device's free memory (%.2f GB)", n_mid, n_out,
                   need / 1e9, free_b / 1e9);
        const int unroll = unroll_depth();
        auto h = open_handle<mi355rec_dscorer>(2);
        h->n_users = n_users; h->n_mid = n_mid; h->n_items = n_out; h->ldb = ldb; h->unroll = unroll;
        hipStream_t s = h->stream;
        h->a_ptr.upload(a_indptr, (size_t)n_users + 1, s);
        h->a_idx.alloc(std::max<size_t>(na, 1));
        h->a_val.alloc(std::max<size_t>(na, 1));
        if (na) {
            MI_HIP(hipMemcpyAsync(h->a_idx.ptr, a_indices, sizeof(int) * na, hipMemcpyHostToDevice, s));
            MI_HIP(hipMemcpyAsync(h->a_val.ptr, a_data, sizeof(float) * na, hipMemcpyHostToDevice, s));
        }
        h->seen_ptr.upload(seen_indptr, (size_t)n_users + 1, s);
        h->seen_idx.alloc(std::max<size_t>(ns, 1));
        if (ns) MI_HIP(hipMemcpyAsync(h->seen_idx.ptr, seen_indices, sizeof(int) * ns, hipMemcpyHostToDevice, s));
        h->allowed.alloc(n_out);
        h->a_ptr_host.assign(a_indptr, a_indptr + n_users + 1);
        h->B.alloc_zero((size_t)n_mid * (size_t)ldb, s);          // (B == NULL: zero weights until update / set_from_ease)
        if (B) upload_weights(h.get(), B);
        MI_HIP(hipStreamSynchronize(s));
        *out = h.release();
    });
}

extern "C" int mi355rec_dscorer_update(mi355rec_dscorer_t h, const float *B) {
    return guarded([&] {
        MI_REQUIRE(h && B, "NULL argument");
        ensure_device();
        upload_weights(h, B);
    });
}

extern "C" int mi355rec_dscorer_set_from_ease(mi355rec_dscorer_t h, mi355rec_ease_t ease) {
    return guarded([&] {
        MI_REQUIRE(h && ease, "NULL argument");
        ensure_device();
        const float *W = nullptr;
        int64_t ld = 0;
        int n = 0;
        ease_weights_device(ease, &W, &ld, &n);         // (the weights are in place and the ease handle's stream has drained)
        MI_REQUIRE(n == h->n_mid && n == h->n_items, "the EASE handle holds %d x %d weights, the scorer's are %d x %d", n, n, h->n_mid, h->n_items);
        hipStream_t s = h->stream;
        MI_HIP(hipStreamSynchronize(s));
        h->call_timer.start(s);
        MI_HIP(hipMemcpy2DAsync(h->B.ptr, (size_t)h->ldb * sizeof(float), W, (size_t)ld * sizeof(float), (size_t)n * sizeof(float), (size_t)n,
                                hipMemcpyDeviceToDevice, s));
        h->call_timer.stop(s);
        MI_HIP(hipStreamSynchronize(s));
        h->stats = mi355rec_stats{};
        h->stats.call_ms = h->stats.kernel_ms = h->call_timer.elapsed_ms();
        h->stats.n_launches = h->stats.n_timed = 1;
        h->stats.algorithmic_bytes = 8.0 * (double)n * n;
    });
}

extern "C" int mi355rec_dscorer_recommend(mi355rec_dscorer_t h, const int32_t *user_ids, int32_t n, int32_t cutoff, int32_t remove_seen,
                                          const uint8_t *item_allowed, int32_t *ranked, float *scores) {
    return guarded([&] { recommend(h, user_ids, n, cutoff, remove_seen, item_allowed, ranked, scores); });
}

extern "C" int mi355rec_dscorer_recommend_candidates(mi355rec_dscorer_t h, const int32_t *user_ids, int32_t n, const int32_t *cand_indptr,
                                                     const int32_t *cand_indices, int32_t cutoff, int32_t remove_seen,
                                                     const uint8_t *item_allowed, int32_t *ranked) {
    return guarded([&] { recommend_candidates(h, user_ids, n, cand_indptr, cand_indices, cutoff, remove_seen, item_allowed, ranked); });
}

extern "C" int mi355rec_dscorer_get_stats(mi355rec_dscorer_t h, mi355rec_stats *stats) { return handle_get_stats(h, stats); }

extern "C" void mi355rec_dscorer_destroy(mi355rec_dscorer_t h) { handle_destroy(h); }
