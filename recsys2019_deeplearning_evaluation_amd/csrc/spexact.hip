// spexact.hip -- the EXACT mode of the sparse similarity scorer on MI355X (gfx950): scores[u] = A[u, :] . B with A and B sparse (CSR),
// every score bit for bit what SciPy's csr_matmat gives for float32 operands (Base/BaseSimilarityMatrixRecommender.py:73-92 and
// :101-116: URM_train[users].dot(W_sparse), W_sparse[users].dot(URM_train)).  DESIGN.md section 17.
//
// The contract, per user row: every cell starts at +0.0f; the stored cells (m, w) of A[u] are walked IN STORAGE ORDER and every stored
// cell (j, b) of row m of B does s[j] = s[j] + (w * b) in float32, the product rounded before the add.  Nothing here may contract the
// two into a fused multiply-add (hipcc's default for device code): the pragma below switches contraction off for this translation
// unit.  There is no float atomic anywhere: the order of the adds into a cell is the order of A's cells, never a race.
//
//   spexact_rows_kernel   one workgroup per (user, item tile of at most SPEXACT_TILE columns); the tile of the score row lives in LDS,
//                         cut into sixteen contiguous slices, one per wavefront.  A wavefront OWNS its slice: it zeroes it, walks the
//                         whole profile in storage order, adds the cells of B's rows that fall inside the slice, and stores the slice
//                         to the row in HBM.  Nobody else touches those cells, so the workgroup needs no barrier at all.  B's rows are
//                         strictly ascending (checked when the mode is switched on), so "the part of row m inside slice k" is a
//                         range cuts[m][k] .. cuts[m][k + 1] of the row, found by binary search when the mode is switched on and
//                         again whenever B is replaced (spexact_cuts_kernel, spexact_check_and_cut).  The wavefront takes 64 profile cells at a time: their pieces of B are laid end to
//                         end, every lane loads and multiplies one cell of that sequence (all loads in flight together), then the
//                         pieces are added to the slice one profile cell after the other.
//   spexact_cand_kernel   candidate rows: the candidates are gathered from the full exact rows (a candidate's score IS the row's cell),
//                         then cand_filter_rank (cand.cuh).
//   spexact_check_kernel  every row of B strictly ascending and inside [0, n_items): the first row that is not.
// Full rows are filtered and ranked by the factor scorer's rank_rows_enqueue (score.hip), as the dense scorer's.
// A translation unit of its own, as cand.hip and densescore.hip: the device code of score.hip and cand.hip does not depend on it.
#include "common.h"
#include "score.h"
#include "topk.cuh"
#include "cand.cuh"

#include <algorithm>
#include <climits>

#pragma clang fp contract(off)

namespace mi355rec {
namespace {

constexpr int SPEXACT_THREADS = 1024;
constexpr int SPEXACT_OWNERS = SPEXACT_THREADS / 64;    // wavefronts of a workgroup: each owns one slice of the tile
constexpr int SPEXACT_TILE = 32256;                     // columns of a tile: the widest row score_row_fits_lds ranks in LDS
static_assert(SPEXACT_TILE % SPEXACT_OWNERS == 0, "the widest tile is cut into equal slices");

struct SpExactParams {
    int n_out, tile, slice;         // columns of a tile (<= SPEXACT_TILE) and of an owner's slice (SPEXACT_OWNERS * slice >= tile)
    int n_slices;                   // slices of a whole score row: SPEXACT_OWNERS per tile
    const int *a_ptr, *a_idx, *b_ptr, *b_idx;
    const float *a_val, *b_val;
    const int *cuts;                // [n_mid][n_slices + 1]: where row m of B crosses into slice k (spexact_cuts_kernel)
    const int *users;
    float *scores;                  // [n_batch][n_out], unfiltered
};

// first column of slice k of a score row (k == n_slices: n_out): slice k is owner k % SPEXACT_OWNERS of tile k / SPEXACT_OWNERS
__device__ __forceinline__ int slice_begin(int k, int tile, int slice, int n_out) {
    const int tile_lo = (k / SPEXACT_OWNERS) * tile;
    return min(tile_lo + (k % SPEXACT_OWNERS) * slice, min(tile_lo + tile, n_out));
}

// cuts[m][k] = the first position of row m of B (ascending columns) whose column is >= slice_begin(k): the cells of row m inside
// slice k are cuts[m][k] .. cuts[m][k + 1].  Built once, when the mode is switched on: the scoring kernel then needs no search.
__global__ __launch_bounds__(64) void spexact_cuts_kernel(const int *b_ptr, const int *b_idx, int n_slices, int tile, int slice, int n_out,
                                                          int *cuts) {
    const int m = blockIdx.x;       // one wavefront per row of B, a lane per boundary
    for (int k = threadIdx.x; k <= n_slices; k += 64) {
        const int col = slice_begin(k, tile, slice, n_out);
        int s = b_ptr[m], e = b_ptr[m + 1];
        while (s < e) {
            const int mid = (s + e) >> 1;
            if (b_idx[mid] < col) s = mid + 1; else e = mid;
        }
        cuts[(size_t)m * (n_slices + 1) + k] = s;
    }
}

// The read-modify-writes of one profile cell are behind the wavefront before those of the next one start.  Two successive cells may
// hit the same score cell from DIFFERENT lanes, so program order inside a lane is not enough for the compiler; the wavefront-scope
// fence keeps it from moving an LDS access across this point in any lane.  That suffices because only this wavefront ever touches the
// slice and a wavefront's LDS instructions are executed in the order they are issued: there is nobody to synchronise with, and
// nothing for the hardware to wait for.
__device__ __forceinline__ void next_profile_cell() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(SPEXACT_THREADS) void spexact_rows_kernel(const SpExactParams p) {
    extern __shared__ __attribute__((aligned(16))) float tile_acc[];
    const int lane = threadIdx.x & 63, owner = threadIdx.x >> 6;
    const int b = blockIdx.x, u = p.users[b];
    const int k = blockIdx.y * SPEXACT_OWNERS + owner;                      // this wavefront's slice of the row
    const int lo = slice_begin(k, p.tile, p.slice, p.n_out), hi = slice_begin(k + 1, p.tile, p.slice, p.n_out);
    if (lo >= hi) return;           // (no barrier below)
    float *acc = tile_acc + owner * p.slice;        // acc[j - lo]
    for (int j = lane; j < hi - lo; j += 64) acc[j] = 0.f;
    next_profile_cell();
    const size_t cut_stride = (size_t)p.n_slices + 1;
    const int *__restrict__ b_idx = p.b_idx;
    const float *__restrict__ b_val = p.b_val;
    const int q_end = p.a_ptr[u + 1];
    for (int q0 = p.a_ptr[u]; q0 < q_end; q0 += 64) {
        // lane l: the cells t0 .. t0 + cnt of B that profile cell q0 + l has inside this slice
        int t0 = 0, cnt = 0;
        float w = 0.f;
        if (q0 + lane < q_end) {
            const int *cut = p.cuts + (size_t)p.a_idx[q0 + lane] * cut_stride + k;
            w = p.a_val[q0 + lane];
            t0 = cut[0];
            cnt = cut[1] - t0;
        }
        // the 64 profile cells' pieces laid end to end, in storage order: piece l starts at first[l]
        int end = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int below = __shfl_up(end, d);
            if (lane >= d) end += below;
        }
        const int first = end - cnt;
        const int total = __builtin_amdgcn_readlane(end, 63);
        for (int c0 = 0; c0 < total; c0 += 64) {
            // lane i takes cell c0 + i of that sequence: its piece is the last one that starts at or before it (an empty piece starts
            // where its successor does and comes before it).  Every lane's loads are in flight together.
            const int i = c0 + lane;
            const bool valid = i < total;
            int piece = 0;
#pragma unroll
            for (int step = 32; step > 0; step >>= 1)
                if (__shfl(first, piece + step) <= i) piece += step;
            const int t = __shfl(t0, piece) + (i - __shfl(first, piece));
            const float wp = __shfl(w, piece);
            const int tt = valid ? t : 0;              // (a lane past the end reads a cell that is there and drops it)
            const int col = b_idx[tt];
            const float bv = b_val[tt];
            const int j = col - lo;
            const float product = wp * bv;
            // one profile cell after the other; the lanes of a piece hold different columns (a row of B holds none twice)
            unsigned long long todo = __ballot(valid);
            while (todo) {
                const int cell = __builtin_amdgcn_readlane(piece, __ffsll((long long)todo) - 1);
                const bool mine = valid && piece == cell;
                if (mine) acc[j] = acc[j] + product;
                todo &= ~__ballot(mine);
                next_profile_cell();
            }
        }
    }
    float *row = p.scores + (size_t)b * p.n_out + lo;
    for (int j = lane; j < hi - lo; j += 64) row[j] = acc[j];
}

// the candidates of the exact rows in HBM: scores[b][n_items], unfiltered
template <int THREADS>
__global__ __launch_bounds__(THREADS) void spexact_cand_kernel(const CandParams c, const float *scores, int n_items) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cand_smem[];
    uint64_t *cand = reinterpret_cast<uint64_t *>(cand_smem);
    __shared__ SelectScratch sc;
    __shared__ uint32_t s_nfinite;
    const int tid = threadIdx.x;
    const int b = blockIdx.x, u = c.users[b];
    const int row = c.by_user ? u : b;
    const int c0 = c.cand_ptr[row], ncand = c.cand_ptr[row + 1] - c0;
    const int *items = c.cand_idx + c0;
    const float *srow = scores + (size_t)b * n_items;
    if (tid == 0) { s_nfinite = 0; sc.out_count = 0; }
    for (int i = tid; i < ncand; i += THREADS) {
        const int item = items[i];
        cand[i] = cand_entry(c.allowed && !c.allowed[item] ? -INFINITY : srow[item], i);
    }
    cand_filter_rank<THREADS>(c, u, items, ncand, cand, sc, &s_nfinite, c.ranked + (size_t)b * c.cutoff);
}

// one wavefront per row of B: *first_bad = the lowest row whose column ids are not strictly ascending inside [0, n_out)
__global__ __launch_bounds__(256) void spexact_check_kernel(const int *b_ptr, const int *b_idx, int n_mid, int n_out, int *first_bad) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_mid) return;
    const int s = b_ptr[row], e = b_ptr[row + 1];
    bool bad = false;
    for (int t = s + lane; t < e; t += 64) {
        const int col = b_idx[t];
        bad |= col < 0 || col >= n_out || (t > s && b_idx[t - 1] >= col);
    }
    if (bad) atomicMin(first_bad, row);
}

// h->scores[b][n_items] = the exact row of users[b], unfiltered; the caller has reserved h->scores.  timed: the dispatch carries the
// handle's `timer` events.
void rows_enqueue(mi355rec_spscorer *h, const int *users, int n, bool timed) {
    SpExactParams p{};
    p.n_out = h->n_items;
    p.tile = std::min(h->n_items, SPEXACT_TILE);
    p.slice = div_up(p.tile, SPEXACT_OWNERS);
    p.a_ptr = h->a_ptr.ptr; p.a_idx = h->a_idx.ptr; p.a_val = h->a_val.ptr;
    p.b_ptr = h->b_ptr.ptr; p.b_idx = h->b_idx.ptr; p.b_val = h->b_val.ptr;
    p.users = users; p.scores = h->scores.ptr;
    const int tiles = div_up(h->n_items, p.tile);
    p.n_slices = tiles * SPEXACT_OWNERS; p.cuts = h->cuts.ptr;
    const size_t lds = (size_t)p.slice * SPEXACT_OWNERS * sizeof(float);
    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(spexact_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (timed) hipExtLaunchKernelGGL(spexact_rows_kernel, dim3(n, tiles), dim3(SPEXACT_THREADS), (unsigned)lds, h->stream, h->timer.t0, h->timer.t1, 0, p);
    else hipLaunchKernelGGL(spexact_rows_kernel, dim3(n, tiles), dim3(SPEXACT_THREADS), lds, h->stream, p);
    MI_HIP(hipGetLastError());
}

}  // namespace

// mi355rec_spscorer::enqueue in exact mode: the exact rows go to h->scores, the factor scorer's filter + ranking takes them from there.
// `timer`: the exact kernel alone.
Ranking spexact_enqueue(mi355rec_spscorer *h, const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                        bool keep_scores) {
    const size_t cells = (size_t)n * h->n_items;
    h->reserve((size_t)n * cutoff, cells, score_row_fits_lds(h->n_items, cutoff) ? 0 : cells);
    rows_enqueue(h, users, n, true);
    rank_rows_enqueue(h, users, n, cutoff, remove_seen, allowed, keep_scores);
    return Ranking{h->ranked.ptr, h->stream};
}

// mi355rec_spscorer::enqueue_candidates in exact mode.  `timer`: the exact kernel and the candidates' gather + ranking.
Ranking spexact_enqueue_candidates(mi355rec_spscorer *h, const int *users, int n, int cutoff, int remove_seen, const unsigned char *allowed,
                                   const CandidateRows &rows) {
    hipStream_t s = h->stream;
    check_candidate_cutoff(cutoff);
    h->reserve((size_t)n * cutoff, (size_t)n * h->n_items, 0);
    const CandParams c = cand_params(h, users, cutoff, remove_seen, allowed, rows);
    h->timer.start(s);
    rows_enqueue(h, users, n, false);
    const size_t lds = (size_t)cand_buffer_entries(rows.longest) * 8;
    auto k = spexact_cand_kernel<CAND_THREADS>;
    MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3(n), dim3(CAND_THREADS), lds, s, c, (const float *)h->scores.ptr, h->n_items);
    MI_HIP(hipGetLastError());
    h->timer.stop(s);
    return Ranking{h->ranked.ptr, s};
}

// The pass of exact mode over a B on the device -- the live one (set_exact) or one in the spare buffers that is about to replace it
// (update_b, update_from_slim: the table is a function of B and is swapped in together with it).  The caller holds a ReleaseScope
// over `s`.
void spexact_check_and_cut(mi355rec_spscorer *h, hipStream_t s, const int *b_ptr, const int *b_idx, DeviceBuffer<int> *cuts) {
    DeviceBuffer<int> first_bad;
    int bad = INT_MAX;
    first_bad.upload(&bad, 1, s);
    hipLaunchKernelGGL(spexact_check_kernel, dim3(div_up(h->n_mid, 4)), dim3(256), 0, s, b_ptr, b_idx, h->n_mid, h->n_items, first_bad.ptr);
    MI_HIP(hipGetLastError());
    first_bad.download(&bad, 1, s);
    MI_HIP(hipStreamSynchronize(s));
    MI_REQUIRE(bad == INT_MAX, "exact mode: row %d of B does not hold its column ids strictly ascending inside [0, %d) (a column twice, or unsorted)",
               bad, h->n_items);
    if (!cuts) return;
    const int tile = std::min(h->n_items, SPEXACT_TILE), slice = div_up(tile, SPEXACT_OWNERS);
    const int tiles = div_up(h->n_items, tile);
    if (tiles > 65535) fail(MI355REC_E_UNSUPPORTED, "score rows of %d items: at most %d in exact mode", h->n_items, 65535 * SPEXACT_TILE);
    const int n_slices = tiles * SPEXACT_OWNERS;
    const size_t cells = (size_t)h->n_mid * (n_slices + 1);
    if (cells > ((size_t)1 << 32)) fail(MI355REC_E_UNSUPPORTED, "exact mode: %d rows of B x %d slices of a score row do not fit its table", h->n_mid, n_slices);
    cuts->alloc(cells);
    hipLaunchKernelGGL(spexact_cuts_kernel, dim3(h->n_mid), dim3(64), 0, s, b_ptr, b_idx, n_slices, tile, slice, h->n_items, cuts->ptr);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(s));
}

size_t spexact_table_cells(const mi355rec_spscorer *h) {
    if (!h->exact) return 0;
    const int tiles = div_up(h->n_items, std::min(h->n_items, SPEXACT_TILE));
    return (size_t)h->n_mid * ((size_t)tiles * SPEXACT_OWNERS + 1);
}

}  // namespace mi355rec

using namespace mi355rec;

extern "C" int mi355rec_spscorer_set_exact(mi355rec_spscorer_t h, int32_t exact) {
    return guarded([&] {
        MI_REQUIRE(h, "NULL argument");
        if (!exact) {
            h->exact = 0;
            return;
        }
        ensure_device();
        hipStream_t s = h->stream;
        ReleaseScope scope(s);
        // (the table of the B the scorer holds: a second switch-on finds it there; a call that replaces B replaces the table with it,
        // or drops it while the mode is off)
        DeviceBuffer<int> cuts;
        spexact_check_and_cut(h, s, h->b_ptr.ptr, h->b_idx.ptr, h->cuts.count ? nullptr : &cuts);
        if (!h->cuts.count) h->cuts.swap(cuts);
        h->exact = 1;
    });
}
