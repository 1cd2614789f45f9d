// sim_kernels.cuh -- the column kernels of Compute_Similarity: SimParams, the cell maps (normalise, euclidean_cell, DenomForm), the LDS
// helpers, sim_column_kernel (32-bit / 64-bit cells) and sim_packed_kernel (two 16-bit counts per word).  Included by sim.hip after
// common.h and topk.cuh; the constants the host's schedule shares with the kernels are in sim_plan.h.
#pragma once

#include "sim_plan.h"

namespace mi355rec {
namespace {

// chunks a lane group keeps in flight in the counts instance (round 5: 6 and 8 measured at ML-20M shape: 4.19 / 4.27 ms against 3.99-4.15:
// the stream is not what the accumulation waits for)
#ifndef SIM_DEPTH_UNIT
#define SIM_DEPTH_UNIT 4
#endif
constexpr int MAX_TILE = 32256;      // uint32 count cells of the LDS accumulator: 4 B * (32256 + 4) + 32 KiB selection scratch + statics <= 160 KiB
constexpr int MAX_TILE_F64 = 16128;  // float64 cells (real-valued data): 8 B * (16128 + 4) + 32 KiB
constexpr int NORM_PAD = 1024 + 4;     // zeros behind the norm arrays: the threshold-first selection reads whole rounds of 1024 cells
constexpr int F64_CELLS_PER_THREAD = 16;   // >= MAX_TILE_F64 / 1024 (and the 512-thread launches have <= 5116 cells)

struct SimParams {
    int n_rows, n_cols, n_cols_pad;    // n_cols_pad: neighbour cells of the LDS accumulator (tile width, multiple of 4)
    int acc_cells;                     // n_cols_pad + 4 spare cells that absorb the padding entries of the profiles
    int acc_words;                     // 32-bit words of the accumulator: acc_cells (uint32 counts) or 2 * acc_cells (float64)
    int topK;
    int kind, normalize, unit_col;
    int avg_row, euclid_mode;          // MI355REC_SIM_EUCLIDEAN
    float shrink, tversky_alpha, tversky_beta;
    const int *csr_ptr;
    // Profile stream: every (row, accumulator tile) segment of the CSR matrix, padded to a multiple of 8 entries so
    // that a 16-byte chunk is either entirely inside a segment or entirely outside (no per-entry bounds checks in the
    // hot loop).  Ids are uint16 relative to the tile base; padding entries carry the id of a spare cell and value 0.
    const int *seg_ptr;                // [n_rows * n_tiles + 1], multiples of 8
    const unsigned short *seg_idx16;
    const float *seg_val;
    const short *seg_val16;            // ACC_INT32: the stored values times 2^s as 16-bit integers (same entry order as seg_idx16); seg_val is absent then
    int tile_w, n_tiles;               // accumulator tile width and count (1 when n_cols fits the LDS)
    int *cand_idx;                     // n_tiles > 1: per-workgroup scratch [n_tiles * topK] of per-tile candidates
    float *cand_val;
    const int *csc_ptr, *csc_idx;
    const float *csc_val;
    // Walk lists (built by the constructor, build_walk): per column, what the accumulation walks -- one entry per SLICE of a user's
    // profile segment (at most WALK_SLICE chunks of 8 entries), longest slices first.  All-ones data: walk4 = the slice's number, whose
    // {first entry, end entry} in the profile stream are walk_tab[number] (a 4-byte entry: this list IS the column view of all-ones data,
    // sorted once); valued data: walk16 = {first, end, bits of the column-side value times the row weight, 0}.
    // With accumulator tiles (n_tiles > 1) an entry is a whole user: the row (walk4 / walk16.x), whose per-tile segment bounds come
    // from seg_ptr.
    const int *walk4;
    const uint2 *walk_tab;
    const uint4 *walk16;
    const float *row_w;
    const float *norm, *norm_alpha, *norm_1ma;
    const int4 *items;  // work items of this call, most expensive first: {column, part, n_parts, first part slot}
    const int2 *item_range;   // per work item: the column's [begin, end) in the CSC arrays (saves a dependent round trip per column)
    int n_items, start_col;
    const int *out_slot;    // interleaved parts: output row of every column of the call (NULL: column - start_col)
    float int_scale, int_inv;   // ACC_INT32: 4^s (both factors of a product carry 2^s) and its inverse
    float int_half;             // ACC_INT32: 2^s
    double fixed_scale;     // real-valued data: > 0 = the accumulator holds int64 fixed-point sums, products scaled by this power of two
    double fixed_inv;       //                   (1 / fixed_scale); 0 = float64 sums
    uint32_t *part_buf;     // [part slots][n_cols_pad] partial accumulators of split columns
    unsigned *part_count;   // arrival counters, indexed by the first part slot of a split column
    unsigned long long *phase_ticks;   // diagnostics (MI355REC_SIM_PHASES=1): 100 MHz ticks per phase, summed over workgroups
    int fast_topk;          // 1: threshold-first selection (fast_column_topk) where it applies; 0 (MI355REC_SIM_FAST_TOPK=0): always the full normalise + radix select
    // packed-counts launch + the 32-bit launch behind it (run_columns_lds): the second launch's work list is its own items followed by
    // the columns the packed kernel hands over; *retry_count = its length (read once at kernel start when n_items_dev is set)
    int *retry_count;
    int4 *retry_items;
    int2 *retry_ranges;
    const int *n_items_dev;
    unsigned long long *fast_stats;    // [0] columns finished by the fast path, [1] their candidates, [2] columns that fell back
    unsigned *queue;
    int *out_idx;
    float *out_val;
    float *out_dense;  // [n_local][n_cols] when topK == 0
};

// Denominators of compute_similarity (.pyx:473-504); the +1e-6 is the reference's.  norm_c / norm_j are the column
// norms of the two items (asymmetric cosine: norm^(2 alpha) of c and norm^(2 (1 - alpha)) of j).
__device__ __forceinline__ float normalise(const SimParams &p, float v, float norm_c, float norm_j) {
    if (p.normalize) return v / (norm_c * norm_j + p.shrink + 1e-6f);
    if (p.kind == MI355REC_SIM_JACCARD) return v / (norm_c + norm_j - v + p.shrink + 1e-6f);
    if (p.kind == MI355REC_SIM_DICE) return v / (norm_c + norm_j + p.shrink + 1e-6f);
    if (p.kind == MI355REC_SIM_TVERSKY)
        return v / (v + (norm_c - v) * p.tversky_alpha + (norm_j - v) * p.tversky_beta + p.shrink + 1e-6f);
    if (p.shrink != 0.f) return v / p.shrink;
    return v;
}

// Compute_Similarity_Euclidean.compute_similarity (Euclidean.py:167-203), one cell: the reference works in float32
// NumPy arithmetic (the dtype of the URM), one operation per statement -- restated with explicitly rounded float32
// operations so that no multiply-add is contracted.  sq_* = sum of squares of the column, rt_* = its square root.
// Deviation: a squared distance that rounds below zero is clamped to 0 (the reference takes sqrt of it and emits nan).
// row_weights (:62-72): the dot product is the weighted one (the accumulation multiplies every user's contribution by its weight,
// = dataMatrix_weighted.T.dot(item_data), :153), and the distance VECTOR over the columns is multiplied element by element by the
// weights of the ROWS (:174-175) -- defined for square inputs only, where column j meets row j's weight `w_j`.
__device__ __forceinline__ float euclidean_cell(const SimParams &p, float dot, float sq_c, float sq_j, float rt_c, float rt_j,
                                                float w_j = 1.f, bool weighted = false) {
    float d2 = __fsub_rn(__fadd_rn(sq_j, sq_c), __fmul_rn(2.f, dot));          // (a-b)^2 = a^2 + b^2 - 2ab   (:167-172)
    if (weighted) d2 = __fmul_rn(d2, w_j);                                     // :174-175
    if (p.normalize) d2 = __fdiv_rn(d2, __fmul_rn(rt_c, rt_j));                // :178-179
    if (p.avg_row) d2 = __fdiv_rn(d2, (float)p.n_rows);                        // :181-182
    const float d = __fsqrt_rn(fmaxf(d2, 0.f));                                // :184
    float f = d;                                                               // "lin" :189-190
    if (p.euclid_mode == MI355REC_EUCLID_EXP) f = expf(d);                     // :186-187
    else if (p.euclid_mode == MI355REC_EUCLID_LOG) f = logf(__fadd_rn(d, 1.f));  // :192-193
    return __fdiv_rn(1.f, __fadd_rn(__fadd_rn(f, p.shrink), 1e-9f));
}

// The denominator of `normalise` in ONE form for every mode, d = a * norm_j + (c * v + b), evaluated with two fused operations: used only
// to ORDER cells (the threshold-first selection); every value that is emitted comes from `normalise` itself.
//   normalize (cosine, asymmetric ...)   a = norm_c   b = shrink + 1e-6             c = 0
//   jaccard                              a = 1        b = norm_c + shrink + 1e-6    c = -1
//   dice                                 a = 1        b = norm_c + shrink + 1e-6    c = 0
//   tversky                              a = beta     b = alpha norm_c + shrink + 1e-6   c = 1 - alpha - beta
//   shrink only                          a = 0        b = shrink                    c = 0
//   none                                 a = 0        b = 1                         c = 0      (v * rcp(1) = v)
struct DenomForm {
    float a, b, c;
};
__device__ __forceinline__ DenomForm denominator_form(const SimParams &p, float norm_c) {
    const float s6 = p.shrink + 1e-6f;
    if (p.normalize) return {norm_c, s6, 0.f};
    if (p.kind == MI355REC_SIM_JACCARD) return {1.f, norm_c + s6, -1.f};
    if (p.kind == MI355REC_SIM_DICE) return {1.f, norm_c + s6, 0.f};
    if (p.kind == MI355REC_SIM_TVERSKY) return {p.tversky_beta, __builtin_fmaf(p.tversky_alpha, norm_c, s6), 1.f - p.tversky_alpha - p.tversky_beta};
    if (p.shrink != 0.f) return {0.f, p.shrink, 0.f};
    return {0.f, 1.f, 0.f};
}
__device__ __forceinline__ float approx_denominator(const DenomForm &f, float v, float norm_j) {
    return __builtin_fmaf(f.a, norm_j, __builtin_fmaf(f.c, v, f.b));
}

// float64 -> int64 by the "magic number" addition: for |x| < 2^51, bits(x + 1.5 * 2^52) - bits(1.5 * 2^52) = round-to-nearest-even(x)
constexpr double FIXED_MAGIC = 6755399441055744.0;
constexpr long long FIXED_MAGIC_BITS = 0x4338000000000000ll;

// THREADS: workgroup size; G: lanes that cooperate on one user profile (sub-wave group);
// MODE: what the accumulator cells hold.
//   ACC_COUNTS  all stored values are 1.0 (implicit / set-based data): uint32 co-occurrence counts, the value arrays are never read;
//   ACC_INT32   every stored value is a small multiple of a power of two (star ratings, half stars): the products, scaled by that
//               power of two squared, are small integers and their sums are EXACT in an int32 cell -- ds_add_u32 at the speed of the
//               counts, and one accumulator tile where 8-byte cells need two (26 744 columns at ML-20M shape);
//   ACC_WIDE    any other real-valued data (or row weights): int64 fixed-point or float64 sums in 8-byte cells.
struct alignas(16) SimShared {
    int4 item;
    int2 range;
    int col, last;
    uint32_t npos, nneg, ncand, kmin, kmax;
    SelectScratch sc;
};
// LDS byte address of the cell whose id is half `HI` of the packed id pair `w` (the accumulator starts at LDS address 0)
template <int HI, int SHIFT>
__device__ __forceinline__ unsigned lds_cell_address(unsigned w) {
    unsigned a;
    if (HI) asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(a) : "v"((unsigned)SHIFT), "v"(w));
    else asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(a) : "v"((unsigned)SHIFT), "v"(w));
    return a;
}
typedef __attribute__((address_space(3))) unsigned lds_u32_t;
typedef __attribute__((address_space(3))) unsigned long long lds_u64_t;
typedef __attribute__((address_space(3))) double lds_f64_t;
__device__ __forceinline__ void lds_add_u32(unsigned byte_address, unsigned v) {
    __hip_atomic_fetch_add((lds_u32_t *)(size_t)byte_address, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_add_u64(unsigned byte_address, unsigned long long v) {
    __hip_atomic_fetch_add((lds_u64_t *)(size_t)byte_address, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_add_f64(unsigned byte_address, double v) {
    __hip_atomic_fetch_add((lds_f64_t *)(size_t)byte_address, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int THREADS, int G, int MODE>
__global__ __launch_bounds__(THREADS, 4) void sim_column_kernel(const SimParams p) {
    constexpr bool UNIT = MODE == ACC_COUNTS;        // no values
    constexpr bool CELL32 = MODE != ACC_WIDE;        // 4-byte integer cells
    // LDS: [accumulator | selection scratch | the workgroup's few shared scalars].  The kernel has NO static LDS, so the accumulator
    // starts at LDS address 0 and a cell's address is its id times the cell size -- one SDWA shift per entry instead of extract + shift
    // + base (lds_cell_address; checked once below).
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *acc = smem;
    uint32_t *aux = reinterpret_cast<uint32_t *>(smem + p.acc_words);
    SimShared &shared = *reinterpret_cast<SimShared *>(aux + AUX_WORDS);
    SelectScratch &sc = shared.sc;
    int &s_col = shared.col, &s_last = shared.last;
    int4 &s_item = shared.item;
    int2 &s_range = shared.range;
    uint32_t &s_npos = shared.npos, &s_nneg = shared.nneg, &s_ncand = shared.ncand, &s_kmin = shared.kmin, &s_kmax = shared.kmax;
    if ((unsigned)(size_t)(__attribute__((address_space(3))) float *)smem != 0u) __builtin_trap();

    const int tid = threadIdx.x, lane = tid & 63;
    const int gl = tid % G;

    unsigned long long t_prev = p.phase_ticks ? wall_clock64() : 0ull;
    // (diagnostics: [8] earliest start, [9] latest end, [10] sum of the workgroups' own spans, [11] longest single work item, [12] its column)
    const unsigned long long t_start = t_prev;
    if (p.phase_ticks && tid == 0) atomicMin(&p.phase_ticks[8], t_start);
    auto mark = [&](int phase) {
        if (p.phase_ticks && tid == 0) {
            const unsigned long long now = wall_clock64();
            atomicAdd(&p.phase_ticks[phase], now - t_prev);
            t_prev = now;
        }
    };
    // The next work item is pulled while the current one is still in its normalisation / top-K phases: thread 0 issues the queue
    // atomic after the accumulation (A), requests the item's descriptor one phase later (B) and files both in LDS after the
    // top-K (C), where the loop head finds them -- without it every column starts with three dependent round trips (queue ->
    // descriptor -> CSC bounds: 2-3 us of ~20).  None of this state is live during the accumulation (the register peak).
    // (behind a packed-counts launch the list has grown by the columns that kernel handed over: its length is read from the device)
    const int n_items = p.n_items_dev ? *p.n_items_dev : p.n_items;
    int nx_slot = -1;                        // thread 0 only
    auto pull_now = [&]() {                  // thread 0, synchronous: the first item, and after a split column's part that does not finish the column
        const int sl = nx_slot >= 0 ? nx_slot : (int)atomicAdd(p.queue, 1u);
        s_col = sl;
        if (sl < n_items) {
            s_item = p.items[sl];
            s_range = p.item_range[sl];
        }
        nx_slot = -1;
    };
    if (tid == 0) pull_now();
    // (Measured and rejected, round 6: requesting the next column's first walk entries while the current column's survivors are ranked.
    // Every __syncthreads waits for ALL outstanding loads of the wavefront, so the requests were simply waited for at the next barrier
    // of the selection -- its phase grew by what the loop head saved, 3.85 ms against 3.81.)
    for (;;) {
        __syncthreads();
        const int slot = s_col;
        if (slot >= n_items) break;
        const int4 item = s_item;
        const unsigned long long t_item = p.phase_ticks ? wall_clock64() : 0ull;
        auto item_done = [&]() {
            if (p.phase_ticks && tid == 0) {
                const unsigned long long span = wall_clock64() - t_item;
                if (span > atomicMax(&p.phase_ticks[11], span)) p.phase_ticks[12] = (unsigned long long)item.x;
            }
        };
        const int c = item.x;
        const int cbeg = s_range.x, cend = s_range.y;    // the column's walk list
        int4 nx_item = make_int4(0, 0, 0, 0);
        int2 nx_range = make_int2(0, 0);
        auto request_next = [&]() {          // (B) thread 0
            if (nx_slot < n_items) {
                nx_item = p.items[nx_slot];
                nx_range = p.item_range[nx_slot];
            }
        };
        auto file_next = [&]() {             // (C) thread 0
            s_col = nx_slot;
            s_item = nx_item;
            s_range = nx_range;
            nx_slot = -1;
        };
        // (a heavy column split over several workgroups, item.z > 1: this one is part item.y, whose wavefronts take their stripes of
        // the walk list like the wavefronts of any other part -- see the dealing below)
        const size_t out_base = (size_t)(p.out_slot ? p.out_slot[c] : c - p.start_col) * p.topK;
        int *wg_cand_idx = p.cand_idx + (size_t)blockIdx.x * p.n_tiles * p.topK;
        float *wg_cand_val = p.cand_val + (size_t)blockIdx.x * p.n_tiles * p.topK;
        long long total_nonzero = 0;

        // Columns wider than the LDS accumulator are processed in tiles of tile_w neighbour ids: every CSR entry
        // belongs to exactly one (row, tile) segment of the profile stream (ids are stored tile-relative), so the
        // tiles together read each profile once.  n_tiles == 1 is the common case.
        for (int tile = 0; tile < p.n_tiles; ++tile) {
        const int tile_base = tile * p.tile_w;
        const int n_tile = min(p.tile_w, p.n_cols - tile_base);
        if (tid == 0) {
            s_npos = 0;
            s_nneg = 0;
            s_ncand = 0;
            s_kmin = 0xFFFFFFFFu;
            s_kmax = 0u;
        }

        // The column's walk list (slices of user profiles, longest first) is dealt to the wavefronts in stripes: units of GPW consecutive
        // entries -- one per lane group -- go to the NV = WAVES x parts "virtual wavefronts" of the column in serpentine order (every
        // other stripe reversed), so every wavefront of every part sees the same mix of lengths; entry q of virtual wavefront vw is
        //     cbeg + ((q / GPW) * NV + pos) * GPW + q % GPW,     pos = vw or NV - 1 - vw by the parity of the stripe q / GPW.
        // Consecutive entries of the sorted list have (nearly) the same number of chunks: the GPW groups of a wavefront finish their
        // entries of a round together and the wavefronts of a column finish together -- with the CSC's row order and whole profiles
        // one heavy user kept its lane group busy while the others idled (42 of 64 lanes per ds_add at ML-20M shape, scripts/analysis/
        // sim_lane_census.py; 59 with this dealing).
        constexpr int WAVES = THREADS / 64, GPW = 64 / G;
        const int wave = tid >> 6, sub = lane / G;
        const int NV = WAVES * item.z, vw = item.y * WAVES + wave;
        auto entry_in = [&](int first, int nv, int v, int q) {       // position in a column's walk list of the q-th entry of its virtual wavefront v of nv
            const int stripe = q / GPW, pos = (stripe & 1) ? nv - 1 - v : v;
            return first + (stripe * nv + pos) * GPW + (q % GPW);
        };
        auto entry_of = [&](int q) { return entry_in(cbeg, NV, vw, q); };
        // Walk entries (and, with accumulator tiles, the CSR bounds behind them) are the only dependent loads of the stream.  They
        // run two rounds (of 64 entries per wavefront) ahead: entries of round r+2 and bounds of round r+1 are requested while round r
        // streams, and the first round's entries are requested before the accumulator is cleared.
        auto load_entry = [&](int at, int end, int &ex, int &ey, float &cv) {
            if (at < end) {
                if (UNIT) {
                    ex = p.walk4[at];
                    ey = 0;
                    cv = 1.f;
                } else {
                    const uint4 e = p.walk16[at];
                    ex = (int)e.x;
                    ey = (int)e.y;
                    cv = __uint_as_float(e.z);
                }
            } else {
                ex = 0;
                ey = -1;                               // (marks a lane without an entry)
            }
        };
        auto load_user = [&](int q, int &ex, int &ey, float &cv) { load_entry(entry_of(q), cend, ex, ey, cv); };
        auto load_bounds = [&](int ex, int ey, float cv, int &rs, int &re, float &r) {
            r = cv;
            if (p.n_tiles == 1) {
                if (UNIT && ey >= 0) {                 // the slice's bounds: one more (L2-resident) look-up, a round ahead like the tiles' bounds
                    const uint2 e = p.walk_tab[ex];
                    ex = (int)e.x;
                    ey = (int)e.y;
                }
                rs = ex;
                re = ey;
            } else if (ey >= 0) {                      // accumulator tiles: .x is the row
                const int *sp = p.seg_ptr + ((size_t)ex * p.n_tiles + tile);
                rs = sp[0];
                re = sp[1];
            } else {
                rs = 0;
                re = -1;
            }
        };
        int x_first = 0, y_first = -1, x_next = 0, y_next = -1, t_rs = 0, t_re = -1;
        float cv_first = 1.f, cv_next = 1.f, t_r = 0.f;
        load_user(lane, x_first, y_first, cv_first);
        load_user(64 + lane, x_next, y_next, cv_next);

        // ---- clear this_item_weights (.pyx:365-370) ----
        {
            float4 *a4 = reinterpret_cast<float4 *>(acc);
            for (int w = tid; w < p.acc_words / 4; w += THREADS) a4[w] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        load_bounds(x_first, y_first, cv_first, t_rs, t_re, t_r);
        __syncthreads();
        mark(0);

        // ---- computeItemSimilarities (.pyx:376-406): users of column c, then every item of each user ----
        // A wavefront takes 64 of its users per round: lane l puts user l's CSR bounds and weight into a
        // wavefront-private table in the selection scratch.  Its GPW lane groups then walk the table round-robin,
        // streaming each profile segment in 16-byte chunks (8 uint16 column ids per lane).  Segments are padded to whole
        // chunks, so a lane's chunk is valid or not as a whole: the accumulation is 8 x (extract id, ds_add) with
        // nothing else -- on the 16-lane SIMDs of CDNA every wave64 VALU instruction costs 4 issue cycles, and the
        // per-entry bounds checks of an unpadded layout made this loop VALU-issue-bound (3.7 of 5.8 ms at ML-20M shape).
        // The stream is also latency-bound (one workgroup per CU = 16 wavefronts, each load ~1 us away), so every group
        // runs a fetch cursor DEPTH chunks ahead of its consume cursor: DEPTH loads per lane in flight, issued
        // unconditionally (finished groups re-read a hot line) so that the wait counters are static and the consume
        // side only ever waits for the oldest chunk.
        // UNIT data accumulates integer counts with ds_add_u32; real-valued data accumulates float64 products -- like the
        // reference, whose accumulator is a double array.  (Measured on gfx950, random cells, per CU and ns: ds_add_u32 21.6
        // lane-adds, ds_add_u64 13.2, ds_add_f64 7.2, ds_add_f32 0.8 -- the float32 LDS atomic is 27x slower than the integer
        // one and 9x slower than the float64 one.)  Because the 64-bit INTEGER atomic is 1.8x faster than the float64 one, the
        // products are accumulated as int64 fixed point whenever the host found a power-of-two scale that keeps every sum
        // inside 62 bits and every product's rounding below 1e-7 of the smallest normalised result (p.fixed_scale > 0):
        // x * scale is rounded to an integer by adding 1.5 * 2^52 in float64 (one fma) and subtracting that constant's bits;
        // integer sums are exact and independent of the order of the adds.
        // (exact int32 sums: ids and values are one 16-byte chunk each per lane -- three of them in flight)
        constexpr int DEPTH = UNIT ? SIM_DEPTH_UNIT : (MODE == ACC_INT32 ? 3 : 2);
        unsigned *acc_u = reinterpret_cast<unsigned *>(acc);
        double *acc_d = reinterpret_cast<double *>(acc);
        const bool fixed_point = MODE == ACC_WIDE && p.fixed_scale > 0.0;
        // (the id stream through a buffer descriptor: a 32-bit byte offset per load instead of 64-bit address arithmetic; the stream holds
        // fewer than 2^31 entries of 2 bytes -- checked by the constructor -- so the descriptor's 32-bit size covers it)
        const __amdgpu_buffer_rsrc_t idx_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(p.seg_idx16), 0, (int)0xFFFFFFF0u, 0x00020000);
        const float4 *val4 = reinterpret_cast<const float4 *>(p.seg_val);
        const uint4 *val8 = reinterpret_cast<const uint4 *>(p.seg_val16);
        int4 *tab = reinterpret_cast<int4 *>(aux) + wave * 64;       // [64] x {rs, re, weight, -}: one 16-byte read per entry
        // All-ones data, one tile (the headline instance): the same walk with the bookkeeping pared down.  The table holds {first, end}
        // pairs (128 per wavefront, the upper half stays {0, 0}: a group that has run out of entries reads an empty slice and stays where
        // it is); per step a group checks whether its slice is used up, READS ITS NEXT TABLE ENTRY UNCONDITIONALLY (no branch, no nested
        // loop, no count of pending chunks) and applies it after the eight atomics of the oldest chunk, then fetches: 36 instructions
        // per step where the general loop below has 61.  Measured in round 6: the phase takes the same time either way (524 against
        // 518 workgroup-ms at ML-20M shape) -- like prefetch depth, the stream's origin and the atomics' count, the instruction count
        // is not what it waits for; kept because sim_packed_kernel shares the loop and it is the
        // simpler code.
        const bool lean = UNIT && p.n_tiles == 1;
        int2 *tab2 = reinterpret_cast<int2 *>(aux) + wave * 128;
        if (lean) tab2[64 + lane] = make_int2(0, 0);
        for (int base = 0; entry_of(base) < cend; base += 64) {
            const bool have = t_re >= 0;                 // (a prefix of the lanes: entry_of grows with q)
            const int n_here = __popcll(__ballot(have));
            if (lean) tab2[lane] = have ? make_int2(t_rs, t_re) : make_int2(0, 0);
            else if (have) tab[lane] = make_int4(t_rs, t_re, __float_as_int(t_r), 0);
            load_bounds(x_next, y_next, cv_next, t_rs, t_re, t_r);                     // for the next round
            load_user(base + 128 + lane, x_next, y_next, cv_next);                    // for the round after
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (lean) {
                const int g8 = 8 * gl;
                int m = sub;
                int f_t, f_re;
                {
                    const int2 e = tab2[m];
                    f_t = e.x;
                    f_re = e.y;
                }
                uint4 ids[DEPTH];
                bool ok[DEPTH];
                auto fetch = [&](int d) {
                    const int at = f_t + g8;
                    ok[d] = at < f_re;
                    ids[d] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(idx_rsrc, at * 2, 0, 0));
                    f_t += 8 * G;
                };
                auto step = [&](int d) {
                    const bool done = f_t >= f_re;           // (group-uniform: the slice is used up)
                    m = min(m + (done ? GPW : 0), 127);
                    const int2 e = tab2[m];                  // requested before the atomics below, needed after them
                    if (ok[d]) {
                        const unsigned ww[4] = {ids[d].x, ids[d].y, ids[d].z, ids[d].w};
#pragma unroll
                        for (int q = 0; q < 8; ++q)
                            lds_add_u32((q & 1) ? lds_cell_address<1, 2>(ww[q >> 1]) : lds_cell_address<0, 2>(ww[q >> 1]), 1u);
                    }
                    f_t = done ? e.x : f_t;
                    f_re = done ? e.y : f_re;
                    fetch(d);
                };
#pragma unroll
                for (int d = 0; d < DEPTH; ++d) {
                    if (d) {
                        const bool done = f_t >= f_re;
                        m = min(m + (done ? GPW : 0), 127);
                        const int2 e = tab2[m];
                        f_t = done ? e.x : f_t;
                        f_re = done ? e.y : f_re;
                    }
                    fetch(d);
                }
                for (;;) {
                    bool any = false;
#pragma unroll
                    for (int d = 0; d < DEPTH; ++d) {
                        any |= ok[d];
                        step(d);
                    }
                    if (__ballot(any) == 0ull) break;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    // the table is rewritten by the next round
                __builtin_amdgcn_wave_barrier();
                continue;
            }

            // fetch cursor of this lane group
            int m = sub - GPW, f_t = 0, f_re = 0;
            float f_r = 0.f;
            bool f_have = true;
            auto next_user = [&]() {        // moves the fetch cursor to the group's next non-empty segment
                do {
                    m += GPW;
                    f_have = m < n_here;
                    if (f_have) {
                        const int4 e = tab[m];
                        f_t = e.x;
                        f_re = e.y;
                        f_r = __int_as_float(e.z);
                    }
                } while (f_have && f_t >= f_re);      // empty segments exist only with accumulator tiles
            };
            next_user();
            uint4 ids[DEPTH];
            float4 vlo[DEPTH], vhi[DEPTH];
            int c_t[DEPTH], c_re[DEPTH];      // chunk position of the lane; end of the group's segment (0: no chunk)
            float c_r[DEPTH];
            int pending = 0;
            auto fetch = [&](int d) {
                const int at = f_have ? f_t + 8 * gl : 8 * gl;       // finished groups: a valid, cache-hot address
                c_t[d] = at;
                c_re[d] = f_have ? f_re : 0;
                c_r[d] = f_r;
                ids[d] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(idx_rsrc, at * 2, 0, 0));
                if (MODE == ACC_INT32) {
                    vlo[d] = __builtin_bit_cast(float4, val8[at >> 3]);       // eight int16 values
                } else if (!UNIT) {
                    vlo[d] = val4[at >> 2];
                    vhi[d] = val4[(at >> 2) + 1];
                }
                if (f_have) {
                    ++pending;
                    f_t += 8 * G;
                    if (f_t >= f_re) next_user();
                }
            };
            // (An interleaved lane <-> entry mapping -- neighbouring lanes on neighbouring profile entries, hoping for
            // neighbouring LDS banks -- was measured 11 % slower than 8 consecutive entries per lane.)
            auto consume = [&](int d) {
                if (c_re[d] > 0) --pending;
                if (c_t[d] < c_re[d]) {
                    const unsigned ww[4] = {ids[d].x, ids[d].y, ids[d].z, ids[d].w};
                    const float vv[8] = {vlo[d].x, vlo[d].y, vlo[d].z, vlo[d].w, vhi[d].x, vhi[d].y, vhi[d].z, vhi[d].w};
                    const double rd = (double)c_r[d];
                    if (MODE == ACC_INT32) {
                        // (column value * 2^s) * (row value * 2^s): two integers of at most 12 bits -- the row side comes from the stream
                        // as int16 (a third of the bytes of ids + float32 values: the stream, not the atomics, was what made this
                        // instance twice as slow as the counts), one 24-bit multiply, an integer add
                        const int ri = __float2int_rn(c_r[d] * p.int_half);
                        const uint4 vq = __builtin_bit_cast(uint4, vlo[d]);
                        const unsigned vw[4] = {vq.x, vq.y, vq.z, vq.w};
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const unsigned at = (e & 1) ? lds_cell_address<1, 2>(ww[e >> 1]) : lds_cell_address<0, 2>(ww[e >> 1]);
                            const int v = (e & 1) ? (int)vw[e >> 1] >> 16 : (int)(short)(vw[e >> 1] & 0xFFFFu);
                            lds_add_u32(at, (unsigned)__mul24(ri, v));
                        }
                    } else if (MODE == ACC_WIDE && fixed_point) {
                        const double rs = rd * p.fixed_scale;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const unsigned at = (e & 1) ? lds_cell_address<1, 3>(ww[e >> 1]) : lds_cell_address<0, 3>(ww[e >> 1]);
                            const double q = __builtin_fma(rs, (double)vv[e], FIXED_MAGIC);
                            lds_add_u64(at, (unsigned long long)(__double_as_longlong(q) - FIXED_MAGIC_BITS));
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            if (UNIT) lds_add_u32((e & 1) ? lds_cell_address<1, 2>(ww[e >> 1]) : lds_cell_address<0, 2>(ww[e >> 1]), 1u);
                            else lds_add_f64((e & 1) ? lds_cell_address<1, 3>(ww[e >> 1]) : lds_cell_address<0, 3>(ww[e >> 1]), rd * (double)vv[e]);
                        }
                    }
                }
            };
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) fetch(d);
            while (pending > 0) {
#pragma unroll
                for (int d = 0; d < DEPTH; ++d) {
                    consume(d);
                    fetch(d);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");    // the table is rewritten by the next round
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        mark(1);
        if (tid == 0 && tile == 0) nx_slot = (int)atomicAdd(p.queue, 1u);       // next work item: requested now, looked at later
        if (UNIT && item.w < 0) {
            // A column with 65 536 users or more behind a packed-counts launch: its parts (each fewer users than that) were accumulated
            // there, two 16-bit counts per word, and published; this item -- {column, 0, 1, -(1 + first slot)} with the EMPTY walk list
            // [parts, parts) -- adds them up into 32-bit cells and selects.
            const int n_words = p.n_cols_pad / 2;
            const uint32_t *src = p.part_buf + (size_t)(-(item.w + 1)) * p.n_cols_pad;
            for (int w = tid; w < n_words; w += THREADS) {
                unsigned lo = 0u, hi = 0u;
                for (int q = 0; q < cbeg; ++q) {
                    const unsigned v = src[(size_t)q * p.n_cols_pad + w];
                    lo += v & 0xFFFFu;
                    hi += v >> 16;
                }
                acc_u[2 * w] = lo;
                acc_u[2 * w + 1] = hi;
            }
            __syncthreads();
            mark(2);
        }
        if (item.z > 1) {
            const int pub_words = CELL32 ? p.n_cols_pad : 2 * p.n_cols_pad;
            // Split column: publish this part's accumulator; the workgroup that arrives last adds the parts up (in
            // part order, so the float result does not depend on arrival order) and carries on with the column.
            // Nobody waits for anybody.
            {
                uint4 *dst = reinterpret_cast<uint4 *>(p.part_buf + (size_t)(item.w + item.y) * pub_words);   // spare cells are not published
                const uint4 *src = reinterpret_cast<const uint4 *>(acc);
                for (int w = tid; w < pub_words / 4; w += THREADS) dst[w] = src[w];
            }
            // Every wavefront waits until its own stores have reached the L2; after the barrier ONE thread makes them
            // visible device-wide (agent-scope release: L2 write-back) and counts the arrival; the last arriver
            // acquires (invalidates this CU's L1 / stale L2 lines) on behalf of the whole workgroup.  A fence per
            // thread costs ~50 us per part on gfx950 (16 wavefronts x write-back + invalidate).
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                __threadfence();
                s_last = atomicAdd(&p.part_count[item.w], 1u) == (unsigned)(item.z - 1);
                if (s_last) __threadfence();
            }
            __syncthreads();
            if (!s_last) {
                mark(2);
                if (tid == 0) pull_now();
                continue;
            }
            const uint4 *src = reinterpret_cast<const uint4 *>(p.part_buf + (size_t)item.w * pub_words);
            const size_t stride4 = (size_t)pub_words / 4;
            for (int w = tid; w < pub_words / 4; w += THREADS) {
                uint4 a = src[w];
                for (int q = 1; q < item.z; ++q) {
                    const uint4 b = src[q * stride4 + w];
                    if (CELL32) {
                        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
                    } else if (p.fixed_scale > 0.0) {   // two int64 cells
                        const unsigned long long a0 = (((unsigned long long)a.y << 32) | a.x) + (((unsigned long long)b.y << 32) | b.x);
                        const unsigned long long a1 = (((unsigned long long)a.w << 32) | a.z) + (((unsigned long long)b.w << 32) | b.z);
                        a = make_uint4((unsigned)a0, (unsigned)(a0 >> 32), (unsigned)a1, (unsigned)(a1 >> 32));
                    } else {   // two float64 cells
                        const double a0 = __hiloint2double((int)a.y, (int)a.x) + __hiloint2double((int)b.y, (int)b.x);
                        const double a1 = __hiloint2double((int)a.w, (int)a.z) + __hiloint2double((int)b.w, (int)b.z);
                        a = make_uint4((unsigned)__double2loint(a0), (unsigned)__double2hiint(a0), (unsigned)__double2loint(a1),
                                       (unsigned)__double2hiint(a1));
                    }
                }
                reinterpret_cast<uint4 *>(acc)[w] = a;
            }
            __syncthreads();
            mark(2);
        }
        // the diagonal was accumulated like any other cell: clear it (the reference never adds to it, .pyx:392)
        if (tid == 0 && c >= tile_base && c < tile_base + n_tile) {
            if (CELL32) acc[c - tile_base] = 0.f;
            else acc_d[c - tile_base] = 0.0;
        }
        if (CELL32 && p.fast_topk) {
            // the histogram of block_kth_largest_prefix16 (256 words; the wavefront tables are dead) and, with the spare cells (they
            // absorbed the padding entries), the zeros the last round of the selection's scans reads behind the tile
            for (int w = tid; w < 1024; w += THREADS) aux[w] = 0u;
            if (tid < 4) acc[p.n_cols_pad + tid] = 0.f;
        }
        __syncthreads();

        // ---- threshold-first top-K (4-byte cells, one tile, topK > 0, a positive denominator) ----
        // The full path below divides every cell (IEEE division: ~10 VALU operations), counts signs and key ranges, and then
        // scans the 26 744 cells of an ML-20M column two or three more times for the radix select: 17.8 of the ~19 us a column costs
        // besides its accumulation.  Only the K winners need their exact value.  So: (A) every thread takes the maximum of
        // v * rcp(denominator) over its own cells (approximate: a few ulp) -- the K-th largest of these THREADS maxima is a lower
        // bound T0 on the K-th largest cell of the column, and a tight one (the winners of a column are spread over the threads);
        // (B) one more scan compares v with Tf * denominator, Tf = T0 (1 - 2^-19): no division, and the margin (32 ulp) covers the
        // rounding of both approximations (<= 4 ulp each), so every cell whose EXACT value reaches the exact K-th largest value
        // passes -- ties included; (C) the survivors (~1.05 K) are divided exactly (`normalise`, the same instructions as below),
        // ranked by (value, lowest index first) and the first K emitted.  The result is identical to the full path's, bit for bit
        // (tests/test_sim_gpu.py::test_fast_topk_equals_full_selection).  Fewer than K positive thread maxima (sparse columns) or
        // more survivors than the candidate buffer holds (4 096: masses of equal values): the full path runs, the accumulator is untouched.
        if (CELL32 && p.fast_topk && !(item.z == 1 && item.w == 1)) {          // (.w == 1: a light column, see the schedule)
            const bool asym = p.normalize && p.kind == MI355REC_SIM_ASYMMETRIC;
            const float norm_c = asym ? p.norm_alpha[c] : p.norm[c];
            const float4 *nj4 = reinterpret_cast<const float4 *>(asym ? p.norm_1ma : p.norm);
            const uint32_t K = (uint32_t)p.topK;
            // Thread t owns the cells t, t + THREADS, t + 2 THREADS, ...: neighbouring ids -- whose values are often neighbours too
            // (ids ordered by popularity or by age) -- sit in different threads, so a run of large cells is a run of large thread maxima.
            // (With four adjacent cells per thread the bound was loose: 262 survivors per column for K = 100.)  Cells and norms are
            // fetched in rounds of THREADS: ds_read_b32 at one address register + a constant offset; the norms with buffer loads (one
            // offset register, the round in the scalar offset, zeros beyond the array) -- nothing per cell is kept between the two
            // scans: 32 norms per thread do not fit next to the kernel's state in the 128 registers of a 1024-thread workgroup (they
            // went to scratch and came back one dependent reload per cell).  The round that straddles the end of the tile reads the
            // spare cells and the first words of the selection scratch: all zero (cleared above; the histogram is zero again when
            // block_kth_largest_prefix16 returns), and a zero cell neither raises a maximum nor passes the bar.
            constexpr int CPT = (MAX_TILE + 1023) / 1024;      // rounds (512-thread tiles are narrower than half of MAX_TILE)
            constexpr int CAND_MAX = AUX_WORDS / 2;            // 8-byte entries: (norm, id) of a survivor, then its (value key, ~id)
            constexpr int BATCH = 16, HALF = 8;
            const float *nj = reinterpret_cast<const float *>(nj4);
            const __amdgpu_buffer_rsrc_t nj_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(nj), 0, n_tile * 4, 0x00020000);
            int tid_o = tid;                                   // (opaque: or the 32 addresses are computed before the persistent loop and parked in scratch)
            asm volatile("" : "+v"(tid_o));
            const int n_rounds = (p.n_cols_pad + THREADS - 1) / THREADS;
            const DenomForm form = denominator_form(p, norm_c);
            auto cell_value = [&](unsigned q) { return UNIT ? (float)q : (float)(int)q * p.int_inv; };
            // one batch of rounds: the norms of BATCH cells are requested together, the cells are read from LDS while they are on their
            // way, then `use(round, value, norm)`.  Rounds behind the tile (a batch is not cut short) and the lanes of the last round
            // that lie behind it read the first spare cell: zero.
            const unsigned cell_at = (unsigned)tid_o * 4u, cell_end = (unsigned)p.n_cols_pad * 4u;      // byte offsets into the accumulator
            auto request_norms = [&](int b, float (&dst)[BATCH]) {
#pragma unroll
                for (int i = 0; i < BATCH; ++i)
                    dst[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(nj_rsrc, tid_o * 4, (b + i) * THREADS * 4, 0));
            };
            // (sixteen norms per request and thread, nothing requested ahead: a scan of an ML-20M column is two L2 round trips instead of
            // the four that eight double-buffered norms made it -- working on eight cells never hid the next request's latency; the same
            // 24 registers: sixteen norms + eight cells)
            auto scan_cells = [&](auto &&use) {
#pragma unroll
                for (int bi = 0; bi < CPT / BATCH; ++bi) {
                    const int b = bi * BATCH;
                    if (b >= n_rounds) break;                              // (block-uniform)
                    float nrm[BATCH];
                    request_norms(b, nrm);
#pragma unroll
                    for (int hf = 0; hf < BATCH / HALF; ++hf) {
                        unsigned cnt[HALF];
#pragma unroll
                        for (int i = 0; i < HALF; ++i)
                            cnt[i] = *reinterpret_cast<const unsigned *>(reinterpret_cast<const char *>(acc) +
                                                                         min(cell_at + (unsigned)(b + hf * HALF + i) * (THREADS * 4u), cell_end));
#pragma unroll
                        for (int i = 0; i < HALF; ++i) use(b + hf * HALF + i, cell_value(cnt[i]), nrm[hf * HALF + i]);
                    }
                }
            };
            // (A) thread maxima of the approximate values
            float m = 0.f;
            scan_cells([&](int, float v, float norm_j) { m = fmaxf(m, v * __builtin_amdgcn_rcpf(approx_denominator(form, v, norm_j))); });
            mark(5);
            if (p.phase_ticks) {          // (diagnostics only: the wait for the slowest wavefront of the scan, apart from the selection)
                __syncthreads();
                mark(7);
            }
            // (block_kth_largest_bin12 -- one 12-bit pass, three barriers, 4 060 cycles against 5 960 in scripts/micro/kth_select.hip --
            // was measured here: the phase went from 91 to 63 workgroup-ms, its 12 % more survivors cost 4 of them back, and the
            // un-instrumented kernel was 0.08-0.11 ms SLOWER in both sessions: the two-pass 16-bit prefix stays)
            const uint32_t p16 = block_kth_largest_prefix16<THREADS>(float_key(m), K, aux, sc);
            mark(3);
            bool done = p16 > (ZERO_KEY >> 16);                    // else: fewer than K threads hold a positive cell
            if (done) {
                if (tid == 0 && tile == 0) request_next();
                const float Tf = key_float(p16 << 16) * 0.99999809265136719f;        // 1 - 2^-19
                // (B) cells that can reach the top K -> list of (neighbour norm, cell id)
                uint64_t *cand = reinterpret_cast<uint64_t *>(aux);
                if (tid == 0) sc.out_count = 0;
                scan_cells([&](int round, float v, float norm_j) {
                    // (v > 0 is tested on its own: the rounds of a batch that lie behind the tile read zero CELLS by construction, but their
                    // NORMS rest on the buffer range check covering the scalar offset -- a zero cell must not pass on a stale norm)
                    if (v > 0.f && v >= Tf * approx_denominator(form, v, norm_j)) {
                        const uint32_t at = atomicAdd(&s_ncand, 1u);
                        if (at < (uint32_t)CAND_MAX) cand[at] = ((uint64_t)__float_as_uint(norm_j) << 32) | (uint32_t)(tid_o + round * THREADS);
                    }
                });
                __syncthreads();
                mark(6);
                const uint32_t n_cand = s_ncand;
                if (n_cand > (uint32_t)CAND_MAX || n_cand < K) {         // (n_cand < K cannot happen: at least K cells passed (A)'s bar)
                    __syncthreads();
                    if (tid == 0) s_ncand = 0;
                    if (p.fast_stats && tid == 0) atomicAdd(&p.fast_stats[2], 1ull);
                    if (p.fast_stats && tid == 0 && n_cand > (uint32_t)CAND_MAX) atomicAdd(&p.fast_stats[3], 1ull);
                    done = false;
                } else {
                    if (p.fast_stats && tid == 0) {
                        atomicAdd(&p.fast_stats[0], 1ull);
                        atomicAdd(&p.fast_stats[1], (unsigned long long)n_cand);
                    }
                    // (C) the survivors' exact values (one survivor per thread, in place), rank, emit
                    for (uint32_t t = tid; t < n_cand; t += THREADS) {
                        const uint64_t e = cand[t];
                        const uint32_t j = (uint32_t)e;
                        const float x = normalise(p, cell_value(acc_u[j]), norm_c, __uint_as_float((uint32_t)(e >> 32)));
                        cand[t] = ((uint64_t)float_key(x) << 32) | (uint32_t)(~j);
                    }
                    __syncthreads();
                    block_rank_emit<THREADS>(cand, (int)n_cand, p.topK, K, 0u, sc, p.out_idx + out_base, p.out_val + out_base);
                }
            }
            if (done) {
                if (tid == 0 && tile == 0) file_next();
                __syncthreads();
                mark(4);
                continue;
            }
        }

        // ---- normalisation (.pyx:473-504), in place; count signs for the selection ----
        uint32_t npos = 0, nneg = 0, kmin = 0xFFFFFFFFu, kmax = 0u;   // key range of the positive cells
        {
            const bool asym = p.normalize && p.kind == MI355REC_SIM_ASYMMETRIC;
            const bool euclid = p.kind == MI355REC_SIM_EUCLIDEAN;      // every cell but the diagonal gets a value
            const float norm_c = asym ? p.norm_alpha[c] : p.norm[c];
            const float sq_c = euclid ? p.norm_alpha[c] : 0.f;         // euclidean: norm_alpha holds the sums of squares
            const float *nj = (asym ? p.norm_1ma : p.norm) + tile_base;
            const float *sqj = p.norm_alpha + tile_base;
            auto account = [&](float v) {
                npos += v > 0.f;
                nneg += v < 0.f;
                if (v > 0.f) {
                    const uint32_t key = float_key(v);
                    kmin = min(kmin, key);
                    kmax = max(kmax, key);
                }
            };
            if (CELL32) {
                // counts, or exact integer sums of products scaled by int_scale (a power of four)
                auto cell_value = [&](unsigned q) { return UNIT ? (float)q : (float)(int)q * p.int_inv; };
                const float4 *nj4 = reinterpret_cast<const float4 *>(nj);
                float4 *a4 = reinterpret_cast<float4 *>(acc);
                const int n_quads = p.n_cols_pad / 4;
                // four cells per thread and step (the norm arrays are padded to a multiple of 4; cells beyond n_tile are 0)
                if (euclid) {
                    for (int w = tid; w < n_quads; w += THREADS) {
                        const uint4 qu = reinterpret_cast<const uint4 *>(acc)[w];
                        const float4 n4 = nj4[w];
                        const float4 s4 = reinterpret_cast<const float4 *>(sqj)[w];
                        float vv[4] = {cell_value(qu.x), cell_value(qu.y), cell_value(qu.z), cell_value(qu.w)};
                        const float nn[4] = {n4.x, n4.y, n4.z, n4.w};
                        const float ss[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int j = 4 * w + e;
                            vv[e] = (j < n_tile && tile_base + j != c) ? euclidean_cell(p, vv[e], sq_c, ss[e], norm_c, nn[e]) : 0.f;
                            account(vv[e]);
                        }
                        a4[w] = make_float4(vv[0], vv[1], vv[2], vv[3]);
                    }
                } else {
                    // The neighbours' norms come from L2: loaded inside the loop, behind the test for an all-zero quad, every
                    // step paid a full round trip (6.5 of them per column at ML-20M shape = the whole phase); all of a thread's
                    // quads are requested up front instead (8 steps cover MAX_TILE / 4 / 1024; 512-thread tiles are narrower).
                    constexpr int NPF = 8;
                    float4 npf[NPF];
                    const int n_quads_valid = (n_tile + 3) >> 2;          // (the last tile is narrower than the accumulator: the norm arrays end with it)
#pragma unroll
                    for (int i = 0; i < NPF; ++i) {
                        const int w = tid + i * THREADS;
                        npf[i] = nj4[w < n_quads_valid ? w : 0];
                    }
#pragma unroll
                    for (int i = 0; i < NPF; ++i) {
                        const int w = tid + i * THREADS;
                        if (w < n_quads) {
                            const uint4 qu = reinterpret_cast<const uint4 *>(acc)[w];
                            if ((qu.x | qu.y | qu.z | qu.w) != 0u) {
                                float vv[4] = {cell_value(qu.x), cell_value(qu.y), cell_value(qu.z), cell_value(qu.w)};
                                const float nn[4] = {npf[i].x, npf[i].y, npf[i].z, npf[i].w};
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    if (vv[e] != 0.f) {
                                        vv[e] = normalise(p, vv[e], norm_c, nn[e]);
                                        account(vv[e]);
                                    }
                                }
                                a4[w] = make_float4(vv[0], vv[1], vv[2], vv[3]);
                            }
                        }
                    }
                }
            } else {
                // float64 sums -> normalised float32 values in the first half of the same LDS bytes.  In two batches of cells
                // (half the registers of one batch of 16: the 1024-thread instance sits at its 128-register cap): batch h reads
                // cells [8h T, 8(h+1) T) -- bytes [64h T, 64(h+1) T) -- into registers, barrier, writes float32 to bytes
                // [32h T, 32(h+1) T): batch 0 overwrites only cells it has read itself, batch 1 only cells batch 0 has read.
                // The norms are loaded unconditionally (not behind `v != 0`), so that the 8 loads of a batch are in flight together.
                constexpr int HALF = F64_CELLS_PER_THREAD / 2;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    float reg[HALF], njv[HALF], sqv[HALF];
#pragma unroll
                    for (int k = 0; k < HALF; ++k) {
                        const int j = tid + (half * HALF + k) * THREADS;
                        njv[k] = nj[j < n_tile ? j : 0];
                        sqv[k] = euclid ? sqj[j < n_tile ? j : 0] : 0.f;
                    }
#pragma unroll
                    for (int k = 0; k < HALF; ++k) {
                        const int j = tid + (half * HALF + k) * THREADS;
                        float v = 0.f;
                        if (j < n_tile) {
                            v = p.fixed_scale > 0.0 ? (float)((double)(long long)reinterpret_cast<const unsigned long long *>(acc)[j] * p.fixed_inv)
                                                    : (float)acc_d[j];
                            if (euclid) {
                                if (tile_base + j != c) {
                                    const bool weighted = p.row_w != nullptr;       // (weights always take this accumulator)
                                    v = euclidean_cell(p, v, sq_c, sqv[k], norm_c, njv[k], weighted ? p.row_w[tile_base + j] : 1.f, weighted);
                                } else {
                                    v = 0.f;
                                }
                                account(v);
                            } else if (v != 0.f) {
                                v = normalise(p, v, norm_c, njv[k]);
                                account(v);
                            }
                        }
                        reg[k] = v;
                    }
                    __syncthreads();
#pragma unroll
                    for (int k = 0; k < HALF; ++k) {
                        const int j = tid + (half * HALF + k) * THREADS;
                        if (j < p.n_cols_pad) acc[j] = reg[k];
                    }
                }
            }
        }
        if (p.topK == 0) {  // dense output (.pyx:507-510)
            if (tid == 0 && tile == 0) {
                request_next();
                file_next();
            }
            __syncthreads();
            float *dst = p.out_dense + (size_t)(p.out_slot ? p.out_slot[c] : c - p.start_col) * p.n_cols + tile_base;
            for (int j = tid; j < n_tile; j += THREADS) dst[j] = acc[j];
            __syncthreads();
            continue;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            npos += __shfl_down(npos, off);
            nneg += __shfl_down(nneg, off);
            kmin = min(kmin, (uint32_t)__shfl_down(kmin, off));
            kmax = max(kmax, (uint32_t)__shfl_down(kmax, off));
        }
        if (lane == 0) {
            if (npos) {
                atomicAdd(&s_npos, npos);
                atomicMin(&s_kmin, kmin);
                atomicMax(&s_kmax, kmax);
            }
            if (nneg) atomicAdd(&s_nneg, nneg);
        }
        __syncthreads();
        npos = s_npos;
        nneg = s_nneg;
        total_nonzero += npos + nneg;
        mark(3);
        if (tid == 0 && tile == 0) request_next();                               // its descriptor arrives during the top-K
        if (p.n_tiles == 1) {
            // ---- top-K: the K largest cells of the FULL column (zeros compete, then are dropped), value-descending,
            //      emitted like the COO triples of .pyx:550-562 with -1 padding ----
            block_topk_emit<THREADS>(acc, n_tile, p.topK, npos, nneg, TOPK_ZEROS_COMPETE, aux, sc, &s_ncand,
                                     p.out_idx + out_base, p.out_val + out_base, 0, nullptr, -1, s_kmin, s_kmax);
        } else {
            // the tile's K best non-zero cells go to the workgroup's scratch; zeros are accounted for in the merge
            block_topk_emit<THREADS>(acc, n_tile, p.topK, npos, nneg, TOPK_NONZERO, aux, sc, &s_ncand,
                                     wg_cand_idx + tile * p.topK, wg_cand_val + tile * p.topK, tile_base);
        }
        if (tid == 0 && tile == 0) file_next();
        __syncthreads();
        mark(4);
        }  // tiles

        if (p.n_tiles > 1 && p.topK > 0) {
            // ---- merge of the per-tile candidates: the K largest of the whole column, zeros competing ----
            const int n_m = p.n_tiles * p.topK;
            if (tid == 0) { s_npos = 0; s_nneg = 0; s_ncand = 0; }
            __threadfence_block();
            __syncthreads();
            uint32_t npos = 0, nneg = 0;
            for (int j = tid; j < n_m; j += THREADS) {
                const float v = wg_cand_idx[j] >= 0 ? wg_cand_val[j] : 0.f;
                acc[j] = v;
                npos += v > 0.f;
                nneg += v < 0.f;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                npos += __shfl_down(npos, off);
                nneg += __shfl_down(nneg, off);
            }
            if (lane == 0) {
                if (npos) atomicAdd(&s_npos, npos);
                if (nneg) atomicAdd(&s_nneg, nneg);
            }
            __syncthreads();
            block_topk_emit<THREADS>(acc, n_m, p.topK, s_npos, s_nneg, TOPK_ZEROS_COMPETE, aux, sc, &s_ncand,
                                     p.out_idx + out_base, p.out_val + out_base, 0, wg_cand_idx,
                                     (long long)p.n_cols - total_nonzero);
            __syncthreads();
        }
        item_done();
    }
    if (p.phase_ticks && tid == 0) {
        const unsigned long long t_end = wall_clock64();
        atomicMax(&p.phase_ticks[9], t_end);
        atomicAdd(&p.phase_ticks[10], t_end - t_start);
    }
}

// ---------------------------------------- packed counts: two workgroups per CU ----------------------------------------
// The column kernel above keeps one workgroup per CU: a 32-bit cell per neighbour takes most of the LDS at ML-20M / Netflix shape, and a
// column's phases run one after the other -- accumulation (LDS atomics, the stream), then four latency-bound selection phases during
// which the atomic unit idles; measured in round 6, neither phase comes near a hardware limit of its own (profiles/r6_sim_phases.txt).
// Two co-resident workgroups interleave them.  They fit because, for all-ones data, a cell (c, j) never exceeds the number of users of
// column c: a column with fewer than 65 536 users needs 16 bits per cell.  This kernel packs two neighbours per LDS word -- neighbour
// j lives in half j & 1 of word j >> 1 and is incremented by 1 or 65 536 with the same 32-bit atomic; a half cannot carry into the other
// -- so an ML-20M column takes 53 KiB, two 512-thread workgroups share a CU, and the same id stream, walk lists and threshold-first
// selection serve (thread maxima over the words' two cells each, exact values of the survivors, rank, emit: bit-identical output).
// NOT handled here, by the host's choice of work items: columns with 65 536 users or more, columns that the schedule would split,
// light columns -- the 32-bit kernel runs them in a second launch, together with the columns whose threshold-first selection does
// not go through (fewer than K positive thread maxima, more survivors than the buffer holds): this kernel appends those to the
// second launch's work list (p.retry_count / p.retry_items), the accumulator is simply abandoned.
constexpr int PACKED_AUX_WORDS = 4096;          // 16 KiB: the wavefront tables (8 x 1 KiB), then histogram / candidates (2 048 x 8 B)
template <int THREADS, int G>
__global__ __launch_bounds__(THREADS, 4) void sim_packed_kernel(const SimParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned *accw = reinterpret_cast<unsigned *>(smem);                       // [acc_words] two 16-bit counts per word (+ spare words)
    uint32_t *aux = reinterpret_cast<uint32_t *>(smem) + p.acc_words;
    SimShared &shared = *reinterpret_cast<SimShared *>(aux + PACKED_AUX_WORDS);
    SelectScratch &sc = shared.sc;
    int &s_col = shared.col;
    int4 &s_item = shared.item;
    int2 &s_range = shared.range;
    uint32_t &s_ncand = shared.ncand;
    if ((unsigned)(size_t)(__attribute__((address_space(3))) float *)smem != 0u) __builtin_trap();
    const int tid = threadIdx.x, lane = tid & 63;
    const int gl = tid % G;
    constexpr int WAVES = THREADS / 64, GPW = 64 / G, DEPTH = SIM_DEPTH_UNIT;
    const int wave = tid >> 6, sub = lane / G;
    const int n_words = p.n_cols_pad / 2;                                       // words that hold neighbours (n_cols_pad is a multiple of 4)

    unsigned long long t_prev = p.phase_ticks ? wall_clock64() : 0ull;
    const unsigned long long t_start = t_prev;
    if (p.phase_ticks && tid == 0) atomicMin(&p.phase_ticks[8], t_start);
    auto mark = [&](int phase) {
        if (p.phase_ticks && tid == 0) {
            const unsigned long long now = wall_clock64();
            atomicAdd(&p.phase_ticks[phase], now - t_prev);
            t_prev = now;
        }
    };
    int nx_slot = -1;                        // thread 0 only (the next work item is pulled early, see sim_column_kernel)
    if (tid == 0) {
        const int sl = (int)atomicAdd(p.queue, 1u);
        s_col = sl;
        if (sl < p.n_items) {
            s_item = p.items[sl];
            s_range = p.item_range[sl];
        }
    }
    const __amdgpu_buffer_rsrc_t idx_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(p.seg_idx16), 0, (int)0xFFFFFFF0u, 0x00020000);
    for (;;) {
        __syncthreads();
        const int slot = s_col;
        if (slot >= p.n_items) break;
        const int4 item = s_item;
        const unsigned long long t_item = p.phase_ticks ? wall_clock64() : 0ull;
        const int c = item.x;
        const int cbeg = s_range.x, cend = s_range.y;
        int4 nx_item = make_int4(0, 0, 0, 0);
        int2 nx_range = make_int2(0, 0);
        const size_t out_base = (size_t)(p.out_slot ? p.out_slot[c] : c - p.start_col) * p.topK;

        // the wavefront's stripes of the column's walk list (serpentine over the WAVES x parts virtual wavefronts, as in sim_column_kernel)
        const int n_parts = item.z & 0xFFFF;
        const bool parts_only = (item.z >> 16) != 0;        // a column of 65 536 users or more: the 32-bit launch adds its parts up
        const int NV = WAVES * n_parts, vw = item.y * WAVES + wave;
        auto entry_of = [&](int q) {
            const int stripe = q / GPW, pos = (stripe & 1) ? NV - 1 - vw : vw;
            return cbeg + (stripe * NV + pos) * GPW + (q % GPW);
        };
        auto load_user = [&](int q, int &ex) {
            const int at = entry_of(q);
            ex = at < cend ? p.walk4[at] : -1;
        };
        auto load_bounds = [&](int ex, int &rs, int &re) {
            if (ex >= 0) {
                const uint2 e = p.walk_tab[ex];
                rs = (int)e.x;
                re = (int)e.y;
            } else {
                rs = 0;
                re = -1;
            }
        };
        int x_first, x_next, t_rs, t_re;
        load_user(lane, x_first);
        load_user(64 + lane, x_next);
        {
            uint4 *a4 = reinterpret_cast<uint4 *>(accw);
            for (int w = tid; w < p.acc_words / 4; w += THREADS) a4[w] = make_uint4(0u, 0u, 0u, 0u);
        }
        load_bounds(x_first, t_rs, t_re);
        __syncthreads();
        mark(0);

        // ---- accumulation: the lean walk of sim_column_kernel, the increment chosen by the id's lowest bit ----
        int2 *tab2 = reinterpret_cast<int2 *>(aux) + wave * 128;
        tab2[64 + lane] = make_int2(0, 0);
        for (int base = 0; entry_of(base) < cend; base += 64) {
            tab2[lane] = t_re >= 0 ? make_int2(t_rs, t_re) : make_int2(0, 0);
            load_bounds(x_next, t_rs, t_re);
            load_user(base + 128 + lane, x_next);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int g8 = 8 * gl;
            int m = sub, f_t, f_re;
            {
                const int2 e = tab2[m];
                f_t = e.x;
                f_re = e.y;
            }
            uint4 ids[DEPTH];
            bool ok[DEPTH];
            auto fetch = [&](int d) {
                const int at = f_t + g8;
                ok[d] = at < f_re;
                ids[d] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(idx_rsrc, at * 2, 0, 0));
                f_t += 8 * G;
            };
            auto add_pair = [&](unsigned w) {                 // the two ids of one stream word
                const unsigned a0 = lds_cell_address<0, 1>(w) & 0xFFFFFFFCu, a1 = lds_cell_address<1, 1>(w) & 0xFFFFFFFCu;
                lds_add_u32(a0, (w & 1u) ? 0x10000u : 1u);
                lds_add_u32(a1, (w & 0x10000u) ? 0x10000u : 1u);
            };
            auto step = [&](int d) {
                const bool done = f_t >= f_re;
                m = min(m + (done ? GPW : 0), 127);
                const int2 e = tab2[m];
                if (ok[d]) {
                    add_pair(ids[d].x);
                    add_pair(ids[d].y);
                    add_pair(ids[d].z);
                    add_pair(ids[d].w);
                }
                f_t = done ? e.x : f_t;
                f_re = done ? e.y : f_re;
                fetch(d);
            };
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {
                if (d) {
                    const bool done = f_t >= f_re;
                    m = min(m + (done ? GPW : 0), 127);
                    const int2 e = tab2[m];
                    f_t = done ? e.x : f_t;
                    f_re = done ? e.y : f_re;
                }
                fetch(d);
            }
            for (;;) {
                bool any = false;
#pragma unroll
                for (int d = 0; d < DEPTH; ++d) {
                    any |= ok[d];
                    step(d);
                }
                if (__ballot(any) == 0ull) break;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        mark(1);
        if (tid == 0) nx_slot = (int)atomicAdd(p.queue, 1u);
        if (n_parts > 1 || parts_only) {
            // Split column (see sim_column_kernel): publish the part's words; the workgroup that arrives last adds the parts up -- the sums
            // stay below 65 536 per half, the column has fewer users than that -- and carries on with the column.  (parts_only: nobody
            // here adds anything up.)
            const int pub_words = n_words;
            {
                uint4 *dst = reinterpret_cast<uint4 *>(p.part_buf + (size_t)(item.w + item.y) * p.n_cols_pad);
                const uint4 *src = reinterpret_cast<const uint4 *>(accw);
                for (int w = tid; w < pub_words / 4; w += THREADS) dst[w] = src[w];
                if (tid < (pub_words & 3)) p.part_buf[(size_t)(item.w + item.y) * p.n_cols_pad + (pub_words & ~3) + tid] = accw[(pub_words & ~3) + tid];
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                __threadfence();
                shared.last = parts_only ? 0 : (atomicAdd(&p.part_count[item.w], 1u) == (unsigned)(n_parts - 1));
                if (shared.last) __threadfence();
            }
            __syncthreads();
            if (!shared.last) {
                mark(2);
                if (tid == 0) {          // (synchronous: nothing of this item is left to hide the requests behind)
                    s_col = nx_slot;
                    if (nx_slot < p.n_items) {
                        s_item = p.items[nx_slot];
                        s_range = p.item_range[nx_slot];
                    }
                    nx_slot = -1;
                }
                continue;
            }
            const uint32_t *src = p.part_buf + (size_t)item.w * p.n_cols_pad;
            for (int w = tid; w < pub_words; w += THREADS) {
                uint32_t a = src[w];
                for (int q = 1; q < n_parts; ++q) a += src[(size_t)q * p.n_cols_pad + w];
                accw[w] = a;
            }
            __syncthreads();
            mark(2);
        }
        // the diagonal was accumulated like any other cell; the spare words absorbed the padding entries; the wavefront tables are dead:
        // zero the histogram of block_kth_largest_prefix16 and what the scans read behind the last word
        if (tid == 0) accw[c >> 1] &= (c & 1) ? 0x0000FFFFu : 0xFFFF0000u;
        for (int w = tid; w < 1024; w += THREADS) aux[w] = 0u;
        if (tid < p.acc_words - n_words) accw[n_words + tid] = 0u;
        if (tid == 0) s_ncand = 0;
        __syncthreads();

        // ---- threshold-first top-K over the words (see sim_column_kernel for the argument): thread t owns words t, t + THREADS, ... ----
        bool done = false;
        {
            const bool asym = p.normalize && p.kind == MI355REC_SIM_ASYMMETRIC;
            const float norm_c = asym ? p.norm_alpha[c] : p.norm[c];
            const float *nj = asym ? p.norm_1ma : p.norm;
            const uint32_t K = (uint32_t)p.topK;
            constexpr int CPT = (MAX_TILE / 2 + THREADS - 1) / THREADS;     // rounds of THREADS words
            constexpr int CAND_MAX = PACKED_AUX_WORDS / 2;
            constexpr int BATCH = 8;                                        // words: sixteen cells and norms
            const __amdgpu_buffer_rsrc_t nj_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(nj), 0, p.n_cols_pad * 4, 0x00020000);
            int tid_o = tid;
            asm volatile("" : "+v"(tid_o));
            const int n_rounds = (n_words + THREADS - 1) / THREADS;
            const DenomForm form = denominator_form(p, norm_c);
            const unsigned word_at = (unsigned)tid_o * 4u, word_end = (unsigned)n_words * 4u;      // byte offsets (behind the last word: a zeroed spare word)
            auto scan_words = [&](auto &&use) {
#pragma unroll
                for (int bi = 0; bi < CPT / BATCH; ++bi) {
                    const int b = bi * BATCH;
                    if (b >= n_rounds) break;
                    float2 nrm[BATCH];
#pragma unroll
                    for (int i = 0; i < BATCH; ++i)
                        nrm[i] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(nj_rsrc, tid_o * 8, (b + i) * THREADS * 8, 0));
                    unsigned wd[BATCH];
#pragma unroll
                    for (int i = 0; i < BATCH; ++i)
                        wd[i] = *reinterpret_cast<const unsigned *>(reinterpret_cast<const char *>(accw) + min(word_at + (unsigned)(b + i) * (THREADS * 4u), word_end));
#pragma unroll
                    for (int i = 0; i < BATCH; ++i) {
                        use(b + i, 0, (float)(wd[i] & 0xFFFFu), nrm[i].x);
                        use(b + i, 1, (float)(wd[i] >> 16), nrm[i].y);
                    }
                }
            };
            // (two maxima per thread -- over its words' low and high cells: the bound on the K-th largest cell comes from 2 x THREADS keys, as
            // tight as the 1024-thread kernel's: 102 survivors per ML-20M column instead of 164 with one maximum over both)
            float mx0 = 0.f, mx1 = 0.f;
            scan_words([&](int, int half, float v, float norm_j) {
                const float a = v * __builtin_amdgcn_rcpf(approx_denominator(form, v, norm_j));
                if (half) mx1 = fmaxf(mx1, a);
                else mx0 = fmaxf(mx0, a);
            });
            mark(5);
            const uint32_t p16 = block_kth_largest_prefix16<THREADS, 2>(float_key(mx0), K, aux, sc, float_key(mx1));
            mark(3);
            done = p16 > (ZERO_KEY >> 16);
            if (done) {
                if (tid == 0 && nx_slot < p.n_items) {
                    nx_item = p.items[nx_slot];
                    nx_range = p.item_range[nx_slot];
                }
                const float Tf = key_float(p16 << 16) * 0.99999809265136719f;
                uint64_t *cand = reinterpret_cast<uint64_t *>(aux);
                if (tid == 0) sc.out_count = 0;
                scan_words([&](int round, int half, float v, float norm_j) {
                    if (v > 0.f && v >= Tf * approx_denominator(form, v, norm_j)) {
                        const uint32_t at = atomicAdd(&s_ncand, 1u);
                        if (at < (uint32_t)CAND_MAX) cand[at] = ((uint64_t)__float_as_uint(norm_j) << 32) | (uint32_t)(2 * (tid_o + round * THREADS) + half);
                    }
                });
                __syncthreads();
                mark(6);
                const uint32_t n_cand = s_ncand;
                if (n_cand > (uint32_t)CAND_MAX || n_cand < K) {
                    done = false;
                } else {
                    if (p.fast_stats && tid == 0) {
                        atomicAdd(&p.fast_stats[0], 1ull);
                        atomicAdd(&p.fast_stats[1], (unsigned long long)n_cand);
                    }
                    for (uint32_t t = tid; t < n_cand; t += THREADS) {
                        const uint64_t e = cand[t];
                        const uint32_t j = (uint32_t)e;
                        const unsigned wv = accw[j >> 1];
                        const float x = normalise(p, (float)((j & 1u) ? wv >> 16 : wv & 0xFFFFu), norm_c, __uint_as_float((uint32_t)(e >> 32)));
                        cand[t] = ((uint64_t)float_key(x) << 32) | (uint32_t)(~j);
                    }
                    __syncthreads();
                    block_rank_emit<THREADS>(cand, (int)n_cand, p.topK, K, 0u, sc, p.out_idx + out_base, p.out_val + out_base);
                }
            }
        }
        if (!done) {        // the 32-bit kernel's launch takes the column over (whole, whatever path failed here)
            if (tid == 0) {
                if (nx_slot < p.n_items && nx_item.z == 0) {          // (the descriptor of the next item was not asked for yet)
                    nx_item = p.items[nx_slot];
                    nx_range = p.item_range[nx_slot];
                }
                const int k = atomicAdd(p.retry_count, 1);
                p.retry_items[k] = make_int4(c, 0, 1, 0);
                p.retry_ranges[k] = make_int2(cbeg, cend);
            }
        }
        if (tid == 0) {
            s_col = nx_slot;
            s_item = nx_item;
            s_range = nx_range;
            nx_slot = -1;
            if (p.phase_ticks) {
                const unsigned long long span = wall_clock64() - t_item;
                if (span > atomicMax(&p.phase_ticks[11], span)) p.phase_ticks[12] = (unsigned long long)c;
            }
        }
        __syncthreads();
        mark(4);
    }
    if (p.phase_ticks && tid == 0) {
        const unsigned long long t_end = wall_clock64();
        atomicMax(&p.phase_ticks[9], t_end);
        atomicAdd(&p.phase_ticks[10], t_end - t_start);
    }
}

}  // namespace
}  // namespace mi355rec
