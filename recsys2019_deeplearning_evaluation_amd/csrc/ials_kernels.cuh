// ials_kernels.cuh -- the device code of an IALS half-step (ials.hip), except the solve stage of a two-stage epoch (ials_solve.cuh):
// the kernels' argument block, G = Y^T Y, the row kernel (whole rows of a one-kernel epoch; the Gramian stage of a two-stage epoch)
// and the CSR -> CSC build of the create call.  The constants it shares with the host are in ials_plan.h.
#pragma once

#include "ials_diag.cuh"
#include "ials_plan.h"

namespace mi355rec {
namespace {

struct IalsParams {
    int k;
    double reg;
    const int *ptr, *idx;      // sparse rows being solved (users: C as CSR; items: C as CSC)
    const float *conf;
    const double *Y;           // fixed side factors (n_other x k)
    const double *G;           // Y^T Y (k x k)
    double *X;                 // factors being solved (n x k)
    const int4 *items;         // work items of this call, most expensive first: {row, part, n_parts, first part slot}
    int n_local;               // number of work items
    double *part_buf;          // [part slots][SLOTS * 4 * ROW_THREADS] partial augmented Gramians of split rows (accumulator layout)
    unsigned *part_count;      // arrival counters, indexed by the first part slot of a split row
    unsigned *queue;
    double *systems;           // two-stage epochs: [rows of the batch][SLOTS * 4 * ROW_THREADS] augmented systems (accumulator layout)
    const int *sys_slot;       // two-stage epochs: slab of every work item's row in `systems`
    int same_panel_wave;       // diagnostics (MI355REC_IALS_SAME_PANEL_WAVE=1): every workgroup's panel wavefront is wavefront 0
    unsigned long long *phases;   // optional (MI355REC_IALS_PHASES=1): shader-clock totals of {base, Gramian, Cholesky, back substitution}, rows
};

__device__ __forceinline__ unsigned long long ials_stamp() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

// G += Y[rows]^T Y[rows]; 256 threads as a 16 x 16 grid, thread owns G[ty + 16 (a0 + a)][tx + 16 (b0 + b)], a, b < KT16: the
// whole matrix in one launch (a0 = b0 = 0, KT16 = tiles per side; up to 14 x 14 cells = 392 registers per thread), or -- 15 and 16
// tiles per side, k > 224 -- one launch per 8 x 8 quadrant.
template <int KT16>
__global__ __launch_bounds__(256) void gram_kernel(const double *Y, int n, int k, double *G, int a0, int b0) {
    __shared__ double ys[8][256];
    const int tid = threadIdx.x, ty = tid >> 4 | a0 << 4, tx = (tid & 15) | b0 << 4;
    double acc[KT16][KT16];
#pragma unroll
    for (int a = 0; a < KT16; ++a)
#pragma unroll
        for (int b = 0; b < KT16; ++b) acc[a][b] = 0.0;
    const int rows_per_block = (n + gridDim.x - 1) / gridDim.x;
    const int r0 = blockIdx.x * rows_per_block, r1 = min(n, r0 + rows_per_block);
    for (int base = r0; base < r1; base += 8) {
        const int nr = min(8, r1 - base);
        __syncthreads();
        for (int e = tid; e < 8 * 256; e += 256) {
            const int r = e >> 8, f = e & 255;
            ys[r][f] = (r < nr && f < k) ? Y[(size_t)(base + r) * k + f] : 0.0;
        }
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            double ya[KT16], yb[KT16];
#pragma unroll
            for (int a = 0; a < KT16; ++a) {
                ya[a] = ys[r][(ty + 16 * a) & 255];        // (tiles past the 16th do not exist: masked at the end)
                yb[a] = ys[r][(tx + 16 * a) & 255];
            }
#pragma unroll
            for (int a = 0; a < KT16; ++a)
#pragma unroll
                for (int b = 0; b < KT16; ++b) acc[a][b] += ya[a] * yb[b];
        }
    }
#pragma unroll
    for (int a = 0; a < KT16; ++a)
#pragma unroll
        for (int b = 0; b < KT16; ++b) {
            const int r = ty + 16 * a, c = tx + 16 * b;
            if (r < k && c < k && r < 256 && c < 256) atomicAdd(&G[(size_t)r * k + c], acc[a][b]);
        }
}

// ---- the row solver ---------------------------------------------------------------------------------------------------------
// One 512-thread workgroup (8 wavefronts) per row.  The augmented system
//        [ B    rhs ]      B = YtY + Y_I^T (C_I - 1) Y_I + reg I,  rhs = Y_I^T c_I
//        [ rhs^T  * ]
// lives in REGISTERS as 16 x 16 tiles of its lower triangle in the accumulator layout of v_mfma_f64_16x16x4_f64 (lane l,
// element i holds row 4 i + l / 16, column l % 16; checked on the device, scripts/micro/mfma_f64.hip); tile t belongs to
// wavefront t % 8 (up to 15 tiles = 120 VGPRs per wavefront at k = 224).  Row k of the augmented matrix carries rhs, so its Cholesky row IS the forward substitution.
//   (1) tiles = G + reg I;
//   (2) Gramian: profile rows staged through LDS 16 at a time, every tile takes one MFMA per 4 profile rows
//       (A operand (c - 1) y, B operand y; the rhs row takes c instead of (c - 1) y) -- the FP64 matrix pipe, 2 LDS reads per
//       512 multiply-adds instead of 14 per 28;
//   (3) blocked right-looking Cholesky, 16-column panels: panel tiles -> LDS; the diagonal tile is factored by 16 lanes of one
//       wavefront (a row each, rows broadcast with v_readlane: no barriers inside); triangular solve of the panel, one lane per
//       row; trailing update tile -= X_I X_J^T on the matrix pipe.  4 barriers per panel (52 at k = 200) instead of one per
//       column twice over (400);
//   (4) back substitution by tile rows: x_I from the diagonal tile (16 lanes), then every tile (I, J < I) subtracts its
//       L^T x_I from segment J.
// Round 1 kept 32 x 32 register tiles on the FP64 vector pipe with one barrier per column: VALU-issue bound in the
// factorisation (2240 cycles per column: 28 multiply-adds among ~180 instructions on 16 wavefronts) and staging-latency bound
// in the Gramian (1440 cycles per profile row); measured 832 k cycles per user row at ML-20M shape, k = 200.
constexpr double AUG_DIAG = 1e200;       // diagonal of the rhs row: keeps the last pivot positive, never used

__device__ __forceinline__ double swap_sum16(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    auto lo = __builtin_amdgcn_permlane16_swap((unsigned)b, (unsigned)b, false, false);
    auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi[0] << 32) | (unsigned)lo[0]) +
           __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi[1] << 32) | (unsigned)lo[1]);
}
__device__ __forceinline__ double swap_sum32(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    auto lo = __builtin_amdgcn_permlane32_swap((unsigned)b, (unsigned)b, false, false);
    auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi[0] << 32) | (unsigned)lo[0]) +
           __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi[1] << 32) | (unsigned)lo[1]);
}

// The tile coordinates of a wavefront never change, so the compiler hoists every per-tile address computation (4 global
// addresses + 8 LDS addresses per tile) out of the row loop and then spills them: ~150 live address registers at 13 tiles.
// Passing the lane coordinates through an empty asm at the start of each phase keeps those computations where they are used.
__device__ __forceinline__ int not_invariant(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// STAGE 0: the whole row in one workgroup (Gramian, Cholesky, back substitution).
// Two-stage epochs (the default where it pays, half_step): STAGE 1 builds the augmented systems of a batch of rows and leaves them in
// HBM in the layout the MFMA accumulators have (512 consecutive doubles per store, 196 KB per row at k = 200); STAGE 2 loads them and
// solves.  The factorisation is a chain of 13 panels whose diagonal tile is factored and inverted by ONE wavefront (58 % of the
// Cholesky's cycles, measured) while the matrix pipe idles; the fused kernel holds the tiles AND the Gramian's staging in 256
// registers, one workgroup per CU, so nothing else can run meanwhile.  The solve alone fits 128 registers: two workgroups per CU, and
// one row's panel chain hides behind the other's trailing updates -- what the wide register file of a CU is for.
// THREADS: 512 for the one-kernel epoch (256 registers per lane: tiles + staging of a whole row); the Gramian stage of a two-stage epoch
// runs 1024 threads -- sixteen wavefronts with half the tiles each (6 slots at k = 200), four per SIMD instead of two: the row's
// profile is staged once, and while two wavefronts of a SIMD wait at the chunk's barriers or for their operands the other two feed the
// matrix pipe (with two per SIMD the Gramian reached 47 % of it).  (Measured and not kept: two chunks staged in LDS, chunk n + 1 written
// while chunk n is multiplied, one barrier per chunk -- 161 k cycles per user row against 99 k.)
template <int SLOTS, int STAGE, int THREADS>
__global__ __launch_bounds__(THREADS) void ials_row_kernel(const IalsParams p) {
    static_assert(STAGE == 0 || STAGE == 1, "the solve stage is ials_solve_kernel");
    static_assert(THREADS == 512 || THREADS == 1024, "CHUNK profile rows are staged by THREADS / 64 wavefronts");
    // profile rows staged per LDS round: 16; the Gramian stage (which has the LDS to itself) takes GRAM_CHUNK -- half as many barriers per row
    constexpr int CHUNK = STAGE == 1 ? GRAM_CHUNK : mi355rec::CHUNK;
    constexpr int WAVES = THREADS / 64, RPW = CHUNK / WAVES;      // profile rows a wavefront stages per chunk
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ short s_tI[MAX_NT], s_tJ[MAX_NT];
    __shared__ int s_row;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = p.k, KT = (k + 1 + 15) / 16, KP = KT * 16, NT = KT * (KT + 1) / 2;
    double *const ya = lds;                                         // [CHUNK][KP]   A side: (c - 1) y, c in column k
    double *const yb = ya + CHUNK * KP;                             // [CHUNK][KP]   B side: y
    double *const P = lds;                                          // [KT][16][TP]  panel tiles (aliases the staging area)
    double *const Linv = lds + (STAGE == 1 ? 2 * GRAM_CHUNK * KP : max(2 * CHUNK * KP, KT * 16 * TP));   // [KT][16][TP]  inverses of the factored diagonal tiles
    double *const zv = Linv + KT * 16 * TP + KT * 16;               // [KP] forward-substituted rhs
    double *const xv = zv + KP;                                     // [KP] solution
    double *const acc = xv + KP;                                    // [KP] sum of L[I][J]^T x_I over the tile rows already solved

    for (int t = tid; t < NT; t += THREADS) {                   // tile t = I (I + 1) / 2 + J of the lower triangle
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= t) ++I;
        s_tI[t] = (short)I;
        s_tJ[t] = (short)(t - I * (I + 1) / 2);
    }
    __syncthreads();
    int tIs[SLOTS], tJs[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const int t = wave + WAVES * s;
        tIs[s] = t < NT ? __builtin_amdgcn_readfirstlane((int)s_tI[t]) : -1;
        tJs[s] = t < NT ? __builtin_amdgcn_readfirstlane((int)s_tJ[t]) : -1;
    }
    const int Ik = k >> 4, rk = k & 15;                             // tile row and local row of the rhs row
    // staging roles: wavefront w fetches profile rows RPW w .. RPW w + RPW - 1 of a chunk, lanes across the factors (4 x 64 >= 224 + 1)
    constexpr int SPL = 4;

    for (;;) {
        __syncthreads();
        if (tid == 0) s_row = (int)atomicAdd(p.queue, 1u);
        __syncthreads();
        const int slot = s_row;
        if (slot >= p.n_local) break;
        const int4 item = p.items[slot];
        const int row = item.x;
        int beg = p.ptr[row], end = p.ptr[row + 1];
        // A row whose Gramian alone would keep one workgroup busy for a large share of the call -- the most popular item at ML-20M
        // shape: 10^5 profile rows x k^2 on ONE CU = 26 ms, every partition of the item half-step waits for it -- is split: part q of
        // n accumulates the profile rows [beg, end) below into its own tiles (part 0 starts from YtY + reg I, the others from zero),
        // publishes them, and the part that arrives last adds the parts up IN PART ORDER (the result does not depend on who is
        // last) and solves.  Nobody waits for anybody.
        if (item.z > 1) {
            const PartRange mine = part_range(beg, end, item.y, item.z, CHUNK);
            beg = mine.beg;
            end = mine.end;
        }
        const bool first_part = item.y == 0;
        unsigned long long t0 = 0, t1 = 0, t2 = 0, t3 = 0;
        if (p.phases && tid == 0) t0 = ials_stamp();

        // (2a) the first chunk of profile rows is requested before anything else; item ids and confidences run one chunk
        // further ahead than the factor rows they address (two dependent global round trips otherwise)
        constexpr size_t SYS_DOUBLES = (size_t)SLOTS * 4 * THREADS;
        d4 C[SLOTS];
        double pre[RPW][SPL];
        double pre_c[RPW], next_c[RPW];
        int next_item[RPW];
        auto fetch_ids = [&](int base) {
#pragma unroll
            for (int h = 0; h < RPW; ++h) {
                const int r = base + RPW * wave + h;
                next_item[h] = r < end ? p.idx[r] : -1;
                next_c[h] = r < end ? (double)p.conf[r] : 0.0;
            }
        };
        auto fetch_rows = [&]() {                                    // rows of the ids fetched last
#pragma unroll
            for (int h = 0; h < RPW; ++h) {
                const bool ok = next_item[h] >= 0;
                pre_c[h] = next_c[h];
                const double *src = p.Y + (size_t)(ok ? next_item[h] : 0) * k;
#pragma unroll
                for (int q = 0; q < SPL; ++q) {
                    const int f = lane + 64 * q;
                    pre[h][q] = ok && f < k ? src[f] : 0.0;
                }
            }
        };
        fetch_ids(beg);
        fetch_rows();
        fetch_ids(beg + CHUNK);

        // (1) B = YtY + reg I                                      (IALSRecommender.py:199)
        // Every lane's 4 x SLOTS cells of G are requested first, unconditionally (clamped addresses), and patched afterwards: with the
        // load inside the `r < k && c < k` test every cell waited for its own round trip to the L2 (37 k cycles per row, a quarter
        // of the Gramian stage).
        {
        const int g = not_invariant(lane >> 4), cl = not_invariant(lane & 15);
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const int tI = max(tIs[s], 0), tJ = max(tJs[s], 0);
#pragma unroll
            for (int i = 0; i < 4; ++i) C[s][i] = p.G[(size_t)min(16 * tI + 4 * i + g, k - 1) * k + min(16 * tJ + cl, k - 1)];
            // (one kernel: four tiles' loads in flight at a time -- its registers are full; the Gramian stage of a two-stage epoch
            // requests all of them at once)
            if (STAGE == 0 && (s & 3) == 3) asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = 16 * tIs[s] + 4 * i + g, c = 16 * tJs[s] + cl;
                double v = C[s][i];
                if (r == c) v += p.reg;
                if (r >= k || c >= k) v = r == c ? (r == k ? AUG_DIAG : 1.0) : 0.0;   // identity padding keeps the factorisation well defined
                if (tIs[s] < 0 || !first_part) v = 0.0;
                C[s][i] = v;
            }
        }
        }
        if (p.phases && tid == 0) { asm volatile("" ::"v"(C[0][0])); t1 = ials_stamp(); }

        // (2) A = Y_I^T ((c - 1) o Y_I), rhs = Y_I^T c             (:197, :201): the matrix pipe works on chunk n while the
        // loads of chunk n + 1 are in flight
        for (int base = beg; base < end; base += CHUNK) {
            const int nr = min(CHUNK, end - base);
            __syncthreads();                                         // the previous chunk has been consumed
#pragma unroll
            for (int h = 0; h < RPW; ++h) {
                const int r = RPW * wave + h;
                const double c = pre_c[h];
#pragma unroll
                for (int q = 0; q < SPL; ++q) {
                    const int f = lane + 64 * q;
                    if (f < KP) {
                        const double y = pre[h][q];
                        ya[r * KP + f] = f == k ? c : y * (c - 1.0);     // (y is 0 beyond k and for rows past the profile)
                        yb[r * KP + f] = y;
                    }
                }
            }
            if (base + CHUNK < end) {
                fetch_rows();
                fetch_ids(base + 2 * CHUNK);
            }
            __syncthreads();
            const int groups = (nr + 3) >> 2;
            const int g = not_invariant(lane >> 4), cl = not_invariant(lane & 15);
            // all operand reads of a group of 4 profile rows first, then the MFMAs (no branch between them: a wavefront with
            // fewer tiles than slots runs its spare slot on tile (0, 0) and never looks at the result) -- otherwise every MFMA
            // waits for its own two LDS reads (117 instead of 32 cycles per MFMA, measured)
            for (int q = 0; q < groups; ++q) {
                const double *ar = ya + (4 * q + g) * KP + cl, *br = yb + (4 * q + g) * KP + cl;
                double av[SLOTS], bv[SLOTS];
#pragma unroll
                for (int s = 0; s < SLOTS; ++s) {
                    av[s] = ar[16 * max(tIs[s], 0)];
                    bv[s] = br[16 * max(tJs[s], 0)];
                }
#pragma unroll
                for (int s = 0; s < SLOTS; ++s) C[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[s], C[s], 0, 0, 0);
            }
        }
        if (item.z > 1) {
            constexpr size_t PART_DOUBLES = (size_t)SLOTS * 4 * THREADS;
            {
                double *dst = p.part_buf + (size_t)(item.w + item.y) * PART_DOUBLES;
#pragma unroll
                for (int s = 0; s < SLOTS; ++s)
#pragma unroll
                    for (int i = 0; i < 4; ++i) dst[(size_t)(s * 4 + i) * THREADS + tid] = C[s][i];
            }
            // every wavefront waits for its own stores; ONE thread then makes them visible device-wide (agent-scope release) and
            // counts the arrival; the last arriver acquires on behalf of the workgroup (same protocol as the similarity kernel's
            // split columns)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                __threadfence();
                const bool last = atomicAdd(&p.part_count[item.w], 1u) == (unsigned)(item.z - 1);
                if (last) __threadfence();
                s_row = last ? 1 : 0;
            }
            __syncthreads();
            const bool last = s_row != 0;
            if (!last) continue;
            const double *src = p.part_buf + (size_t)item.w * PART_DOUBLES;
#pragma unroll
            for (int s = 0; s < SLOTS; ++s)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    double v = 0.0;
                    for (int q = 0; q < item.z; ++q) v += src[(size_t)q * PART_DOUBLES + (size_t)(s * 4 + i) * THREADS + tid];
                    C[s][i] = v;
                }
        }
        if (p.phases && tid == 0) { asm volatile("" ::"v"(C[0][0])); t2 = ials_stamp(); }
        if (STAGE == 1) {                                            // hand the system to the solve stage
            double *dst = p.systems + (size_t)p.sys_slot[slot] * SYS_DOUBLES;
#pragma unroll
            for (int s = 0; s < SLOTS; ++s)
#pragma unroll
                for (int i = 0; i < 4; ++i) dst[(size_t)(s * 4 + i) * THREADS + tid] = C[s][i];
            if (p.phases && tid == 0) {
                atomicAdd(&p.phases[0], t1 - t0);
                atomicAdd(&p.phases[1], t2 - t1);
                atomicAdd(&p.phases[4], 1ull);
            }
            continue;
        }

        // (3) blocked Cholesky of the augmented matrix, panel J = columns 16 J .. 16 J + 15
        for (int J = 0; J < KT; ++J) {
            const int g = not_invariant(lane >> 4), cl = not_invariant(lane & 15);
            __syncthreads();                                         // (the staging area / the previous panel is no longer read)
#pragma unroll
            for (int s = 0; s < SLOTS; ++s)
                if (tJs[s] == J) {
                    double *tile = P + (tIs[s] - J) * 16 * TP;
#pragma unroll
                    for (int i = 0; i < 4; ++i) tile[(4 * i + g) * TP + cl] = C[s][i];
                }
            __syncthreads();
            unsigned long long c0 = 0, c1 = 0, c2 = 0;
            if (p.phases && tid == 0) c0 = ials_stamp();
            if (wave == 0) factor_and_invert_diagonal_tile(P, Linv + J * 16 * TP, lane);
            if (p.phases && tid == 0) { asm volatile("" ::: "memory"); c1 = ials_stamp(); }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                if (tJs[s] == J && tIs[s] > J) {                     // X = T L_JJ^-T on the matrix pipe: the owner's registers ARE the result
                    double *tile = P + (tIs[s] - J) * 16 * TP;
                    const double *li = Linv + J * 16 * TP;
                    d4 X = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int q = 0; q < 4; ++q) X = __builtin_amdgcn_mfma_f64_16x16x4f64(tile[cl * TP + 4 * q + g], li[cl * TP + 4 * q + g], X, 0, 0, 0);
                    C[s] = X;
                    asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");  // (the tile is rewritten below: its operand reads must have issued)
#pragma unroll
                    for (int i = 0; i < 4; ++i) tile[(4 * i + g) * TP + cl] = X[i];
                } else if (tJs[s] == J) {                            // the diagonal tile: L_JJ
#pragma unroll
                    for (int i = 0; i < 4; ++i) C[s][i] = P[(4 * i + g) * TP + cl];
                }
            }
            __syncthreads();
            if (p.phases && tid == 0) c2 = ials_stamp();
#pragma unroll
            for (int s = 0; s < SLOTS; ++s)
                if (tJs[s] > J) {                                    // trailing update: tile -= X_I X_J'^T
                    const double *xa = P + ((tIs[s] - J) * 16 + cl) * TP, *xb = P + ((tJs[s] - J) * 16 + cl) * TP;
                    double av[4], bv[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { av[q] = -xa[4 * q + g]; bv[q] = xb[4 * q + g]; }
#pragma unroll
                    for (int q = 0; q < 4; ++q) C[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], bv[q], C[s], 0, 0, 0);
                }
            if (p.phases && tid == 0) {
                asm volatile("" ::"v"(C[0][0]));
                const unsigned long long c3 = ials_stamp();
                atomicAdd(&p.phases[5], c1 - c0);
                atomicAdd(&p.phases[6], c2 - c1);
                atomicAdd(&p.phases[7], c3 - c2);
            }
        }
        if (p.phases && tid == 0) { asm volatile("" ::"v"(C[0][0])); t3 = ials_stamp(); }

        // (4) back substitution L^T x = z; z is row k of L (the forward substitution came with the factorisation)
        __syncthreads();
        for (int f = tid; f < KP; f += THREADS) { xv[f] = 0.0; acc[f] = 0.0; zv[f] = 0.0; }
        __syncthreads();
        const int g = not_invariant(lane >> 4), cl = not_invariant(lane & 15);
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
            if (tIs[s] == Ik && g == (rk & 3)) zv[16 * tJs[s] + cl] = C[s][rk >> 2];
        __syncthreads();
        for (int I = KT - 1; I >= 0; --I) {
            if (wave == 0) {                                         // x_I = L_II^-T (z_I - acc_I): lane c < 16 takes entry c
                const int c = lane & 15;
                double t = zv[16 * I + c] - acc[16 * I + c];
                if (16 * I + c >= k) t = 0.0;                        // the rhs row and the padding are not unknowns
                double x = 0.0;
#pragma unroll
                for (int m = 0; m < 16; ++m) x += Linv[(I * 16 + m) * TP + c] * lane_bcast(t, m);   // (L^-T)[c][m] = Linv[m][c]
                if (16 * I + c >= k) x = 0.0;
                if (lane < 16) xv[16 * I + c] = x;
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < SLOTS; ++s)
                if (tIs[s] == I && tJs[s] < I) {                     // segment J loses L[I][J]^T x_I
                    double part = 0.0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) part += C[s][i] * xv[16 * I + 4 * i + g];
                    part = swap_sum32(swap_sum16(part));
                    if (g == 0) atomicAdd(&acc[16 * tJs[s] + cl], part);
                }
            __syncthreads();
        }
        if (tid < k) p.X[(size_t)row * k + tid] = xv[tid];
        if (p.phases && tid == 0) {
            const unsigned long long t4 = ials_stamp();
            atomicAdd(&p.phases[0], t1 - t0);
            atomicAdd(&p.phases[1], t2 - t1);
            atomicAdd(&p.phases[4], 1ull);
            atomicAdd(&p.phases[2], t3 - t2);
            atomicAdd(&p.phases[3], t4 - t3);
        }
    }
}

// CSR -> CSC of the confidence matrix on the device (row ids inside a column end up unordered: irrelevant here,
// the Gramian is a sum).
__global__ void ials_count_kernel(const int *idx, size_t nnz, int *cnt) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nnz; i += (size_t)gridDim.x * blockDim.x)
        atomicAdd(&cnt[idx[i]], 1);
}
__global__ __launch_bounds__(1024) void ials_scan_kernel(const int *cnt, int *out, int *cursor, int n) {
    __shared__ long long part[1024];
    const int tid = threadIdx.x;
    const int chunk = (n + 1023) / 1024;
    const int b = tid * chunk, e = min(n, b + chunk);
    long long s = 0;
    for (int i = b; i < e; ++i) s += cnt[i];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        long long t = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += t;
        __syncthreads();
    }
    long long run = tid ? part[tid - 1] : 0;
    for (int i = b; i < e; ++i) {
        out[i] = (int)run;
        cursor[i] = (int)run;
        run += cnt[i];
    }
    if (tid == 1023) out[n] = (int)part[1023];
}
__global__ void ials_scatter_kernel(const int *ptr, const int *idx, const float *val, int n_rows, int *cursor, int *t_idx,
                                    float *t_val) {
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= n_rows) return;
    for (int q = ptr[wave] + lane; q < ptr[wave + 1]; q += 64) {
        const int pos = atomicAdd(&cursor[idx[q]], 1);
        t_idx[pos] = wave;
        t_val[pos] = val[q];
    }
}

}  // namespace
}  // namespace mi355rec
