// ials_solve.cuh -- the solve stage of a two-stage IALS epoch (ials.hip): the systems the Gramian stage (ials_kernels.cuh) left in HBM
// are factored and solved, two workgroups per CU.
#pragma once

#include "ials_kernels.cuh"

namespace mi355rec {
namespace {

// ---- the solve stage of a two-stage epoch ----------------------------------------------------------------------------------
// One 512-thread workgroup per row, TWO workgroups per CU (128 registers per lane): wavefront 0 is the PANEL wavefront -- it factors
// and inverts the diagonal tile of every panel and solves the diagonal blocks of the back substitution -- and holds no tile;
// wavefronts 1..7 hold the lower-triangle tiles (tile t on wavefront 1 + t % 7, slot t / 7: 13 slots = 104 registers at k = 200) and
// do the matrix-pipe work: panel solves and trailing updates.  The two roles run different code between the same barriers, so the
// register allocation is the larger of the two, not their sum (tiles 104 + operands; diagonal tile 64 + the inverse) -- in the
// one-kernel epoch every wavefront carries both.  While one workgroup's panel wavefront works through its 16 pivots, the other
// workgroup of the CU has the matrix pipe.  Algorithm and order of operations: those of ials_row_kernel steps (3), (4); the factors
// of a two-stage epoch agree with the one-kernel epoch's to 1e-12 (two compilations of the same expressions; the back substitution's
// LDS atomics add in arrival order in both).
// Measured and not kept (round 5): the diagonal tile with DPP row broadcasts instead of v_readlane (factor alone 103 k cycles per row
// against ~80 k; factor + inverse 559 k against 158 k), and no inverse at all -- panel tiles solved by substitution on the tile
// wavefronts (DPP), back substitution by substitution on the panel wavefront: the Cholesky took 274 k cycles per row against 267 k, the
// back substitution 60 k against 35 k; the columns of L through LDS (broadcast reads) instead of SGPRs: diagonal tiles 317 k cycles per
// row against 158 k (the panel wavefront's share of the 128 registers is small: its rows went to scratch).
template <int SLOTS>
__global__ __launch_bounds__(ROW_THREADS, 4) void ials_solve_kernel(const IalsParams p, int gram_slots, int gram_threads) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ short s_tI[MAX_NT], s_tJ[MAX_NT];
    __shared__ int s_row;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = p.k, KT = (k + 1 + 15) / 16, KP = KT * 16, NT = KT * (KT + 1) / 2;
    double *const P = lds;                                          // [KT][16][TP]  panel tiles
    double *const Ld = lds + KT * 16 * TP;                          // [KT][16][TP]  inverses of the factored diagonal tiles
    double *const zv = Ld + KT * 16 * TP + KT * 16;                 // [KP] forward-substituted rhs
    double *const xv = zv + KP;                                     // [KP] solution
    double *const acc = xv + KP;                                    // [KP] sum of L[I][J]^T x_I over the tile rows already solved
    for (int t = tid; t < NT; t += ROW_THREADS) {
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= t) ++I;
        s_tI[t] = (short)I;
        s_tJ[t] = (short)(t - I * (I + 1) / 2);
    }
    __syncthreads();
    const int Ik = k >> 4, rk = k & 15;                             // tile row and local row of the rhs row
    const size_t sys_doubles = (size_t)gram_slots * 4 * gram_threads;      // (the Gramian stage's workgroup wrote the slab)
    const int gram_waves = gram_threads / 64;
    // The two workgroups of a CU should not have their panel wavefronts on the same SIMD (both chains would share one issue port:
    // measured 120 k -> 158 k cycles of diagonal-tile work per row).  Wavefront w of a workgroup sits on SIMD w % 4 and the second
    // half of the grid is what doubles the CUs up (both observed, neither promised: a wrong guess costs speed only) -- the second
    // half takes wavefront 2 as its panel wavefront.  Tile wavefronts are numbered 0..6 in the order of the remaining indices.
    const int panel_wave = 2 * (int)(blockIdx.x >= gridDim.x / 2 && gridDim.x > 1 && !p.same_panel_wave);
    const bool is_panel = wave == panel_wave;
    const int tile_wave = wave - (wave > panel_wave);               // 0 .. 6 for the others

    for (;;) {
        __syncthreads();
        if (tid == 0) s_row = (int)atomicAdd(p.queue, 1u);
        __syncthreads();
        const int slot = s_row;
        if (slot >= p.n_local) break;
        const int row = p.items[slot].x;
        unsigned long long t2 = 0, t3 = 0;
        const bool clock = p.phases && is_panel && lane == 0;
        if (clock) t2 = ials_stamp();
        if (is_panel) {
            // ---- the panel wavefront ----
            for (int J = 0; J < KT; ++J) {
                __syncthreads();
                __syncthreads();                                     // the panel's tiles are in LDS
                unsigned long long c0 = 0;
                if (clock) c0 = ials_stamp();
                // (s_setprio 3 around it -- the chain everybody waits for first at the issue port -- changes nothing: measured)
                factor_and_invert_diagonal_tile(P, Ld + J * 16 * TP, lane);
                if (clock) { asm volatile("" ::: "memory"); atomicAdd(&p.phases[5], ials_stamp() - c0); }
                __syncthreads();
                __syncthreads();
            }
            if (clock) t3 = ials_stamp();
            __syncthreads();
            __syncthreads();
            __syncthreads();
            for (int I = KT - 1; I >= 0; --I) {                      // x_I = L_II^-T (z_I - acc_I) by substitution: lane c < 16 takes entry c
                const int c = lane & 15;
                double t = zv[16 * I + c] - acc[16 * I + c];
                if (16 * I + c >= k) t = 0.0;                        // the rhs row and the padding are not unknowns
                double x = 0.0;
#pragma unroll
                for (int m = 0; m < 16; ++m) x += Ld[(I * 16 + m) * TP + c] * lane_bcast(t, m);   // (L^-T)[c][m] = Linv[m][c]
                if (16 * I + c >= k) x = 0.0;
                if (lane < 16) xv[16 * I + c] = x;
                __syncthreads();
                __syncthreads();
            }
        } else {
            // ---- a tile wavefront ----
            int tIs[SLOTS], tJs[SLOTS];
            d4 C[SLOTS];
            {
                const double *src = p.systems + (size_t)p.sys_slot[slot] * sys_doubles;
#pragma unroll
                for (int s = 0; s < SLOTS; ++s) {
                    const int t = tile_wave + TILE_WAVES * s;
                    tIs[s] = t < NT ? __builtin_amdgcn_readfirstlane((int)s_tI[t]) : -1;
                    tJs[s] = t < NT ? __builtin_amdgcn_readfirstlane((int)s_tJ[t]) : -1;
                    // stage 1 left tile t in slot t / W of its wavefront t % W (W wavefronts)
                    const double *ts = src + (size_t)(t / gram_waves) * 4 * gram_threads + (t % gram_waves) * 64 + lane;
#pragma unroll
                    for (int i = 0; i < 4; ++i) C[s][i] = t < NT ? ts[(size_t)i * gram_threads] : 0.0;
                }
            }
            for (int J = 0; J < KT; ++J) {
                const int g = not_invariant(lane >> 4), cl = not_invariant(lane & 15);
                __syncthreads();                                     // (the previous panel is no longer read)
#pragma unroll
                for (int s = 0; s < SLOTS; ++s)
                    if (tJs[s] == J) {
                        double *tile = P + (tIs[s] - J) * 16 * TP;
#pragma unroll
                        for (int i = 0; i < 4; ++i) tile[(4 * i + g) * TP + cl] = C[s][i];
                    }
                __syncthreads();
                __syncthreads();                                     // the panel wavefront has factored the diagonal tile
#pragma unroll
                for (int s = 0; s < SLOTS; ++s) {
                    if (tJs[s] == J && tIs[s] > J) {                 // X = T L_JJ^-T on the matrix pipe: the owner's registers ARE the result
                        double *tile = P + (tIs[s] - J) * 16 * TP;
                        const double *li = Ld + J * 16 * TP;
                        d4 X = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                        for (int q = 0; q < 4; ++q) X = __builtin_amdgcn_mfma_f64_16x16x4f64(tile[cl * TP + 4 * q + g], li[cl * TP + 4 * q + g], X, 0, 0, 0);
                        C[s] = X;
                        asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");  // (the tile is rewritten below: its operand reads must have issued)
#pragma unroll
                        for (int i = 0; i < 4; ++i) tile[(4 * i + g) * TP + cl] = X[i];
                    } else if (tJs[s] == J) {                        // the diagonal tile: L_JJ
#pragma unroll
                        for (int i = 0; i < 4; ++i) C[s][i] = P[(4 * i + g) * TP + cl];
                    }
                }
                __syncthreads();
#pragma unroll
                for (int s = 0; s < SLOTS; ++s)
                    if (tJs[s] > J) {                                // trailing update: tile -= X_I X_J'^T
                        const double *xa = P + ((tIs[s] - J) * 16 + cl) * TP, *xb = P + ((tJs[s] - J) * 16 + cl) * TP;
                        double av[4], bv[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) { av[q] = -xa[4 * q + g]; bv[q] = xb[4 * q + g]; }
#pragma unroll
                        for (int q = 0; q < 4; ++q) C[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], bv[q], C[s], 0, 0, 0);
                    }
            }
            // (4) back substitution L^T x = z; z is row k of L (the forward substitution came with the factorisation)
            __syncthreads();
            for (int f = tile_wave * 64 + lane; f < KP; f += ROW_THREADS - 64) { xv[f] = 0.0; acc[f] = 0.0; zv[f] = 0.0; }
            __syncthreads();
            const int g = not_invariant(lane >> 4), cl = not_invariant(lane & 15);
#pragma unroll
            for (int s = 0; s < SLOTS; ++s)
                if (tIs[s] == Ik && g == (rk & 3)) zv[16 * tJs[s] + cl] = C[s][rk >> 2];
            __syncthreads();
            for (int I = KT - 1; I >= 0; --I) {
                __syncthreads();                                     // the panel wavefront has x_I
#pragma unroll
                for (int s = 0; s < SLOTS; ++s)
                    if (tIs[s] == I && tJs[s] < I) {                 // segment J loses L[I][J]^T x_I
                        double part = 0.0;
#pragma unroll
                        for (int i = 0; i < 4; ++i) part += C[s][i] * xv[16 * I + 4 * i + g];
                        part = swap_sum32(swap_sum16(part));
                        if (g == 0) atomicAdd(&acc[16 * tJs[s] + cl], part);
                    }
                __syncthreads();
            }
        }
        if (tid < k) p.X[(size_t)row * k + tid] = xv[tid];
        if (clock) {
            const unsigned long long t4 = ials_stamp();
            atomicAdd(&p.phases[2], t3 - t2);
            atomicAdd(&p.phases[3], t4 - t3);
        }
    }
}

}  // namespace
}  // namespace mi355rec
