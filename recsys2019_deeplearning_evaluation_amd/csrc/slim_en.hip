// slim_en.hip -- SLIM ElasticNet (SLIM_ElasticNet/SLIMElasticNetRecommender.py:41-149) on MI355X (gfx950).
//
// The reference fits one sklearn ElasticNet per item (sparse coordinate descent, _cd_fast.pyx sparse_enet_coordinate_descent,
// fit_intercept=False, selection='random').  In exact arithmetic that solver is coordinate descent on the Gram matrix G = X^T X,
// one matrix shared by every target: with H = G w, q = G[:, j] and d = diag G (d_j := 0 for the target j),
//     t = q_ii - H_ii + d_ii w_ii,   w_ii <- 0 if (positive && t < 0) else sign(t) max(|t| - l1, 0) / (d_ii + l2),
//     H += (w_new - w_old) G[:, ii]   when w_ii changed.
// The coordinate of every draw is sklearn's xorshift (our_rand_r, sklearn/utils/_random.pxd) seeded per target; a sweep is
// n_items draws, skipped coordinates (d == 0) still consume theirs.  The duality-gap stop test (_cd_fast.pyx:499-546) runs in fp64.
//
// Kernels
//   slimen_diag_kernel   d_k = sum_u X_uk^2 in the column's stored order (the reference's norm_cols_X, fp32);
//   slimen_gram_kernel   G row by row, one workgroup per item: sum over the users of item j of x_uj * X[u, :], accumulated in LDS
//                        (float atomics: exact for integer / quantised values) or, beyond the LDS or with
//                        MI355REC_SLIMEN_GLOBAL_GRAM=1, in the row of G itself;
//   slimen_fit_kernel    a persistent grid, one target per workgroup, targets taken from a queue word by a vector atomic.  H lives in
//                        LDS (H_LDS) or in a per-workgroup global slot; w lives in a per-workgroup global slot behind a nonzero
//                        bitmask in LDS (w is read only where the bit is set, so a slot is never cleared).
//
// Exact speculative windows: between two changes of w, H is constant, so the next WINDOW = 512 draws of the sequence can all be
// evaluated against the same H at once.  Every lane derives its own xorshift state by jump tables (the generator is linear over
// GF(2): state after n steps = XOR of the images of the set bits), the block finds the first draw whose value changes, accepts every
// draw up to and including it, applies that one H update and resumes at the next draw.  Runs of unchanged coordinates (the zeros
// that stay zero) cost one step of the block instead of 512 serial steps; the result is the serial sequence's.
//
// After the fit each workgroup selects the target's coefficients: local_topK = min(nnz - 1, topK) largest by value
// (SLIMElasticNetRecommender.py:107-111), ties at the cut towards the lower index, by a 4 x 8-bit radix select over the set bits.
#include "common.h"
#include "topk.cuh"

#include <algorithm>
#include <cstdlib>
#include <memory>

using namespace mi355rec;

namespace {

constexpr int THREADS = 512;
constexpr int WAVES = THREADS / 64;
constexpr int WINDOW = THREADS;                 // draws evaluated per block step
constexpr int GRAM_THREADS = 512;
constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr size_t FIT_STATIC_LDS = 16 * 1024;    // FitShared: jump tables, broadcast words, reduction scratch, histogram

__host__ __device__ inline uint32_t xorshift_step(uint32_t s) {
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return s;
}

// ------------------------------------------------------------------------------------------------------------------------------
__global__ void slimen_diag_kernel(const int *col_ptr, const float *col_val, int n_items, float *diag) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_items) return;
    float s = 0.f;
    for (int p = col_ptr[k]; p < col_ptr[k + 1]; ++p) s += col_val[p] * col_val[p];
    diag[k] = s;
}

template <bool LDS_ACC>
__global__ __launch_bounds__(GRAM_THREADS) void slimen_gram_kernel(const int *row_ptr, const int *row_idx, const float *row_val,
                                                                   const int *col_ptr, const int *col_idx, const float *col_val,
                                                                   int n_items, float *G) {
    extern __shared__ __attribute__((aligned(16))) float acc[];
    const int j = blockIdx.x;
    float *Gj = G + (size_t)j * n_items;
    if (LDS_ACC) {
        for (int k = threadIdx.x; k < n_items; k += GRAM_THREADS) acc[k] = 0.f;
        __syncthreads();
    }
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    for (int p = col_ptr[j] + wave; p < col_ptr[j + 1]; p += GRAM_THREADS / 64) {
        const int u = col_idx[p];
        const float xj = col_val[p];
        for (int e = row_ptr[u] + lane; e < row_ptr[u + 1]; e += 64) {
            if (LDS_ACC) atomicAdd(&acc[row_idx[e]], xj * row_val[e]);
            else atomicAdd(&Gj[row_idx[e]], xj * row_val[e]);
        }
    }
    if (LDS_ACC) {
        __syncthreads();
        for (int k = threadIdx.x; k < n_items; k += GRAM_THREADS) Gj[k] = acc[k];
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
struct FitArgs {
    const float *G, *diag;
    const uint32_t *seeds;          // per target of the range (0 already replaced by 1)
    const uint32_t *jump;           // [32 x 64] lane table (bit b, lane l: e_b advanced l + 1 steps), then [8 x 32] wave table (64 w steps)
    float *w_slots, *h_slots;       // per workgroup, n_items each (h_slots: global-H instance only)
    unsigned *queue;                // next target (offset in the range)
    int n_items, start, n_targets, max_iter, positive, topK, slots_per_target;
    float l1, l2, tol;
    int *out_idx;                   // [n_targets x slots_per_target]
    float *out_val;
    int *out_n, *out_iter, *out_conv;
    unsigned long long *counters;   // accepted changes, sweeps, block steps, gap tests
};

struct FitShared {
    uint32_t jl[32 * 64];
    uint32_t jw[WAVES * 32];
    uint32_t state;                 // xorshift state before the next draw
    int pos, it, stop, change_ii, target;
    float w_max, d_w_max, delta;
    int first[WAVES];               // per wave: first changing lane (64: none)
    float wmax_w[WAVES], dmax_w[WAVES];
    double red[WAVES][5];
    unsigned hist[256];
    unsigned sel_prefix;
    int sel_need, sel_out;
    int tie_base[THREADS];
};

__device__ __forceinline__ float wave_prefix_max(float v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_up(v, o, 64);
        if (lane >= o) v = fmaxf(v, u);
    }
    return v;
}

template <class T> __device__ __forceinline__ T wave_reduce_sum(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_reduce_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

template <bool H_LDS>
__global__ __launch_bounds__(THREADS) void slimen_fit_kernel(FitArgs a) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    __shared__ FitShared sh;
    const int N = a.n_items;
    const int nmask = (N + 31) / 32;
    uint32_t *mask = reinterpret_cast<uint32_t *>(dyn);                  // nonzero bits of w
    float *H = H_LDS ? dyn + nmask : a.h_slots + (size_t)blockIdx.x * N;
    float *w = a.w_slots + (size_t)blockIdx.x * N;
    const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64;

    for (int i = tid; i < 32 * 64; i += THREADS) sh.jl[i] = a.jump[i];
    for (int i = tid; i < WAVES * 32; i += THREADS) sh.jw[i] = a.jump[32 * 64 + i];

    unsigned long long n_changes = 0, n_sweeps = 0, n_steps = 0, n_tests = 0;
    for (;;) {
        __syncthreads();
        if (tid == 0) sh.target = (int)atomicAdd(a.queue, 1u);
        __syncthreads();
        const int t_off = sh.target;
        if (t_off >= a.n_targets) break;
        const int j = a.start + t_off;
        const float *q = a.G + (size_t)j * N;                            // G symmetric: row j = column j
        const float yy = a.diag[j];
        const float tolj = a.tol * yy;

        for (int i = tid; i < nmask; i += THREADS) mask[i] = 0u;
        for (int i = tid; i < N; i += THREADS) H[i] = 0.f;
        if (tid == 0) {
            sh.state = a.seeds[t_off];
            sh.pos = 0;
            sh.it = 0;
            sh.stop = 0;
            sh.w_max = 0.f;
            sh.d_w_max = 0.f;
        }
        int converged = 0, n_iter = a.max_iter;
        if (yy == 0.f) {                   // an empty target: the reference idles through max_iter sweeps, w stays 0
            __syncthreads();
        } else {
            __syncthreads();
            for (;;) {
                // ---- one block step: WINDOW draws against the same H
                const uint32_t s0 = sh.state;
                const int pos = sh.pos;
                uint32_t base = s0;
                if (wave) {
                    base = 0u;
                    for (int b = 0; b < 32; ++b)
                        if ((s0 >> b) & 1u) base ^= sh.jw[wave * 32 + b];
                }
                uint32_t s = 0u;
                for (int b = 0; b < 32; ++b)
                    if ((base >> b) & 1u) s ^= sh.jl[b * 64 + lane];
                const bool valid = pos + tid < N;
                int ii = 0;
                bool counted = false, changed = false;
                float wnew = 0.f, wold = 0.f;
                if (valid) {
                    ii = (int)((s & 0x7FFFFFFFu) % (uint32_t)N);
                    const float d = ii == j ? 0.f : a.diag[ii];
                    if (d != 0.f) {
                        counted = true;
                        wold = (mask[ii >> 5] >> (ii & 31)) & 1u ? w[ii] : 0.f;
                        const float t = (q[ii] - H[ii]) + d * wold;
                        if (a.positive && t < 0.f) wnew = 0.f;
                        else wnew = copysignf(fmaxf(fabsf(t) - a.l1, 0.f), t) / (d + a.l2);
                        changed = wnew != wold;
                    }
                }
                const unsigned long long bal = __ballot(changed);
                const float pm = wave_prefix_max(counted ? fabsf(wnew) : 0.f, lane);
                const float pd = wave_prefix_max(counted ? fabsf(wnew - wold) : 0.f, lane);
                if (lane == 63) {
                    sh.first[wave] = bal ? (int)__builtin_ctzll(bal) : 64;
                    sh.wmax_w[wave] = pm;
                    sh.dmax_w[wave] = pd;
                }
                __syncthreads();
                int f = WINDOW;
                for (int v = 0; v < WAVES; ++v)
                    if (sh.first[v] < 64) {
                        f = v * 64 + sh.first[v];
                        break;
                    }
                const int accepted = f < WINDOW ? f + 1 : min(WINDOW, N - pos);
                if (tid == accepted - 1) {         // the last accepted draw carries the sequence on
                    float wm = sh.w_max, dm = sh.d_w_max;
                    for (int v = 0; v < wave; ++v) {
                        wm = fmaxf(wm, sh.wmax_w[v]);
                        dm = fmaxf(dm, sh.dmax_w[v]);
                    }
                    sh.w_max = fmaxf(wm, pm);
                    sh.d_w_max = fmaxf(dm, pd);
                    sh.state = s;
                    sh.pos = pos + accepted;
                    sh.change_ii = changed ? ii : -1;
                    if (changed) {
                        sh.delta = wnew - wold;
                        w[ii] = wnew;
                        const uint32_t bit = 1u << (ii & 31);
                        mask[ii >> 5] = wnew != 0.f ? (mask[ii >> 5] | bit) : (mask[ii >> 5] & ~bit);
                    }
                }
                __syncthreads();
                ++n_steps;
                const int cii = sh.change_ii;
                if (cii >= 0) {
                    ++n_changes;
                    const float delta = sh.delta;
                    const float *g = a.G + (size_t)cii * N;
                    for (int k = tid; k < N; k += THREADS) H[k] += delta * g[k];
                    __syncthreads();
                }
                if (sh.pos < N) continue;

                // ---- end of a sweep (_cd_fast.pyx:499-546)
                ++n_sweeps;
                const int it = sh.it;
                const float wmx = sh.w_max, dwm = sh.d_w_max;
                bool stop = false;
                if (wmx == 0.f || dwm / wmx < a.tol || it == a.max_iter - 1) {
                    ++n_tests;
                    double xta_max = 0.0, wq = 0.0, wh = 0.0, l1n = 0.0, ww = 0.0;   // XtA_j = 0 takes part in the max (or max |.|)
                    for (int k = tid; k < N; k += THREADS) {
                        const double wk = (mask[k >> 5] >> (k & 31)) & 1u ? (double)w[k] : 0.0;
                        const double hk = H[k], qk = q[k];
                        if (k != j) {
                            const double x = qk - hk - (double)a.l2 * wk;
                            xta_max = fmax(xta_max, a.positive ? x : fabs(x));
                        }
                        if (wk != 0.0) {
                            wq += wk * qk;
                            wh += wk * hk;
                            l1n += fabs(wk);
                            ww += wk * wk;
                        }
                    }
                    xta_max = wave_reduce_max(xta_max);
                    wq = wave_reduce_sum(wq);
                    wh = wave_reduce_sum(wh);
                    l1n = wave_reduce_sum(l1n);
                    ww = wave_reduce_sum(ww);
                    if (lane == 0) {
                        sh.red[wave][0] = xta_max;
                        sh.red[wave][1] = wq;
                        sh.red[wave][2] = wh;
                        sh.red[wave][3] = l1n;
                        sh.red[wave][4] = ww;
                    }
                    __syncthreads();
                    double dual = 0.0, WQ = 0.0, WH = 0.0, L1 = 0.0, WW = 0.0;
                    for (int v = 0; v < WAVES; ++v) {
                        dual = fmax(dual, sh.red[v][0]);
                        WQ += sh.red[v][1];
                        WH += sh.red[v][2];
                        L1 += sh.red[v][3];
                        WW += sh.red[v][4];
                    }
                    const double l1 = a.l1, l2 = a.l2, Y = yy;
                    const double Rn = Y - 2.0 * WQ + WH;
                    double c, gap;
                    if (dual > l1) {
                        c = l1 / dual;
                        gap = 0.5 * Rn * (1.0 + c * c);
                    } else {
                        c = 1.0;
                        gap = Rn;
                    }
                    gap += l1 * L1 - c * (Y - WQ) + 0.5 * l2 * (1.0 + c * c) * WW;
                    if (gap < (double)tolj) {
                        stop = true;
                        converged = 1;
                    }
                }
                n_iter = it + 1;
                if (it + 1 >= a.max_iter) stop = true;
                __syncthreads();
                if (tid == 0) {
                    sh.it = it + 1;
                    sh.pos = 0;
                    sh.w_max = 0.f;
                    sh.d_w_max = 0.f;
                }
                __syncthreads();
                if (stop) break;
            }
        }

        // ---- selection: local_topK = min(nnz - 1, topK) largest values, ties towards the lower index
        int nnz = 0;
        for (int i = tid; i < nmask; i += THREADS) nnz += __popc(mask[i]);
        nnz = wave_reduce_sum(nnz);
        if (lane == 0) sh.red[wave][0] = (double)nnz;
        __syncthreads();
        nnz = 0;
        for (int v = 0; v < WAVES; ++v) nnz += (int)sh.red[v][0];
        const int K = a.topK < 0 ? nnz : min(nnz - 1, a.topK);            // topK = -1: every nonzero (diagnostics)
        int *oi = a.out_idx + (size_t)t_off * a.slots_per_target;
        float *ov = a.out_val + (size_t)t_off * a.slots_per_target;
        if (K > 0) {
            // K-th largest key among the set bits, 8 bits at a time
            uint32_t prefix = 0u;
            int need = K;                  // rank still to find inside the current prefix
            for (int shift = 24; shift >= 0; shift -= 8) {
                for (int i = tid; i < 256; i += THREADS) sh.hist[i] = 0u;
                __syncthreads();
                const uint32_t hi_mask = shift == 24 ? 0u : (0xFFFFFFFFu << (shift + 8));
                for (int k = tid; k < N; k += THREADS) {
                    if (!((mask[k >> 5] >> (k & 31)) & 1u)) continue;
                    const uint32_t key = float_key(w[k]);
                    if ((key & hi_mask) == prefix) atomicAdd(&sh.hist[(key >> shift) & 255u], 1u);
                }
                __syncthreads();
                if (tid == 0) {
                    int above = 0, bin = 255;
                    for (; bin > 0; --bin) {
                        if (above + (int)sh.hist[bin] >= need) break;
                        above += (int)sh.hist[bin];
                    }
                    sh.sel_prefix = prefix | ((uint32_t)bin << shift);
                    sh.sel_need = need - above;
                }
                __syncthreads();
                prefix = sh.sel_prefix;
                need = sh.sel_need;
                __syncthreads();
            }
            // keys above the cut: all of them; keys equal to it: the `need` lowest indices.  Every thread owns a contiguous range.
            const int per = (N + THREADS - 1) / THREADS;
            const int k0 = min(N, tid * per), k1 = min(N, k0 + per);
            int ties = 0;
            for (int k = k0; k < k1; ++k)
                if (((mask[k >> 5] >> (k & 31)) & 1u) && float_key(w[k]) == prefix) ++ties;
            sh.tie_base[tid] = ties;
            if (tid == 0) sh.sel_out = 0;
            __syncthreads();
            if (tid == 0) {
                int run = 0;
                for (int v = 0; v < THREADS; ++v) {
                    const int c = sh.tie_base[v];
                    sh.tie_base[v] = run;
                    run += c;
                }
            }
            __syncthreads();
            int tie_rank = sh.tie_base[tid];
            for (int k = k0; k < k1; ++k) {
                if (!((mask[k >> 5] >> (k & 31)) & 1u)) continue;
                const float v = w[k];
                const uint32_t key = float_key(v);
                bool keep = key > prefix;
                if (key == prefix) keep = tie_rank++ < need;
                if (keep) {
                    const int slot = (int)atomicAdd((unsigned *)&sh.sel_out, 1u);
                    oi[slot] = k;
                    ov[slot] = v;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            a.out_n[t_off] = max(K, 0);
            a.out_iter[t_off] = n_iter;
            a.out_conv[t_off] = converged;
        }
    }
    if (tid == 0) {
        atomicAdd(&a.counters[0], n_changes);
        atomicAdd(&a.counters[1], n_sweeps);
        atomicAdd(&a.counters[2], n_steps);
        atomicAdd(&a.counters[3], n_tests);
    }
}

// Jump tables of the generator: lane table [bit b][lane l] = e_b advanced l + 1 steps, wave table [wave v][bit b] = e_b advanced 64 v steps.
std::vector<uint32_t> jump_tables() {
    std::vector<uint32_t> t(32 * 64 + WAVES * 32);
    for (int b = 0; b < 32; ++b) {
        uint32_t s = 1u << b;
        for (int l = 0; l < 64; ++l) {
            s = xorshift_step(s);
            t[b * 64 + l] = s;
        }
        uint32_t r = 1u << b;
        for (int v = 0; v < WAVES; ++v) {
            t[32 * 64 + v * 32 + b] = r;
            for (int n = 0; n < 64; ++n) r = xorshift_step(r);
        }
    }
    return t;
}

}  // namespace

struct mi355rec_slimen : Handle {                     // `timer`: the fit kernel; `call_timer`: the Gram build of create
    int n_users = 0, n_items = 0;
    DeviceBuffer<float> G, diag, w_slots, h_slots, out_val;
    DeviceBuffer<int> out_idx, out_n, out_iter, out_conv;
    DeviceBuffer<uint32_t> seeds, jump;
    DeviceBuffer<unsigned> queue;
    DeviceBuffer<unsigned long long> counters;
    int n_targets = 0, slots_per_target = 0, h_in_lds = 0, gram_in_lds = 0;
    double gram_ms = 0.0;
    unsigned long long counts[4] = {0, 0, 0, 0};

    ~mi355rec_slimen() { shutdown(); }
};

extern "C" int mi355rec_slimen_create(mi355rec_slimen_t *out, int32_t n_users, int32_t n_items, const int32_t *row_ptr,
                                      const int32_t *row_idx, const float *row_val, const int32_t *col_ptr, const int32_t *col_idx,
                                      const float *col_val) {
    return guarded([&] {
        MI_REQUIRE(out && row_ptr && col_ptr, "NULL argument");
        MI_REQUIRE(n_users > 0 && n_items > 0, "empty URM (%d x %d)", n_users, n_items);
        *out = nullptr;
        auto h = open_handle<mi355rec_slimen>(2);
        h->n_users = n_users;
        h->n_items = n_items;
        ReleaseScope scope(h->stream);
        hipStream_t s = h->stream;
        const size_t g_bytes = (size_t)n_items * n_items * sizeof(float);
        size_t free_b = 0, total_b = 0;
        MI_HIP(hipMemGetInfo(&free_b, &total_b));
        const size_t nnz = (size_t)row_ptr[n_users];
        const size_t need = g_bytes + 8 * nnz * 2 + ((size_t)1 << 30);      // G, both URM layouts, 1 GiB for the fit's slots and outputs
        MI_REQUIRE(need <= free_b, "the Gram matrix of %d items (%.2f GB) does not fit the device's free memory (%.2f GB)", n_items,
                   g_bytes / 1e9, free_b / 1e9);
        DeviceBuffer<int> rp, ri, cp, ci;
        DeviceBuffer<float> rv, cv;
        rp.upload(row_ptr, n_users + 1, s);
        ri.upload(row_idx, std::max<size_t>(nnz, 1), s);
        rv.upload(row_val, std::max<size_t>(nnz, 1), s);
        cp.upload(col_ptr, n_items + 1, s);
        ci.upload(col_idx, std::max<size_t>(nnz, 1), s);
        cv.upload(col_val, std::max<size_t>(nnz, 1), s);
        h->G.alloc(g_bytes / sizeof(float));
        h->diag.alloc(n_items);
        h->call_timer.start(s);
        hipLaunchKernelGGL(slimen_diag_kernel, dim3(div_up(n_items, 256)), dim3(256), 0, s, cp.ptr, cv.ptr, n_items, h->diag.ptr);
        MI_HIP(hipGetLastError());
        const size_t acc_lds = (size_t)n_items * sizeof(float);
        const char *force = getenv("MI355REC_SLIMEN_GLOBAL_GRAM");
        h->gram_in_lds = acc_lds <= LDS_LIMIT && !(force && atoi(force));
        if (h->gram_in_lds) {
            auto k = slimen_gram_kernel<true>;
            MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)acc_lds));
            hipLaunchKernelGGL(k, dim3(n_items), dim3(GRAM_THREADS), acc_lds, s, rp.ptr, ri.ptr, rv.ptr, cp.ptr, ci.ptr, cv.ptr, n_items,
                               h->G.ptr);
        } else {
            MI_HIP(hipMemsetAsync(h->G.ptr, 0, g_bytes, s));
            hipLaunchKernelGGL(slimen_gram_kernel<false>, dim3(n_items), dim3(GRAM_THREADS), 0, s, rp.ptr, ri.ptr, rv.ptr, cp.ptr, ci.ptr,
                               cv.ptr, n_items, h->G.ptr);
        }
        MI_HIP(hipGetLastError());
        h->call_timer.stop(s);
        auto jt = jump_tables();
        h->jump.upload(jt.data(), jt.size(), s);
        MI_HIP(hipStreamSynchronize(s));
        h->gram_ms = h->call_timer.elapsed_ms();
        *out = h.release();
    });
}

extern "C" int mi355rec_slimen_fit(mi355rec_slimen_t h, int32_t start_item, int32_t end_item, const uint32_t *seeds, double alpha,
                                   double l1_ratio, int32_t positive, int32_t topK, int32_t max_iter, double tol) {
    return guarded([&] {
        MI_REQUIRE(h && (seeds || start_item == end_item), "NULL argument");
        MI_REQUIRE(0 <= start_item && start_item <= end_item && end_item <= h->n_items, "item range [%d, %d) outside [0, %d)", start_item,
                   end_item, h->n_items);
        MI_REQUIRE(l1_ratio >= 0.0 && l1_ratio <= 1.0, "l1_ratio must be between 0 and 1, provided value was %g", l1_ratio);
        MI_REQUIRE(alpha >= 0.0 && topK >= -1 && max_iter >= 1, "alpha >= 0, topK >= -1 and max_iter >= 1 required");
        ensure_device();
        ReleaseScope scope(h->stream);
        hipStream_t s = h->stream;
        const int N = h->n_items, n_t = end_item - start_item;
        h->n_targets = n_t;
        h->slots_per_target = std::max(1, topK < 0 ? N - 1 : std::min(topK, N - 1));
        // l1 / l2 as sklearn forms them (alpha * l1_ratio * n_samples in float64) and hands them to the float32 solver
        const float l1 = (float)(alpha * l1_ratio * h->n_users), l2 = (float)(alpha * (1.0 - l1_ratio) * h->n_users);
        std::vector<uint32_t> sd(seeds, seeds + n_t);
        for (auto &v : sd) v = v ? v : 1u;                         // our_rand_r replaces a zero state by 1
        h->seeds.upload(sd.data(), std::max(n_t, 1), s);
        h->out_idx.alloc((size_t)std::max(n_t, 1) * h->slots_per_target);
        h->out_val.alloc((size_t)std::max(n_t, 1) * h->slots_per_target);
        h->out_n.alloc(std::max(n_t, 1));
        h->out_iter.alloc(std::max(n_t, 1));
        h->out_conv.alloc(std::max(n_t, 1));
        h->queue.alloc_zero(1, s);
        h->counters.alloc_zero(4, s);

        const int nmask = (N + 31) / 32;
        const size_t lds_h = (size_t)nmask * 4 + (size_t)N * 4;
        const char *force = getenv("MI355REC_SLIMEN_GLOBAL_H");
        h->h_in_lds = (lds_h + FIT_STATIC_LDS <= LDS_LIMIT) && !(force && atoi(force));
        const int cus = multiprocessor_count();
        const int grid = std::max(1, std::min(n_t, h->h_in_lds ? cus : 2 * cus));
        const size_t dyn = h->h_in_lds ? lds_h : (size_t)nmask * 4;
        h->w_slots.alloc((size_t)grid * N);
        if (!h->h_in_lds) h->h_slots.alloc((size_t)grid * N);

        FitArgs a{};
        a.G = h->G.ptr;
        a.diag = h->diag.ptr;
        a.seeds = h->seeds.ptr;
        a.jump = h->jump.ptr;
        a.w_slots = h->w_slots.ptr;
        a.h_slots = h->h_in_lds ? nullptr : h->h_slots.ptr;
        a.queue = h->queue.ptr;
        a.n_items = N;
        a.start = start_item;
        a.n_targets = n_t;
        a.max_iter = max_iter;
        a.positive = positive ? 1 : 0;
        a.topK = topK;
        a.slots_per_target = h->slots_per_target;
        a.l1 = l1;
        a.l2 = l2;
        a.tol = (float)tol;
        a.out_idx = h->out_idx.ptr;
        a.out_val = h->out_val.ptr;
        a.out_n = h->out_n.ptr;
        a.out_iter = h->out_iter.ptr;
        a.out_conv = h->out_conv.ptr;
        a.counters = h->counters.ptr;
        h->timer.start(s);
        if (n_t > 0) {
            if (h->h_in_lds) {
                auto k = slimen_fit_kernel<true>;
                MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
                hipLaunchKernelGGL(k, dim3(grid), dim3(THREADS), dyn, s, a);
            } else {
                hipLaunchKernelGGL(slimen_fit_kernel<false>, dim3(grid), dim3(THREADS), dyn, s, a);
            }
            MI_HIP(hipGetLastError());
        }
        h->timer.stop(s);
        MI_HIP(hipMemcpyAsync(h->counts, h->counters.ptr, sizeof(h->counts), hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
        const double ms = h->timer.elapsed_ms();
        h->stats = mi355rec_stats{};
        h->stats.call_ms = ms;
        h->stats.kernel_ms = ms;
        h->stats.n_launches = n_t > 0 ? 1 : 0;
        h->stats.n_timed = h->stats.n_launches;
        h->stats.n_units = n_t;
        h->stats.algorithmic_bytes = (double)h->counts[0] * N * sizeof(float);   // one row of G per accepted change
    });
}

extern "C" int mi355rec_slimen_get(mi355rec_slimen_t h, int32_t *counts, int32_t *n_iter, int32_t *converged, int32_t *rows, float *values,
                                   int32_t slots_per_target) {
    return guarded([&] {
        MI_REQUIRE(h && counts && n_iter && converged && rows && values, "NULL argument");
        MI_REQUIRE(slots_per_target == h->slots_per_target, "slots_per_target %d, the fit wrote %d", slots_per_target, h->slots_per_target);
        ensure_device();
        ReleaseScope scope(h->stream);
        const int n = h->n_targets;
        if (n == 0) return;
        h->out_n.download(counts, n, h->stream);
        h->out_iter.download(n_iter, n, h->stream);
        h->out_conv.download(converged, n, h->stream);
        h->out_idx.download(rows, (size_t)n * h->slots_per_target, h->stream);
        h->out_val.download(values, (size_t)n * h->slots_per_target, h->stream);
        MI_HIP(hipStreamSynchronize(h->stream));
    });
}

extern "C" int mi355rec_slimen_get_gram(mi355rec_slimen_t h, int32_t row0, int32_t row1, float *rows, float *diag) {
    return guarded([&] {
        MI_REQUIRE(h && rows, "NULL argument");
        MI_REQUIRE(0 <= row0 && row0 <= row1 && row1 <= h->n_items, "row range [%d, %d) outside [0, %d)", row0, row1, h->n_items);
        ensure_device();
        ReleaseScope scope(h->stream);
        const size_t N = (size_t)h->n_items, n = (size_t)(row1 - row0);
        if (n == 0) return;
        MI_HIP(hipMemcpyAsync(rows, h->G.ptr + (size_t)row0 * N, n * N * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        if (diag) MI_HIP(hipMemcpyAsync(diag, h->diag.ptr + row0, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        MI_HIP(hipStreamSynchronize(h->stream));
    });
}

extern "C" int mi355rec_slimen_get_stats(mi355rec_slimen_t h, mi355rec_stats *stats) { return handle_get_stats(h, stats); }

extern "C" int mi355rec_slimen_fit_info(mi355rec_slimen_t h, int64_t *changes, int64_t *sweeps, int64_t *steps, int64_t *gap_tests,
                                        int32_t *h_in_lds, int32_t *gram_in_lds, double *gram_ms) {
    return guarded([&] {
        MI_REQUIRE(h && changes && sweeps && steps && gap_tests && h_in_lds && gram_in_lds && gram_ms, "NULL argument");
        *changes = (int64_t)h->counts[0];
        *sweeps = (int64_t)h->counts[1];
        *steps = (int64_t)h->counts[2];
        *gap_tests = (int64_t)h->counts[3];
        *h_in_lds = h->h_in_lds;
        *gram_in_lds = h->gram_in_lds;
        *gram_ms = h->gram_ms;
    });
}

extern "C" void mi355rec_slimen_destroy(mi355rec_slimen_t h) { handle_destroy(h); }
