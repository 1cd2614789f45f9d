// handoff.hip -- what the device-to-device hand-offs of a trained model to the factor scorer share (gfx950):
//   f64_to_f32_kernel    out[i] = (float)in[i], round to nearest even: the float64 matrices of an IALS handle into the scorer's float32
//                        U and V (mi355rec_scorer_update_from_ials, ials.hip).  A pure stream, 12 bytes per cell: a lane reads two
//                        16-byte pairs of doubles and writes one 16-byte quad of floats, grid-stride over a grid sized to the
//                        device; no LDS.
//   hand_off_check / hand_off_begin / hand_off_end: the refusals, the ordering and the stats of mi355rec_scorer_update_from_mf
//                        (mf.hip, which launches its own getters' kernels) and mi355rec_scorer_update_from_ials.
// A translation unit of its own, like cand.hip: the device code of score.hip, mf.hip and ials.hip stays what it was.
#include "common.h"
#include "score.h"

#include <algorithm>

namespace mi355rec {
namespace {

constexpr int CONVERT_THREADS = 256;

// vec: both pointers are 16-byte aligned -- quads [0, n / 4) go through the wide path, the last n % 4 cells one lane each
__global__ __launch_bounds__(CONVERT_THREADS) void f64_to_f32_kernel(const double *__restrict__ in, float *__restrict__ out, long long n,
                                                                     int vec) {
    const long long stride = (long long)gridDim.x * CONVERT_THREADS;
    const long long t = (long long)blockIdx.x * CONVERT_THREADS + threadIdx.x;
    const long long quads = vec ? n >> 2 : 0;
    const double2 *in2 = reinterpret_cast<const double2 *>(in);
    float4 *out4 = reinterpret_cast<float4 *>(out);
    for (long long q = t; q < quads; q += stride) {
        const double2 a = in2[2 * q], b = in2[2 * q + 1];
        out4[q] = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
    }
    for (long long e = (quads << 2) + t; e < n; e += stride) out[e] = (float)in[e];
}

}  // namespace

void f64_to_f32_enqueue(const double *in, float *out, size_t n, hipStream_t s) {
    if (n == 0) return;
    const int vec = (reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
    const long long work = vec ? std::max<long long>((long long)(n >> 2), (long long)(n & 3)) : (long long)n;
    const int grid = (int)std::max<long long>(1, std::min<long long>(div_up(work, CONVERT_THREADS), 8LL * multiprocessor_count()));
    hipLaunchKernelGGL(f64_to_f32_kernel, dim3(grid), dim3(CONVERT_THREADS), 0, s, in, out, (long long)n, vec);
    MI_HIP(hipGetLastError());
}

void hand_off_check(const mi355rec_scorer *sc, const char *source, int n_users, int n_items, int k, int use_bias) {
    MI_REQUIRE(sc->n_users == n_users, "the %s handle has %d users, the scorer %d", source, n_users, sc->n_users);
    MI_REQUIRE(sc->n_items == n_items, "the %s handle has %d items, the scorer %d", source, n_items, sc->n_items);
    MI_REQUIRE(sc->k == k, "the %s handle has %d factors, the scorer %d", source, k, sc->k);
    MI_REQUIRE((sc->use_bias != 0) == (use_bias != 0), "the %s handle %s biases, the scorer %s", source, use_bias ? "has" : "has no",
               sc->use_bias ? "has them" : "has none");
}

void hand_off_begin(mi355rec_scorer *sc, hipStream_t source) {
    MI_HIP(hipStreamSynchronize(sc->stream));   // lists an evaluator queued on the scorer's stream still read the old model
    sc->call_timer.start(source);
}

void hand_off_end(mi355rec_scorer *sc, hipStream_t source, double bytes, int launches) {
    sc->call_timer.stop(source);
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(source));
    sc->stats = mi355rec_stats{};
    sc->stats.call_ms = sc->stats.kernel_ms = sc->call_timer.elapsed_ms();
    sc->stats.n_launches = sc->stats.n_timed = launches;
    sc->stats.algorithmic_bytes = bytes;
}

}  // namespace mi355rec
