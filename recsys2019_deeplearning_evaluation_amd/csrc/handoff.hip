// handoff.hip -- what the device-to-device hand-offs of a trained model to the factor scorer and to the sparse scorer share (gfx950):
//   f64_to_f32_kernel    out[i] = (float)in[i], round to nearest even: the float64 matrices of an IALS handle into the scorer's float32
//                        U and V (mi355rec_scorer_update_from_ials, ials.hip).  A pure stream, 12 bytes per cell: a lane reads two
//                        16-byte pairs of doubles and writes one 16-byte quad of floats, grid-stride over a grid sized to the
//                        device; no LDS.
//   hand_off_check / hand_off_begin / hand_off_end: the refusals, the ordering and the stats of mi355rec_scorer_update_from_mf
//                        (mf.hip, which launches its own getters' kernels) and mi355rec_scorer_update_from_ials.
//   csr_adopt_kernel     a CSR that is already on the device into the sparse scorer's spare buffers, checked in the same pass; with
//                        spscorer_adopt_begin / spscorer_adopt, the ordering, the refusal and the stats of every device-resident
//                        similarity model that fills the sparse scorer (mi355rec_spscorer_update_from_slim, slim.hip, is the first).
// A translation unit of its own, like cand.hip: the device code of score.hip, mf.hip, ials.hip and slim.hip stays what it was.
#include "common.h"
#include "score.h"
#include "spscorer_plan.h"

#include <algorithm>
#include <climits>

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

constexpr int ADOPT_THREADS = 256;
constexpr int ADOPT_ROWS = ADOPT_THREADS / 64;      // rows of a workgroup: one wavefront each, as spexact_check_kernel

// A CSR on the device (n_rows x n_cols) into out_ptr / out_idx / out_val, checked in the same pass: *first_bad = the lowest row that
// is not canonical -- pointers that do not climb from 0 inside [0, capacity], an id outside [0, n_cols), an id not above its
// predecessor.  The lanes of a row's wavefront stride it by 64: 256 contiguous bytes per load and per store, two loads and two stores
// in flight per lane and step (a row starts wherever its predecessor ends, so there is no 16-byte alignment to build wider
// accesses on); the predecessor's id comes from the neighbouring lane, the first lane's from the cell before.  Lane 0 copies the
// row's pointer, the last row's wavefront the final one as well.  A row whose pointers are bad is not walked at all, and no lane
// touches a cell at or past `capacity` -- the cells both the source and the destination are known to have -- so a CSR that is
// garbage is reported, never followed.  No LDS, 4 wavefronts per workgroup: occupancy is bounded by nothing but the grid.
__global__ __launch_bounds__(ADOPT_THREADS) void csr_adopt_kernel(const int *__restrict__ indptr, const int *__restrict__ indices,
                                                                  const float *__restrict__ data, int n_rows, int n_cols, long long capacity,
                                                                  int *__restrict__ out_ptr, int *__restrict__ out_idx,
                                                                  float *__restrict__ out_val, int *first_bad) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ADOPT_ROWS + (threadIdx.x >> 6);
    if (row >= n_rows) return;          // (wavefront-uniform)
    const int s = indptr[row], e = indptr[row + 1];
    if (lane == 0) {
        out_ptr[row] = s;
        if (row == n_rows - 1) out_ptr[n_rows] = e;
    }
    bool bad = s < 0 || e < s || (long long)e > capacity || (row == 0 && s != 0);
    if (!bad)
        for (int base = s; base < e; base += 64) {
            const int t = base + lane;
            const bool mine = t < e;
            const int col = mine ? indices[t] : 0;
            const float val = mine ? data[t] : 0.f;
            int before = __shfl_up(col, 1);
            if (lane == 0) before = base > s ? indices[base - 1] : -1;
            if (mine) {
                bad |= col < 0 || col >= n_cols || before >= col;
                out_idx[t] = col;
                out_val[t] = val;
            }
        }
    if (__ballot(bad) && lane == 0) atomicMin(first_bad, row);
}

}  // namespace

void spscorer_adopt_begin(mi355rec_spscorer *sc, hipStream_t source) {
    MI_HIP(hipStreamSynchronize(sc->stream));   // lists an evaluator queued on the scorer's stream still read the old B
    sc->timer.start(source);
}

void spscorer_adopt(mi355rec_spscorer *sc, hipStream_t source, const int *indptr, const int *indices, const float *data, size_t max_cells,
                    double build_bytes, int build_launches) {
    spscorer_reserve_spare(sc, max_cells);
    // [0]: the kernel's verdict; [1]: the cells of the new B, read where the kernel wrote them
    DeviceBuffer<int> verdict;
    int word = INT_MAX, nnz = 0;
    verdict.upload(&word, 1, source);
    hipLaunchKernelGGL(csr_adopt_kernel, dim3(div_up(sc->n_mid, ADOPT_ROWS)), dim3(ADOPT_THREADS), 0, source, indptr, indices, data, sc->n_mid,
                       sc->n_items, (long long)std::min(max_cells, sc->spare_idx.count), sc->spare_ptr.ptr, sc->spare_idx.ptr, sc->spare_val.ptr,
                       verdict.ptr);
    MI_HIP(hipGetLastError());
    verdict.download(&word, 1, source);
    MI_HIP(hipMemcpyAsync(&nnz, sc->spare_ptr.ptr + sc->n_mid, sizeof(int), hipMemcpyDeviceToHost, source));
    MI_HIP(hipStreamSynchronize(source));
    // the builders of this library produce canonical rows by construction: this is a bug here, not a caller's mistake
    if (word != INT_MAX)
        fail(MI355REC_E_HIP, "internal error: row %d of the %d x %d CSR handed over on the device is not canonical (row pointers outside [0, %zu] or "
                             "not climbing from 0, a column id outside [0, %d) or not above its predecessor); the scorer keeps its model",
             word, sc->n_mid, sc->n_items, max_cells, sc->n_items);
    int launches = build_launches + 1;
    DeviceBuffer<int> cuts;
    if (sc->exact) {
        spexact_check_and_cut(sc, source, sc->spare_ptr.ptr, sc->spare_idx.ptr, &cuts);
        launches += 2;
    }
    sc->timer.stop(source);
    MI_HIP(hipStreamSynchronize(source));       // neither handle's later work can race the copy
    spscorer_swap_in(sc, (size_t)nnz, cuts);
    sc->stats = mi355rec_stats{};
    sc->stats.call_ms = sc->stats.kernel_ms = sc->timer.elapsed_ms();
    sc->stats.n_launches = sc->stats.n_timed = launches;
    sc->stats.algorithmic_bytes = build_bytes + 2.0 * spscorer_plan::csr_bytes(sc->n_mid, (size_t)nnz)
                                  + spscorer_plan::exact_table_bytes(sc->n_mid, (size_t)nnz, spexact_table_cells(sc));
}

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
