// asy_estimate.hip -- AsySVD's user factors from the learned Y on MI355X (gfx950): USER_factors = URM . Y, every row divided by the square
// root of its profile length -- _estimate_user_factors (MatrixFactorization/Cython/MatrixFactorization_Cython.py:281-304), which the
// reference runs on the host before every validation of an early-stopping fit and once more for the cold users of a new URM.
// DESIGN.md section 20.
//
// The contract is SciPy's csr @ ndarray (csr_matvecs) in float64 bit for bit, then NumPy's row division: every output cell starts at
// +0.0 and walks the user's stored cells IN CSR STORAGE ORDER with acc = acc + ((double)a * Y[i][f]), the product rounded before the
// add, and is divided once, IEEE-rounded, by a divisor the HOST computed (the device's sqrt is no part of the argument).  Nothing here
// may contract the two into a fused multiply-add (hipcc's default for device code): the pragma below switches contraction off for this
// translation unit and mul_add_rn spells the two roundings out, as in densescore.hip.  Only the additions of ONE cell are a chain: no row
// is split, nothing is reduced across lanes, there are no atomics and no LDS, and two calls give the same bytes.
//
//   asy_estimate_kernel   a group of G lanes takes one row and one column tile (asy_estimate_plan.h: layout), a lane keeps VEC adjacent
//                         factors' accumulators in registers.  The group reads G of the row's ids and values at a time, one cell per lane
//                         and coalesced, and hands them round with __shfl; DEPTH rows of Y (16 bytes per lane where VEC is 2) are
//                         requested before the first of them is added, the adds stay in order.  Rows go out longest first.
// Y is a few tens of MB at most and is read nnz / n_items times over: a gather the Infinity Cache and L2 serve, not HBM.
// A translation unit of its own, like cand.hip and handoff.hip: the device code of mf.hip stays what it was.
#include "asy_estimate.h"
#include "asy_estimate_plan.h"

#include <algorithm>
#include <type_traits>
#include <vector>

#pragma clang fp contract(off)

namespace mi355rec {
namespace {

using namespace asy_estimate_plan;

struct AsyEstimateParams {
    AsyEstimateArrays a;
    int k, tiles;
    long long items;
};

// acc + (a * y): two float64 roundings, never one (see above and densescore.hip's mul_add_rn)
__device__ __forceinline__ double mul_add_rn(double acc, double a, double y) {
    const double product = a * y;
    return acc + product;
}

template <int VEC, int G>
__global__ __launch_bounds__(THREADS) void asy_estimate_kernel(const AsyEstimateParams p) {
    using Cells = typename std::conditional<VEC == 2, double2, double>::type;
    constexpr int STEP = G < DEPTH ? G : DEPTH;       // rows of Y in flight per lane: a chunk has no more than G cells
    const int gl = threadIdx.x & (G - 1);
    const long long item = (long long)blockIdx.x * (THREADS / G) + threadIdx.x / G;
    if (item >= p.items) return;        // (a whole group: the lanes that stay shuffle among themselves)
    const int u = p.a.order[item / p.tiles];
    const int f = ((int)(item % p.tiles) * G + gl) * VEC;
    const bool own = f < p.k;           // a lane past the last factor still carries a cell of every chunk
    const Cells *y_col = reinterpret_cast<const Cells *>(p.a.Y + (own ? f : 0));
    const size_t row_stride = (size_t)p.k / VEC;      // in Cells: VEC divides k

    double acc0 = 0.0, acc1 = 0.0;
    const int start = p.a.indptr[u], end = p.a.indptr[u + 1];
    for (int base = start; base < end; base += G) {
        const int t = base + gl;
        const int col = t < end ? p.a.indices[t] : 0;
        const float val = t < end ? p.a.data[t] : 0.f;
        const int n = min(G, end - base);
        // The loads are not predicated: a step past the row's end (or a lane past the last factor) reads a row of Y that is there -- the
        // id of another cell of the chunk, 0 beyond the end -- and its value is dropped.  Only the adds are: a dead step changes nothing.
        for (int j = 0; j < n; j += STEP) {
            Cells y[STEP];
#pragma unroll
            for (int d = 0; d < STEP; ++d) {
                const int c = G > 1 ? __shfl(col, j + d, G) : col;
                y[d] = y_col[(size_t)c * row_stride];
            }
#pragma unroll
            for (int d = 0; d < STEP; ++d) {
                const double a = (double)(G > 1 ? __shfl(val, j + d, G) : val);
                const bool live = d == 0 || j + d < n;        // (j < n: a step's first cell is always there)
                if constexpr (VEC == 2) {
                    acc0 = live ? mul_add_rn(acc0, a, y[d].x) : acc0;
                    acc1 = live ? mul_add_rn(acc1, a, y[d].y) : acc1;
                } else {
                    acc0 = live ? mul_add_rn(acc0, a, y[d]) : acc0;
                }
            }
        }
    }
    if (!own) return;
    const double divisor = p.a.divisor[u];
    if (divisor > 0.0) {
        acc0 = acc0 / divisor;
        acc1 = acc1 / divisor;
    }
    double *cell = p.a.out + (size_t)u * p.k + f;
    if constexpr (VEC == 2) *reinterpret_cast<double2 *>(cell) = make_double2(acc0, acc1);
    else *cell = acc0;
}

template <int VEC, int G>
void launch(const AsyEstimateParams &p, long long grid, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (e0) hipExtLaunchKernelGGL((asy_estimate_kernel<VEC, G>), dim3((unsigned)grid), dim3(THREADS), 0, s, e0, e1, 0, p);
    else hipLaunchKernelGGL((asy_estimate_kernel<VEC, G>), dim3((unsigned)grid), dim3(THREADS), 0, s, p);
}

template <int VEC>
void launch_group(int group, const AsyEstimateParams &p, long long grid, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    switch (group) {
    case 1: return launch<VEC, 1>(p, grid, s, e0, e1);
    case 2: return launch<VEC, 2>(p, grid, s, e0, e1);
    case 4: return launch<VEC, 4>(p, grid, s, e0, e1);
    case 8: return launch<VEC, 8>(p, grid, s, e0, e1);
    case 16: return launch<VEC, 16>(p, grid, s, e0, e1);
    case 32: return launch<VEC, 32>(p, grid, s, e0, e1);
    default: return launch<VEC, 64>(p, grid, s, e0, e1);
    }
}

}  // namespace

void asy_estimate_upload_order(int n_rows, const int32_t *indptr_host, DeviceBuffer<int> &order, hipStream_t s) {
    const int longest = longest_row(n_rows, indptr_host);
    std::vector<int32_t> count((size_t)longest + 2), rows((size_t)n_rows);
    longest_first(n_rows, indptr_host, longest, count.data(), rows.data());
    order.upload(rows.data(), rows.size(), s);
    MI_HIP(hipStreamSynchronize(s));        // `rows` is gone when this returns
}

void asy_estimate_enqueue(int n_rows, int k, const AsyEstimateArrays &a, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    const Layout l = layout(n_rows, k);
    // the 16-byte accesses of the two-factor lanes: k is even, so every row is aligned when the arrays are (device blocks are)
    MI_REQUIRE(l.vec == 1 || (reinterpret_cast<uintptr_t>(a.Y) | reinterpret_cast<uintptr_t>(a.out)) % 16 == 0,
               "internal error: Y or the output of the user-factor estimate is not 16-byte aligned");
    const AsyEstimateParams p{a, k, l.tiles, l.items};
    if (l.vec == 2) launch_group<2>(l.group, p, l.grid, s, e0, e1);
    else launch_group<1>(l.group, p, l.grid, s, e0, e1);
    MI_HIP(hipGetLastError());
}

}  // namespace mi355rec

using namespace mi355rec;

namespace {

// a stream of the pool for one stateless call, handed back drained
struct PooledStream {
    hipStream_t s;
    PooledStream() : s(pooled_stream()) {}
    ~PooledStream() {
        (void)hipStreamSynchronize(s);
        pooled_stream_return(s);
    }
};

}  // namespace

extern "C" int mi355rec_asy_user_factors(int32_t n_rows, int32_t n_items, int32_t k, const int32_t *indptr, const int32_t *indices,
                                         const float *data, const double *Y, const double *row_divisor, double *out) {
    return guarded([&] {
        MI_REQUIRE(indptr && indices && data && Y && row_divisor && out, "NULL argument");
        const Refusal refusal = check_shape(n_rows, n_items, k);
        MI_REQUIRE(refusal != EMPTY_SHAPE, "empty URM");
        MI_REQUIRE(refusal != K_RANGE || k > KMAX, "n_factors must be >= 1");
        if (refusal == K_RANGE) fail(MI355REC_E_UNSUPPORTED, "ASY_SVD: n_factors = %d exceeds %d", k, KMAX);
        // the kernel follows the pointers and indexes Y with the ids as they come: one pass on the host in front of everything
        const spscorer_plan::CsrFinding f = check_csr(n_rows, n_items, indptr, indices);
        using Finding = spscorer_plan::CsrFinding;
        MI_REQUIRE(f.kind != Finding::START_NOT_ZERO, "the row pointers start at %lld, not at 0", (long long)f.value);
        MI_REQUIRE(f.kind != Finding::POINTERS_DECREASE, "the row pointers decrease at row %d (to %lld)", f.row, (long long)f.value);
        MI_REQUIRE(f.kind != Finding::ID_OUTSIDE, "row %d stores the column id %lld, outside [0, %d)", f.row, (long long)f.value, n_items);
        const size_t nnz = (size_t)indptr[n_rows];
        ensure_device();
        PooledStream st;
        ReleaseScope scope(st.s);
        DeviceBuffer<int> d_indptr, d_indices, d_order;
        DeviceBuffer<float> d_data;
        DeviceBuffer<double> d_Y, d_divisor, d_out;
        d_indptr.upload(indptr, (size_t)n_rows + 1, st.s);
        d_indices.upload(indices, nnz, st.s);
        d_data.upload(data, nnz, st.s);
        d_Y.upload(Y, (size_t)n_items * k, st.s);
        d_divisor.upload(row_divisor, (size_t)n_rows, st.s);
        d_out.alloc((size_t)n_rows * k);
        asy_estimate_upload_order(n_rows, indptr, d_order, st.s);
        asy_estimate_enqueue(n_rows, k, {d_indptr.ptr, d_indices.ptr, d_data.ptr, d_Y.ptr, d_divisor.ptr, d_order.ptr, d_out.ptr}, st.s);
        d_out.download(out, (size_t)n_rows * k, st.s);      // (the refusals above are all behind: `out` is written by a call that ran)
        MI_HIP(hipStreamSynchronize(st.s));
    });
}
