// stack.hip -- CSR matrices that are resident in HBM, stacked row-wise into one CSR matrix (gfx950): the dataMatrix of the CF+CBF
// hybrid KNN recommenders (KNN/ItemKNN_CFCBF_Hybrid_Recommender.py:20-25, UserKNN_CFCBF_Hybrid_Recommender.py:21-26) without the
// reference's three SciPy passes (scale, hstack, transpose + CSR conversion) and without a PCIe upload per fit.
//   csr_stack_kernel   ONE launch for all blocks and all three arrays; the block table travels as a kernel argument.
//                      Workgroups [0, g_ptr) write the row pointers (a block's pointers + the cells before it), the next g_cell copy
//                      the column ids (and flag ids outside [0, n_cols)), the last g_cell scale the values.
// A cell array is written in quads: one 16-byte store per lane to a 16-byte aligned destination.  A block's cells start at the nnz of
// the blocks before it, so its SOURCE is not aligned to the destination's quads in general: the quad's four words are read from an
// address that is only 4-byte aligned (the compiler makes one 16-byte global load of them, which global memory on gfx950 takes at
// any dword alignment; consecutive lanes read consecutive 16 bytes).  A quad that straddles two blocks, the tail, or a destination
// the caller did not align, goes word by word.
// A translation unit of its own: sim.hip's device code does not change with it.
#include "common.h"

#include <climits>

namespace mi355rec {
namespace {

constexpr int STACK_THREADS = 256;
constexpr int MAXB = MI355REC_STACK_MAX_BLOCKS;

struct StackTable {
    int n_blocks, n_cols, total_rows, total_cells;
    int vec;                            // both cell destinations are 16-byte aligned
    int g_ptr, g_cell;                  // workgroups of the row-pointer part and of EACH cell array
    int row_start[MAXB + 1], cell_start[MAXB + 1];
    const int *indptr[MAXB];
    const uint32_t *indices[MAXB], *data[MAXB];
    float scale[MAXB];
    int *out_indptr;
    uint32_t *out_indices, *out_data;
    int *bad_index;                     // set to 1 by a column id outside [0, n_cols)
};

struct CellSource {
    const uint32_t *src;                // the block's array, so that src[p - start] is cell p of the stack
    int start, end;
    float scale;
};

// The block that holds cell p (0 <= p < total_cells): the last one that starts at or before p -- an empty block shares its start
// with the next one and is passed over.  Constant indices only: the table stays in scalar registers.
__device__ __forceinline__ CellSource cell_source(const StackTable &t, int p, bool values) {
    CellSource c{values ? t.data[0] : t.indices[0], t.cell_start[0], t.cell_start[1], t.scale[0]};
#pragma unroll
    for (int b = 1; b < MAXB; ++b) {
        if (b < t.n_blocks && p >= t.cell_start[b]) {
            c.src = values ? t.data[b] : t.indices[b];
            c.start = t.cell_start[b];
            c.end = t.cell_start[b + 1];
            c.scale = t.scale[b];
        }
    }
    return c;
}

// a value times the block's scale: one float32 product; a scale of exactly 1 hands the bits on (a signalling NaN stays what it is)
__device__ __forceinline__ uint32_t scaled(uint32_t bits, float scale) {
    return scale == 1.0f ? bits : __float_as_uint(__uint_as_float(bits) * scale);
}

__global__ __launch_bounds__(STACK_THREADS) void csr_stack_kernel(const StackTable t) {
    const int tid = threadIdx.x;
    int wg = blockIdx.x;
    if (wg < t.g_ptr) {
        const int64_t r = (int64_t)wg * STACK_THREADS + tid;
        if (r > t.total_rows) return;
        if (r == t.total_rows) {
            t.out_indptr[r] = t.total_cells;
            return;
        }
        const int *src = t.indptr[0];
        int first = 0, before = 0;
#pragma unroll
        for (int b = 1; b < MAXB; ++b) {
            if (b < t.n_blocks && r >= t.row_start[b]) {
                src = t.indptr[b];
                first = t.row_start[b];
                before = t.cell_start[b];
            }
        }
        t.out_indptr[r] = src[r - first] + before;
        return;
    }
    wg -= t.g_ptr;
    const bool values = wg >= t.g_cell;
    if (values) wg -= t.g_cell;
    uint32_t *out = values ? t.out_data : t.out_indices;
    const int64_t p0 = ((int64_t)wg * STACK_THREADS + tid) * 4;
    if (p0 >= t.total_cells) return;
    bool bad = false;
    const CellSource c = cell_source(t, (int)p0, values);
    if (t.vec && p0 + 4 <= c.end) {             // (c.end <= total_cells: the whole quad is inside one block)
        const uint32_t *s = c.src + ((int)p0 - c.start);
        uint4 q{s[0], s[1], s[2], s[3]};
        if (values) {
            q.x = scaled(q.x, c.scale); q.y = scaled(q.y, c.scale); q.z = scaled(q.z, c.scale); q.w = scaled(q.w, c.scale);
        } else {
            const uint32_t n = (uint32_t)t.n_cols;
            bad = q.x >= n || q.y >= n || q.z >= n || q.w >= n;
        }
        *reinterpret_cast<uint4 *>(out + p0) = q;
    } else {
        const int last = (int)min(p0 + 4, (int64_t)t.total_cells);
        for (int p = (int)p0; p < last; ++p) {
            const CellSource e = cell_source(t, p, values);
            const uint32_t w = e.src[p - e.start];
            if (!values) bad |= w >= (uint32_t)t.n_cols;
            out[p] = values ? scaled(w, e.scale) : w;
        }
    }
    if (bad) atomicOr(t.bad_index, 1);
}

}  // namespace
}  // namespace mi355rec

using namespace mi355rec;

extern "C" int mi355rec_csr_stack_device(int32_t n_blocks, const mi355rec_csr_block *blocks, int32_t n_cols, int32_t *d_indptr,
                                         int32_t *d_indices, float *d_data) {
    return guarded([&] {
        // ---- the host's checks: nothing below them is reached with a table the kernel could leave its arrays with
        MI_REQUIRE(n_blocks >= 1, "csr_stack: %d blocks", n_blocks);
        MI_REQUIRE(blocks && d_indptr && d_indices && d_data, "NULL argument");
        MI_REQUIRE(n_cols >= 0, "csr_stack: %d columns", n_cols);
        if (n_blocks > MAXB) fail(MI355REC_E_UNSUPPORTED, "csr_stack: %d blocks, at most %d", n_blocks, MAXB);
        StackTable t{};
        int64_t rows = 0, cells = 0;
        for (int b = 0; b < n_blocks; ++b) {
            const mi355rec_csr_block &k = blocks[b];
            MI_REQUIRE(k.n_rows >= 0 && k.nnz >= 0, "csr_stack: block %d has %d rows and %d cells", b, k.n_rows, k.nnz);
            MI_REQUIRE(k.d_indptr || k.n_rows == 0, "csr_stack: block %d has no row pointers", b);
            MI_REQUIRE((k.d_indices && k.d_data) || k.nnz == 0, "csr_stack: block %d has %d cells and a NULL array", b, k.nnz);
            MI_REQUIRE(k.n_rows > 0 || k.nnz == 0, "csr_stack: block %d has %d cells in no rows", b, k.nnz);
            t.row_start[b] = (int)rows;
            t.cell_start[b] = (int)cells;
            t.indptr[b] = k.d_indptr;
            t.indices[b] = reinterpret_cast<const uint32_t *>(k.d_indices);
            t.data[b] = reinterpret_cast<const uint32_t *>(k.d_data);
            t.scale[b] = k.scale;
            rows += k.n_rows;
            cells += k.nnz;
            MI_REQUIRE(rows < INT32_MAX && cells <= INT32_MAX,
                       "csr_stack: %lld rows and %lld cells up to block %d do not fit int32 row pointers", (long long)rows, (long long)cells, b);
        }
        for (int b = n_blocks; b <= MAXB; ++b) {
            t.row_start[b] = (int)rows;
            t.cell_start[b] = (int)cells;
        }
        t.n_blocks = n_blocks;
        t.n_cols = n_cols;
        t.total_rows = (int)rows;
        t.total_cells = (int)cells;
        t.vec = ((reinterpret_cast<uintptr_t>(d_indices) | reinterpret_cast<uintptr_t>(d_data)) & 15) == 0;
        t.g_ptr = div_up(rows + 1, STACK_THREADS);
        t.g_cell = div_up(div_up(cells, 4), STACK_THREADS);
        t.out_indptr = d_indptr;
        t.out_indices = reinterpret_cast<uint32_t *>(d_indices);
        t.out_data = reinterpret_cast<uint32_t *>(d_data);
        // ---- the device
        ensure_device();
        hipStream_t s = pooled_stream();
        struct Return {
            hipStream_t s;
            ~Return() {
                (void)hipStreamSynchronize(s);
                pooled_stream_return(s);
            }
        } give_back{s};
        ReleaseScope scope(s);
        DeviceBuffer<int> bad;
        bad.alloc_zero(1, s);
        t.bad_index = bad.ptr;
        hipLaunchKernelGGL(csr_stack_kernel, dim3(t.g_ptr + 2 * t.g_cell), dim3(STACK_THREADS), 0, s, t);
        MI_HIP(hipGetLastError());
        int found = 0;
        bad.download(&found, 1, s);
        MI_HIP(hipStreamSynchronize(s));
        MI_REQUIRE(found == 0, "csr_stack: a block holds a column id outside [0, %d)", n_cols);
    });
}
