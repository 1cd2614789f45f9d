// extern "C" wrapper around the bit-row part of csrc/mf_plan.h for tests/test_mf_bit_rows_plan.py, which compiles it with g++ and
// calls it through ctypes: no GPU, no HIP runtime.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/mf_plan.h"

#include <cstdint>
#include <cstring>

using namespace mi355rec;

// The shape, s[10]: algorithm, n_users, n_items, nnz, k, f64, batch_size, sharded, fast_schedule, bit_rows.
static MfShape shape_of(const int64_t *s) {
    MfShape m;
    m.algorithm = (int)s[0];
    m.n_users = (int)s[1];
    m.n_items = (int)s[2];
    m.nnz = s[3];
    m.k = (int)s[4];
    m.f64 = s[5] != 0;
    m.batch_size = (int)s[6];
    m.sharded = s[7] != 0;
    m.fast_schedule = s[8] != 0;
    m.bit_rows = s[9] != 0;
    return m;
}

static MfKnobs knobs_of(int row_bitmap) {
    MfKnobs k;
    k.row_bitmap = row_bitmap != 0;
    return k;
}

extern "C" int br_row_words(int64_t n_entries) { return bit_row_words(n_entries); }

// MI355REC_MF_ROW_BITMAP as the process's environment has it
extern "C" int br_read_knob() { return read_mf_knobs().row_bitmap; }

// out[4]: keys a workgroup sorts, LDS bytes of the sort kernel without and with the bit row, bit_rows_fit
extern "C" void br_fit(const int64_t *s, int row_bitmap, uint64_t sort_storage_bytes, uint64_t static_lds_bytes, uint64_t lds_limit, int64_t *out) {
    const MfShape m = shape_of(s);
    const int np = sched_np(tasks_per_batch(m));
    const int64_t v[4] = {np, (int64_t)sched_lds_bytes(np, (size_t)sort_storage_bytes),
                          (int64_t)sched_lds_bytes_bit_rows(np, (size_t)sort_storage_bytes, (long long)m.n_users + m.n_items),
                          bit_rows_fit(m, knobs_of(row_bitmap), (size_t)sort_storage_bytes, (size_t)static_lds_bytes, (size_t)lds_limit)};
    memcpy(out, v, sizeof(v));
}

// the in-LDS schedule holds a stream of n_batches mini-batches of this shape
extern "C" int br_fast_fits(const int64_t *s, int64_t n_batches) { return fast_schedule_fits(shape_of(s), MfKnobs{}, n_batches); }

// out[6]: words, row_words and bit_rows of fast_sched_numbers_bit_rows; the same three of fast_sched_numbers
extern "C" void br_numbers(const int64_t *s, uint64_t sort_storage_bytes, int64_t *out) {
    const MfShape m = shape_of(s);
    const FastSchedNumbers a = fast_sched_numbers_bit_rows(m, MfKnobs{}, (size_t)sort_storage_bytes);
    const FastSchedNumbers b = fast_sched_numbers(m, MfKnobs{}, (size_t)sort_storage_bytes);
    const int64_t v[6] = {a.words, a.row_words, a.bit_rows, b.words, b.row_words, b.bit_rows};
    memcpy(out, v, sizeof(v));
}

// out[6]: fast1, table_batches, touched and bit_rows of buffer_plan_bit_rows; touched and bit_rows of buffer_plan
extern "C" void br_buffers(const int64_t *s, uint64_t n_samples, int64_t n_batches, int whole_stream, int64_t *out) {
    const MfShape m = shape_of(s);
    const BufferPlan a = buffer_plan_bit_rows(m, MfKnobs{}, (size_t)n_samples, n_batches, whole_stream != 0);
    const BufferPlan b = buffer_plan(m, MfKnobs{}, (size_t)n_samples, n_batches, whole_stream != 0);
    const int64_t v[6] = {a.fast1, a.table_batches, (int64_t)a.touched, (int64_t)a.bit_rows, (int64_t)b.touched, (int64_t)b.bit_rows};
    memcpy(out, v, sizeof(v));
}

extern "C" void br_parity_constants(int64_t *out) {
    const int64_t v[3] = {PARITY_PARTS, PARITY_PART_MAX, FAST_MAX_BATCHES};
    memcpy(out, v, sizeof(v));
}

// The column pass over rows[n_batches][row_words] and par[n_entries], both in place: every word column, the padding ones included.
extern "C" void br_parity_pass(uint32_t *rows, int row_words, int n_batches, uint8_t *par, int64_t n_entries) {
    for (int w = 0; w < row_words; ++w) parity_column(rows, row_words, n_batches, par, n_entries, w);
}
