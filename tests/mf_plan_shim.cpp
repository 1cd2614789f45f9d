// extern "C" wrapper around csrc/mf_plan.h for tests/test_mf_plan.py, which compiles it with g++ and calls it through ctypes:
// no GPU, no HIP runtime.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/mf_plan.h"

#include <cstdint>
#include <cstring>

using namespace mi355rec;

// The shape as the tests pass it around, s[9]: algorithm, n_users, n_items, nnz, k, f64, batch_size, sharded, fast_schedule.
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
    return m;
}

// The knobs, k[7]: general_schedule, no_fuse, whole_stream_schedule, ticks, group_per_member_schedule, group_no_lookahead, no_graph.
static MfKnobs knobs_of(const int64_t *k) {
    MfKnobs m;
    m.general_schedule = k[0] != 0;
    m.no_fuse = k[1] != 0;
    m.whole_stream_schedule = k[2] != 0;
    m.ticks = k[3] != 0;
    m.group_per_member_schedule = k[4] != 0;
    m.group_no_lookahead = k[5] != 0;
    m.no_graph = k[6] != 0;
    return m;
}

// the process's environment, parsed
extern "C" void mf_read_knobs(int64_t *k) {
    const MfKnobs m = read_mf_knobs();
    const int64_t v[7] = {m.general_schedule, m.no_fuse, m.whole_stream_schedule, m.ticks, m.group_per_member_schedule, m.group_no_lookahead, m.no_graph};
    memcpy(k, v, sizeof(v));
}

extern "C" void mf_constants(int64_t *out) {
    const int64_t v[15] = {SCHED_THREADS, FAST_MAX_BATCHES, FAST_MAX_SLOTS, QTASK_SLOT_MASK, QTASK_OFF_SHIFT, QTASK_OFF_MAX, QTASK_PAIR, SCHED_STAMPS,
                           META_WIDE, SLOT_ABSORBED, MU_SLOTS, ASY_KMAX, ASY_CHUNK, GRAPH_SEGMENT, MAX_GRAPH_BATCHES};
    memcpy(out, v, sizeof(v));
}

// out[6]: LPR and KI of the instance the single-model launch picks (0, 0: the any-k kernel), samples in flight, the class number a
// group stores, LPR and KI of the instance the group's launch picks for that class number (0, 0: none)
extern "C" void mf_width(int k, int f64, int64_t *out) {
    const WidthChoice c = row_width(k, f64 != 0);
    MfShape s;
    s.k = k;
    s.f64 = f64 != 0;
    int lpr = 0, ki = 0;        // launch_batch: the class number of the row width, worked out at the launch
    const bool found = dispatch_width(row_width(k, f64 != 0).klass, [&](auto l, auto i) { lpr = decltype(l)::value, ki = decltype(i)::value; });
    int group_lpr = 0, group_ki = 0;        // launch_group_batch: a dispatch of its own on the class number the group stored
    const int stored = c.klass;
    dispatch_width(stored, [&](auto l, auto i) { group_lpr = decltype(l)::value, group_ki = decltype(i)::value; });
    const int64_t v[6] = {lpr, ki, samples_in_flight(s), stored, group_lpr, group_ki};
    memcpy(out, v, sizeof(v));
    if (found != (c.klass >= 0) || (found && (c.lpr != lpr || c.ki != ki))) out[0] = out[1] = -1;     // the choice and the dispatch read one table
}

// the widest n_factors with an instance: what the group's "any-k kernel" rejection names
extern "C" int mf_widest_k(int f64) { return widest_chunks(RowWidths{}) * vec_of(f64 != 0); }

// out[4]: mini-batches per epoch, fast_schedule_fits(n_batches), schedule_span(n_batches), schedule_draws()
extern "C" void mf_schedule(const int64_t *s, const int64_t *k, int64_t n_batches, int64_t *out) {
    const MfShape m = shape_of(s);
    const MfKnobs kn = knobs_of(k);
    const int64_t v[4] = {batches_per_epoch(m), fast_schedule_fits(m, kn, n_batches), schedule_span(m, kn, n_batches), schedule_draws(m, kn)};
    memcpy(out, v, sizeof(v));
}

// out[11]: np, slot_bits, entry_bits, mid_bytes, words, group, fuse, fill_all, LDS bytes of the sort kernel, slot_rec_stride, whether
// the kernels read the slots-in-use counts
extern "C" void mf_fast_numbers(const int64_t *s, const int64_t *k, uint64_t sort_storage_bytes, int64_t *out) {
    const MfShape m = shape_of(s);
    const MfKnobs kn = knobs_of(k);
    const FastSchedNumbers f = fast_sched_numbers(m, kn, (size_t)sort_storage_bytes);
    const int64_t v[11] = {f.np, f.slot_bits, f.entry_bits, f.mid_bytes, f.words, f.group, f.fuse, f.fill_all,
                           (int64_t)sched_lds_bytes(f.np, (size_t)sort_storage_bytes), slot_rec_stride(m), reads_used_slots(m, kn)};
    memcpy(out, v, sizeof(v));
}

// out[3]: keys a workgroup sorts for mini-batches of tpb header slots, LDS bytes of the middle section and of the whole sort kernel
extern "C" void mf_sched_np(int tpb, uint64_t sort_storage_bytes, int64_t *out) {
    const int np = sched_np(tpb);
    const int64_t v[3] = {np, (int64_t)sched_mid_bytes(np, (size_t)sort_storage_bytes), (int64_t)sched_lds_bytes(np, (size_t)sort_storage_bytes)};
    memcpy(out, v, sizeof(v));
}

// the header-slot rule of the in-LDS schedule for a run of `len` incidences on an instance with `group` samples in flight
extern "C" int mf_list_is_wide(int len, int group) { return list_is_wide(len, group); }
extern "C" int mf_header_slots(int len, int group) { return header_slots(len, group); }

// out[4]: batch_bits, end_bit, end_bit <= 64, by_rank
extern "C" void mf_general(const int64_t *s, int64_t n_batches, int64_t *out) {
    const GeneralSched g = general_sched(shape_of(s), n_batches);
    const int64_t v[4] = {g.batch_bits, g.end_bit, g.fits, g.by_rank};
    memcpy(out, v, sizeof(v));
}

// out[17]: asy, fast1, general, incidences and whether they fit (as asked when `general`: 0, 1 otherwise), table_batches, elements of
// tasks, recs, batch_count, slot_recs, sorted_slot, qtask, used, touched, loss_slots, ticks, sched_ticks
extern "C" void mf_buffers(const int64_t *s, const int64_t *k, uint64_t n_samples, int64_t n_batches, int whole_stream, int64_t *out) {
    const MfShape m = shape_of(s);
    const BufferPlan b = buffer_plan(m, knobs_of(k), (size_t)n_samples, n_batches, whole_stream != 0);
    const int64_t v[17] = {b.asy, b.fast1, b.general, b.general ? (int64_t)b.incidences : 0, b.general ? b.incidences_fit : 1, b.table_batches,
                           (int64_t)b.tasks, (int64_t)b.recs, (int64_t)b.batch_count, (int64_t)b.slot_recs, (int64_t)b.sorted_slot, (int64_t)b.qtask,
                           (int64_t)b.used, (int64_t)b.touched, (int64_t)loss_slot_count(m), (int64_t)tick_count(m), (int64_t)sched_tick_count()};
    memcpy(out, v, sizeof(v));
}

// Mini-batches [first, last) of a stream: out[(b - first) * 6 ..]: batch-local index, schedule in front (0 none, 1 draw, 2 whole stream,
// 3 part), its sample offset, samples and mini-batches (0 without a schedule), mini-batches of the stream end behind (0: none)
extern "C" void mf_walk(const int64_t *s, const int64_t *k, int64_t n_samples, int64_t n_batches, int draw, int64_t first, int64_t last, int64_t *out) {
    const MfShape m = shape_of(s);
    const long long span = schedule_span(m, knobs_of(k), n_batches);
    for (long long b = first; b < last; ++b, out += 6) {
        const StreamStep st = stream_step(n_samples, n_batches, span, m.batch_size, draw != 0, b);
        const bool sched = st.sched != SCHED_NONE;
        const int64_t v[6] = {st.local, st.sched, sched ? st.sample_offset : 0, sched ? st.sched_samples : 0, sched ? st.sched_batches : 0, st.end_batches};
        memcpy(out, v, sizeof(v));
    }
}

// One epoch call of a handle: out[7]: mini-batches per epoch, timed epochs, use_graph, graph segments, first and last mini-batch of the
// last segment, launches accounted
extern "C" void mf_epoch(const int64_t *s, const int64_t *k, int max_timed, int64_t n_epochs, int64_t *out) {
    const MfShape m = shape_of(s);
    const long long per_epoch = batches_per_epoch(m), timed = timed_epochs(max_timed, per_epoch, n_epochs), nb = graph_batches(m);
    const BatchRange r = graph_segment(nb, graph_segments(nb) - 1);
    const int64_t v[7] = {per_epoch, timed, use_graph(m, knobs_of(k), per_epoch, n_epochs, timed), graph_segments(nb), r.first, r.last,
                          n_launches(m, per_epoch, n_epochs)};
    memcpy(out, v, sizeof(v));
}

// ... of a group: out[3]: timed epochs, look-ahead, use_graph
extern "C" void mf_group_epoch(const int64_t *k, int all_fast, int64_t nb, int max_timed, int64_t n_epochs, int64_t *out) {
    const MfKnobs kn = knobs_of(k);
    const long long timed = timed_epochs(max_timed, nb, n_epochs);
    const bool ahead = group_ahead(all_fast != 0, n_epochs, kn);
    const int64_t v[3] = {timed, ahead, group_use_graph(ahead, kn, nb, n_epochs, timed)};
    memcpy(out, v, sizeof(v));
}

extern "C" int mf_group_workgroups(int tpb) { return group_workgroups(tpb); }

// 0: the member fits member 0's launch, 1: another kernel instance, 2: another batch size or number of mini-batches
extern "C" int mf_group_mismatch(const int64_t *first, const int64_t *member) { return group_mismatch(shape_of(first), shape_of(member)); }

// out[4]: workgroups of a mini-batch of tpb header slots, slots per rank, workgroups of this rank, bytes per rank
extern "C" void mf_shard(const int64_t *s, int tpb, int rank, int world, int64_t *out) {
    const ShardPlan p = shard_plan(shape_of(s), tpb, rank, world);
    const int64_t v[4] = {p.wgs, p.slots_per_rank, p.rank_wgs, (int64_t)p.bytes_per_rank};
    memcpy(out, v, sizeof(v));
}

extern "C" double mf_bytes_per_sample(const int64_t *s) { return bytes_per_sample(shape_of(s)); }
