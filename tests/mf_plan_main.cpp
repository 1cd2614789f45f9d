// Stand-alone program around csrc/mf_plan.h, straight through the header.  It runs tables of its own, smaller than those of
// tests/test_mf_plan.py (streams of up to 600 mini-batches), so that it can check the properties that are about memory -- every index a
// plan hands to the kernels stays inside the buffer the plan sizes for it, held in real arrays -- plus that file's cases at the integer
// limits (keys of 64 | 65 bits, 2^31 incidences, rows at the int limit), where the arithmetic itself is what the sanitizer watches.  The
// test builds it with g++ -fsanitize=address,undefined and runs it as a child process; any finding or failed check ends it non-zero.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/mf_plan.h"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace mi355rec;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++failures;                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
        }                                                                   \
    } while (0)

static const char *const NAMES[7] = {"MI355REC_MF_GENERAL_SCHEDULE", "MI355REC_MF_NO_FUSE", "MI355REC_MF_WHOLE_STREAM_SCHEDULE", "MI355REC_MF_TICKS",
                                     "MI355REC_MF_GROUP_PER_MEMBER_SCHEDULE", "MI355REC_MF_GROUP_NO_LOOKAHEAD", "MI355REC_NO_GRAPH"};

static int knobs_on(const MfKnobs &k) {
    return k.general_schedule + k.no_fuse + k.whole_stream_schedule + k.ticks + k.group_per_member_schedule + k.group_no_lookahead + k.no_graph;
}

static void environment() {
    for (const char *name : NAMES) unsetenv(name);
    CHECK(knobs_on(read_mf_knobs()) == 0);
    for (const char *value : {"", "0", "1"}) {
        for (const char *name : NAMES) setenv(name, value, 1);
        CHECK(knobs_on(read_mf_knobs()) == 7);
    }
    for (const char *name : NAMES) unsetenv(name);
    setenv(NAMES[2], "", 1);
    const MfKnobs k = read_mf_knobs();
    CHECK(k.whole_stream_schedule && knobs_on(k) == 1);
    unsetenv(NAMES[2]);
}

static MfShape shape(int algorithm, int n_users, int n_items, long long nnz, int k, bool f64, int batch_size, bool fast) {
    MfShape s;
    s.algorithm = algorithm;
    s.n_users = n_users;
    s.n_items = n_items;
    s.nnz = nnz;
    s.k = k;
    s.f64 = f64;
    s.batch_size = batch_size;
    s.fast_schedule = fast;
    return s;
}

static void widths() {
    for (int f64 = 0; f64 < 2; ++f64)
        for (int k = 1; k <= 520; ++k) {
            const WidthChoice c = row_width(k, f64 != 0);
            int lpr = 0, ki = 0;
            const bool found = dispatch_width(c.klass, [&](auto l, auto i) { lpr = decltype(l)::value, ki = decltype(i)::value; });
            CHECK(found == (c.klass >= 0) && c.klass >= -1 && c.klass < 4);
            if (!found) continue;
            const int vec = vec_of(f64 != 0);
            // the instance covers the row: LPR lanes x KI chunks x VEC factors; a wavefront's lanes are 64 / LPR samples
            CHECK(lpr == c.lpr && ki == c.ki && lpr * ki * vec >= k && k % vec == 0 && c.in_flight == 64 / lpr);
        }
    CHECK(widest_chunks(RowWidths{}) == 128);
    CHECK(!dispatch_width(4, [](auto, auto) {}) && !dispatch_width(-1, [](auto, auto) {}));
}

// Stand-ins for the device buffers of one stream: every element a schedule and its mini-batches name is touched, so an index outside
// what buffer_plan() sizes is a finding of the address sanitizer.
static void touch_stream(const MfShape &s0, const MfKnobs &knobs, long long n_samples, long long n_batches, bool whole_stream) {
    const BufferPlan plan = buffer_plan(s0, knobs, (size_t)n_samples, n_batches, whole_stream);
    MfShape s = s0;
    s.fast_schedule = plan.fast1;
    const long long tpb = tasks_per_batch(s), span = whole_stream ? n_batches : schedule_span(s, knobs, n_batches);
    std::vector<char> samples((size_t)n_samples), tasks(plan.tasks), recs(plan.recs), slot_recs(plan.slot_recs), used(plan.used), batch_count(plan.batch_count);
    long long ends = 0, scheduled = 0;
    for (long long b = 0; b < n_batches; ++b) {
        const StreamStep st = stream_step(n_samples, n_batches, span, s.batch_size, false, b);
        if (st.sched != SCHED_NONE) {
            CHECK(st.sched == (span == n_batches ? SCHED_WHOLE : SCHED_PART));
            const bool fast = runs_fast_schedule(s, knobs, st.sched_batches);
            CHECK(fast || plan.general);                                    // the radix-sort schedule only runs where its buffers were planned
            for (long long i = 0; i < st.sched_samples; i += std::max<long long>(1, st.sched_samples - 1)) samples[(size_t)(st.sample_offset + i)] = 1;
            samples[(size_t)(st.sample_offset + st.sched_samples - 1)] = 1;
            tasks[(size_t)(st.sched_batches * tpb - 1)] = 1;                // headers of the schedule's last mini-batch
            recs[(size_t)(st.sched_batches * tpb - 1)] = 1;
            if (fast) used[(size_t)(st.sched_batches - 1)] = 1;
            else batch_count[(size_t)(st.sched_batches - 1)] = 1;
            scheduled += st.sched_batches;
        }
        // what launch_batch_as addresses for this mini-batch
        tasks[(size_t)((st.local + 1) * tpb - 1)] = 1;
        slot_recs[(size_t)(st.local * slot_rec_stride(s) + 3 * tpb - 1)] = 1;
        if (reads_used_slots(s, knobs) && n_batches == batches_per_epoch(s)) used[(size_t)st.local] = 1;
        ends += st.end_batches;
    }
    CHECK(ends == n_batches && scheduled == n_batches);
}

static void streams() {
    MfKnobs off, whole, general;
    whole.whole_stream_schedule = true;
    general.general_schedule = true;
    for (long long nb : {1, 139, 256, 257, 600})
        for (int algorithm : {MI355REC_MF_BPR, MI355REC_MF_FUNK_SVD})
            for (int k : {64, 10})
                for (const MfKnobs &knobs : {off, whole, general})
                    for (int whole_stream = 0; whole_stream < 2; ++whole_stream) {
                        const int B = 7;
                        const MfShape s = shape(algorithm, (int)(nb - 1) * B, 50, (nb - 1) * B, k, false, B, false);
                        CHECK(batches_per_epoch(s) == nb);
                        touch_stream(s, knobs, nb * B, nb, whole_stream != 0);
                        touch_stream(s, knobs, (nb - 1) * B + 1, nb, whole_stream != 0);      // a replayed stream with a short last mini-batch
                    }
    const BufferPlan asy = buffer_plan(shape(MI355REC_MF_ASY_SVD, 10, 10, 100, 8, false, 1, false), off, 101, 101, false);
    CHECK(asy.asy && asy.tasks == 0 && !asy.general);
    const StreamStep none = stream_step(10, 3, 3, 4, false, 1);
    CHECK(none.sched == SCHED_NONE && none.local == 1 && none.end_batches == 0);
}

static void sort_workgroups() {
    for (int tpb : {1, 3, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8190, 8192}) {
        const int np = sched_np(tpb);
        CHECK(np >= tpb && np >= SCHED_THREADS && (np & (np - 1)) == 0 && np <= FAST_MAX_SLOTS);
        for (size_t storage : {(size_t)0, sizeof(unsigned) * (2 * (size_t)np + 1) + 4, (size_t)70000}) {
            // the sort kernel's LDS: [np] keys | middle: [np + 1] run starts + [np] header slots, or the sort's scratch | [np] flag bytes
            std::vector<char> lds(sched_lds_bytes(np, storage));
            const size_t mid = sched_mid_bytes(np, storage), keys = sizeof(unsigned) * (size_t)np;
            CHECK(mid % 16 == 0 && mid >= storage);
            lds[keys + sizeof(unsigned) * (2 * (size_t)np + 1) - 1] = 1;
            if (storage) lds[keys + storage - 1] = 1;
            lds[keys + mid + (size_t)np - 1] = 1;
        }
    }
    MfKnobs off;
    const FastSchedNumbers f = fast_sched_numbers(shape(MI355REC_MF_BPR, 1 << 20, 1 << 20, 1, 64, false, 100, true), off, 100);
    CHECK(f.slot_bits + f.entry_bits <= 32 && f.fuse == 1 && f.group == 4 && f.words * 32 == FAST_MAX_BATCHES);
}

// a run never takes more header slots than it has incidences (a mini-batch has one slot and one wavefront per incidence); the
// threshold of the instances with 2 and 4 samples in flight is "longer than two rounds"
static void header_slot_rule() {
    for (int group : {1, 2, 4})
        for (int len = 1; len <= 8192; ++len) {
            CHECK(header_slots(len, group) <= len);
            CHECK(header_slots(len, group) == (list_is_wide(len, group) ? 4 : 1));
            if (group > 1) CHECK(list_is_wide(len, group) == (len > 2 * group));
        }
    CHECK(!list_is_wide(3, 1) && list_is_wide(4, 1));
}

static void epochs_and_shards() {
    MfKnobs off;
    for (long long nb : {1ll, 10ll, GRAPH_SEGMENT, GRAPH_SEGMENT + 1, 20001ll, MAX_GRAPH_BATCHES}) {
        std::vector<char> covered((size_t)nb, 0);
        for (long long i = 0; i < graph_segments(nb); ++i) {
            const BatchRange r = graph_segment(nb, i);
            CHECK(r.first < r.last && r.last - r.first <= GRAPH_SEGMENT);
            for (long long b = r.first; b < r.last; ++b) ++covered[(size_t)b];
        }
        for (char c : covered) CHECK(c == 1);
    }
    CHECK(timed_epochs(0, 10, 5) == 0 && timed_epochs(11, 10, 5) == 2 && timed_epochs(11, 10, 1) == 1);
    CHECK(group_ahead(true, 2, off) && !group_ahead(true, 1, off) && !group_ahead(false, 2, off));
    const MfShape s = shape(MI355REC_MF_BPR, 100, 100, 1000, 20, true, 10, true);
    for (int tpb : {1, 4, 5, 3000})
        for (int world : {1, 2, 3, 8}) {
            int total = 0;
            for (int rank = 0; rank < world; ++rank) {
                const ShardPlan p = shard_plan(s, tpb, rank, world);
                std::vector<char> slab(p.bytes_per_rank);       // this rank's rows: 4 slots per workgroup, k doubles each
                if (p.rank_wgs) slab[(size_t)p.rank_wgs * 4 * s.k * sizeof(double) - 1] = 1;
                total += p.rank_wgs;
            }
            CHECK(total == (tpb + 3) / 4);
        }
    CHECK(group_workgroups(3000) == 250 && group_workgroups(1) == 1);
    CHECK(n_launches(shape(MI355REC_MF_ASY_SVD, 1, 1, ASY_CHUNK, 8, false, 1, false), ASY_CHUNK + 1, 3) == 6);
}

// the cases of tests/test_mf_plan.py that sit at an integer limit (no arrays here: the arithmetic is what is checked)
static void integer_limits() {
    const int big = 2147483647;
    const MfShape rows = shape(MI355REC_MF_BPR, big, big, 1, 64, false, 1000, false);
    const GeneralSched at64 = general_sched(rows, 1ll << 32), at65 = general_sched(rows, (1ll << 32) + 1);
    CHECK(at64.end_bit == 64 && at64.fits && at65.end_bit == 65 && !at65.fits);
    MfKnobs off;
    CHECK(!fast_schedule_fits(rows, off, 1) && batches_per_epoch(rows) == big / 1000 + 1);
    const MfShape funk = shape(MI355REC_MF_FUNK_SVD, 1000, 1000, 1ll << 30, 10, false, 1024, false);     // any-k: the radix-sort schedule
    const BufferPlan below = buffer_plan(funk, off, ((size_t)1 << 30) - 1, 1 << 20, false), at = buffer_plan(funk, off, (size_t)1 << 30, 1 << 20, false);
    CHECK(below.general && below.incidences == ((size_t)1 << 31) - 2 && below.incidences_fit);
    CHECK(at.general && at.incidences == (size_t)1 << 31 && !at.incidences_fit);
    CHECK(at.tasks == (((size_t)1 << 20) + 1) * 2048 && at.recs == ((size_t)1 << 20) * 2048);
    const StreamStep last = stream_step((1ll << 30) - 1, 1 << 20, 1 << 20, 1024, false, (1 << 20) - 1);
    CHECK(last.local == (1 << 20) - 1 && last.end_batches == 1 << 20);
    CHECK(widest_chunks(RowWidths{}) * vec_of(false) == 512 && widest_chunks(RowWidths{}) * vec_of(true) == 256);
}

int main() {
    environment();
    widths();
    streams();
    sort_workgroups();
    header_slot_rule();
    epochs_and_shards();
    integer_limits();
    if (failures) {
        fprintf(stderr, "mf_plan_main: %d checks failed\n", failures);
        return 1;
    }
    puts("mf_plan_main: OK");
    return 0;
}
