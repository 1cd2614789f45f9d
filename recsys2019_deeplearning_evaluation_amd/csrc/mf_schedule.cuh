// mf_schedule.cuh -- (row, mini-batch) incidences -> tasks: the radix-sort schedule of a whole stream and the in-LDS schedule
// (one workgroup per mini-batch; fused and pair tasks, wide lists), stream-end kernels.  Included by mf.hip after mf_core.cuh.
#pragma once

#include "mf_plan.h"

namespace mi355rec {
namespace {

// ---- schedule: (row, mini-batch) incidences -> tasks ----------------------------------------------------------------
struct SchedParams {
    long long n_samples;
    int per;                 // incidences per sample: 3 (BPR) / 2 (FunkSVD)
    int n_users, batch_size, batch_bits, tasks_per_batch;
    const int *su, *si, *sj;
    const float *sr;
    unsigned long long *keys;      // unsorted keys: entry << batch_bits | batch
    int *slots;                    // unsorted values: sample * per + role
    const unsigned long long *keys_sorted;
    const int *slots_sorted;
    int *head;                     // 1 where a new (row, batch) run starts
    const int *head_scan;          // inclusive scan of head
    int *task_at;                  // for run heads: index of the task header
    unsigned char *spar;           // per incidence: buffer of the row's version this sample reads
    unsigned char *par;            // per row: buffer of the current version (advanced by the last task of the row)
    int *batch_count;
    int *slot_flag;                // per original slot (sample * per + role): 1 where a task's first incidence sits
    const int *slot_rank;          // exclusive scan of slot_flag
    TaskHeader *tasks;
    int4 *recs;
};

__global__ __launch_bounds__(256) void mf_keys_kernel(const SchedParams s) {
    const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (t >= s.n_samples) return;
    const unsigned long long batch = (unsigned long long)(t / s.batch_size);
    const long long q = t * s.per;
    s.keys[q] = ((unsigned long long)s.su[t] << s.batch_bits) | batch;
    s.slots[q] = (int)q;
    s.keys[q + 1] = ((unsigned long long)(s.n_users + s.si[t]) << s.batch_bits) | batch;
    s.slots[q + 1] = (int)q + 1;
    if (s.per == 3) {
        s.keys[q + 2] = ((unsigned long long)(s.n_users + s.sj[t]) << s.batch_bits) | batch;
        s.slots[q + 2] = (int)q + 2;
    }
}

__global__ __launch_bounds__(256) void mf_heads_kernel(const SchedParams s) {
    const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (q >= s.n_samples * s.per) return;
    const int head = q == 0 || s.keys_sorted[q] != s.keys_sorted[q - 1];
    s.head[q] = head;
    if (head) s.slot_flag[s.slots_sorted[q]] = 1;      // (the sort is stable: the run's first incidence in stream order)
}

// One thread per run head: version parity of the row at this batch, a place in the batch's task array, the header.
__global__ __launch_bounds__(256) void mf_tasks_kernel(const SchedParams s) {
    const long long n = s.n_samples * s.per;
    const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (q >= n || !s.head[q]) return;
    const unsigned long long key = s.keys_sorted[q];
    const int entry = (int)(key >> s.batch_bits);
    const int batch = (int)(key & ((1ull << s.batch_bits) - 1));
    long long end = q + 1;
    while (end < n && !s.head[end]) ++end;
    // rank of this batch among the batches of the stream that touch the row = number of run heads since the row's first
    const unsigned long long first_key = (unsigned long long)entry << s.batch_bits;
    long long lo = 0, hi = q;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (s.keys_sorted[mid] < first_key) lo = mid + 1; else hi = mid;
    }
    const int rank = s.head_scan[q] - s.head_scan[lo];
    const int parity = (s.par[entry] + rank) & 1;
    // the task's place among the mini-batch's headers = the rank of its FIRST incidence (the sort is stable: the smallest
    // sample * per + role of the run) among the first incidences of the batch's tasks: headers are packed at the front of
    // the batch's slots in stream order -- the same layout on every replica of the stream (the exact multi-GPU mode splits a
    // mini-batch's slots over the ranks), with no atomic counter (three mini-batches of 65 536 samples used to serialise
    // 590 k atomics on three addresses: 86 M samples/s against 230 M)
    const long long first_slot = (long long)batch * s.tasks_per_batch;
    // -- or, with a per-batch counter (s.batch_count), simply the next free one: run heads arrive roughly in key order, i.e. the
    // batch's headers end up sorted by row (users first), which the mini-batch kernel of FunkSVD's 20 001 small batches likes
    // better (118 vs 87 M samples/s at ML-20M shape: neighbouring wavefronts gather neighbouring rows, and the workgroups that
    // carry global-bias terms are the leading ones)
    int at = (int)first_slot;
    if (s.batch_count) at += atomicAdd(&s.batch_count[batch], 1);
    else at += s.slot_rank[s.slots_sorted[q]] - s.slot_rank[first_slot];
    s.task_at[q] = at;
    TaskHeader h;
    h.entry = entry;
    h.meta = (int)(end - q) | (parity << 31);
    h.start = (int)q;
    h.pad = 0;
    s.tasks[at].entry = h.entry;
    s.tasks[at].meta = h.meta;
    s.tasks[at].start = h.start;
    s.tasks[at].pad = 0;
    for (long long r = q; r < end; ++r) s.spar[s.slots_sorted[r]] = (unsigned char)parity;
}

// One thread per incidence (sorted order): the sample record with the parities of all its rows.
__global__ __launch_bounds__(256) void mf_recs_kernel(const SchedParams s) {
    const long long n = s.n_samples * s.per;
    const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int slot = s.slots_sorted[q];
    const int sample = slot / s.per, role = slot - sample * s.per;
    const long long base = (long long)sample * s.per;
    int4 rec;
    rec.x = s.su[sample];
    rec.y = s.si[sample];
    rec.z = s.per == 3 ? s.sj[sample] : __float_as_int(s.sr[sample]);
    rec.w = role | (s.spar[base] << 2) | (s.spar[base + 1] << 3) | (s.per == 3 ? s.spar[base + 2] << 4 : 0);
    s.recs[q] = rec;
    if (s.head[q]) {
        s.tasks[s.task_at[q]].rec0 = rec;
        // last task of this row in the stream: the next stream starts from the other buffer
        const int entry = (int)(s.keys_sorted[q] >> s.batch_bits);
        long long end = q + 1;
        while (end < n && !s.head[end]) ++end;
        if (end == n || (int)(s.keys_sorted[end] >> s.batch_bits) != entry) s.par[entry] = s.spar[slot] ^ 1;
    }
}

// ---- fast schedule: one workgroup per mini-batch sorts its incidences in LDS -----------------------------------------------
// The general path above radix-sorts the whole stream (device-wide sort: 120 us for the 417 k incidences
// of a BPR epoch at ML-20M shape, plus 270 us for the task kernel's dependent searches) -- two thirds of the time of the 139
// mini-batches it prepares.  When a mini-batch fits LDS and the stream has at most 256 mini-batches the same tasks come out of
// three short kernels: (1) per mini-batch, a stable radix sort of (row, slot) keys in LDS, run lengths, task slots (lists longer
// than two rounds of one wavefront -- list_is_wide, mf_plan.h -- get the 4 wavefronts of a workgroup: 4 aligned headers), and one bit per (row, mini-batch) in a global bitmap;
// (2) per incidence, the version parity of each of the sample's rows = parity at stream start + number of earlier
// mini-batches with the row's bit set; (3) per row, the parity after the stream, bitmap cleared for the next one.
// BIT ROWS (the default wherever a mini-batch's bit row fits LDS beside the keys: mf_plan.h, bit_rows_fit): the bitmap is stored the
// other way round, [mini-batch][row bit].  (1) collects the mini-batch's row in LDS and writes it out once -- no global atomic, nothing
// to clear; (2') one pass down the word columns, mf_sched_parity_kernel, turns touch bits into version parities in place and moves
// par[] to the end of the stream; (3') the emit kernel reads one word per row.  Headers, records, pair records, used[], the stream
// and par[] after a stream are byte for byte those of the per-row bitmap, which remains for larger shapes and under
// MI355REC_MF_ROW_BITMAP: `touched`, one device-scope atomicOr per run (375 k per epoch at the ML-20M shape, the whole 18.7 us of
// the sort kernel's "headers" phase), row_bits / version_parity in the emit kernel, and the finish kernel behind it.
// (The limits FAST_MAX_BATCHES / FAST_MAX_SLOTS, the layout of header.meta and of qtask[], SCHED_THREADS and SCHED_STAMPS: mf_plan.h.)

struct FastSchedParams {
    long long n_samples;
    int per, n_users, n_entries, batch_size, tasks_per_batch, slot_bits, np, words, group;
    int fill_all;                 // 1: every header slot past the last one in use is zeroed (the one-model kernel launches a wavefront per slot);
                                  // 0: only up to the next multiple of 4 (the group kernel walks the slots in use, a workgroup of four wavefronts at a time)
    int mid_bytes;                // LDS bytes between the keys and the once-touched flags (run starts + header slots, or the sort's scratch)
    int entry_bits;               // bits of a row id (users, then items) + 1: the padding keys' all-ones field sorts last
    int fuse;                     // BPR: a sample whose user row is touched once in the batch takes over its other once-touched rows
    int *su, *si, *sj;
    float *sr;
    // draw = 1: the sort kernel's workgroups DRAW their mini-batch (mf_draw_sample: sample t of epoch e is a pure function of seed, e
    // and t) and store it to su/si/sj/sr, instead of reading back what a sampler launch in front of them wrote; the parity kernel
    // (per-row bitmap: the finish kernel) then advances the epoch counter (advance_epoch = 1) -- never a kernel that reads it, whose later workgroups would see the next
    // epoch.  Zero for replayed streams, schedule parts of a long stream, the group and the exact multi-GPU mode.
    int draw, advance_epoch, bpr, sample_negatives, n_items;
    float quota;
    unsigned long long seed;
    long long samples_per_epoch, first_sample;      // first_sample: index within the epoch of su[0]
    MfState *state;
    const int *indptr, *indices;
    const float *data;
    unsigned long long *ticks;    // optional [n_batches][SCHED_STAMPS] shader-clock stamps of the sort kernel's phases (thread 0 of every workgroup)
    unsigned *touched;            // [n_entries][words]: bit b of row x = mini-batch b of this stream touches x (NULL with bit rows)
    // bit rows (NULL: the per-row bitmap above): [n_batches][row_words], bit x of row b = mini-batch b touches row x as the sort kernel
    // leaves it; = buffer of row x's version in front of mini-batch b once the parity kernel has run
    unsigned *bit_rows;
    int row_words;
    unsigned char *par;           // [n_entries]: buffer of every row's current version at stream start
    int *sorted_slot;             // [n_batches][tasks_per_batch]: per batch-local incidence (sample * per + role) its position in (row, id) order | also << 16
    int *qtask;                   // per sorted position: batch-local slot of its task's (first) header | wide << 30
    int *used;                    // [n_batches]: header slots in use
    TaskHeader *tasks;
    int4 *recs;
    int4 *slot_recs;              // [n_batches][tasks_per_batch][3]: see MfParams
};

// The keys (row << slot_bits | incidence, in incidence order) only have to be grouped by row with the incidences of a row in
// stream order: a STABLE radix sort on the row bits does it in (row bits + 7) / 8 passes (rocPRIM block sort) where the bitonic
// network of round 2 needed 78 barrier-separated stages for 4096 keys (74 us per mini-batch: as much as the mini-batch itself
// once 32 models share a launch).
template <int IPT> struct SchedSort {
    using type = rocprim::block_radix_sort<unsigned, SCHED_THREADS, IPT>;
    static __device__ __forceinline__ void run(unsigned *K, void *storage, int begin_bit, int end_bit) {
        unsigned keys[IPT];
#pragma unroll
        for (int i = 0; i < IPT; ++i) keys[i] = K[threadIdx.x * IPT + i];
        type().sort(keys, *reinterpret_cast<typename type::storage_type *>(storage), (unsigned)begin_bit, (unsigned)end_bit);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < IPT; ++i) K[threadIdx.x * IPT + i] = keys[i];
    }
};
constexpr size_t sched_sort_storage_bytes(int np) {
    return np <= SCHED_THREADS ? sizeof(SchedSort<1>::type::storage_type)
           : (np <= 2 * SCHED_THREADS ? sizeof(SchedSort<2>::type::storage_type)
              : (np <= 4 * SCHED_THREADS ? sizeof(SchedSort<4>::type::storage_type) : sizeof(SchedSort<8>::type::storage_type)));
}

__device__ __forceinline__ void mf_sched_sort_body(const FastSchedParams &s, const int b) {
    extern __shared__ __attribute__((aligned(16))) unsigned sched_lds[];
    unsigned *K = sched_lds;                                   // [np] keys: row << slot_bits | incidence
    int *hpos = reinterpret_cast<int *>(sched_lds + s.np);     // [np + 1] first sorted position of every run
    int *tpos = hpos + s.np + 1;                               // [np] header slot of every task
    typedef rocprim::block_scan<int, SCHED_THREADS> Scan;
    __shared__ typename Scan::storage_type scan_tmp;
    const int tid = threadIdx.x, np = s.np, sb = s.slot_bits;
    const long long first = (long long)b * s.batch_size;
    const int n_in = (int)min((long long)s.batch_size, s.n_samples - first);
    const int m = n_in * s.per;
    auto mark = [&](int phase) {                   // (s.ticks is NULL unless stamps were asked for: a scalar branch, no stamp executes)
        if (s.ticks && tid == 0) s.ticks[(size_t)b * SCHED_STAMPS + phase] = stamp();
    };
    mark(0);
    // the mini-batch's bit row, behind the once-touched flags (its zeroes are published by the barrier behind the keys)
    unsigned *bits = reinterpret_cast<unsigned *>(reinterpret_cast<unsigned char *>(sched_lds) + sizeof(unsigned) * (size_t)np + s.mid_bytes + (size_t)np + 16);
    const bool bit_rows = s.bit_rows != nullptr;
    if (bit_rows)
        for (int w = tid; w < s.row_words; w += SCHED_THREADS) bits[w] = 0;
    if (s.draw) {
        // the workgroup draws its own mini-batch: the keys come from registers, the stream is stored for the emit kernel,
        // last_epoch_samples() and the oracle replay (the epoch word is read here and advanced by the parity / finish kernel)
        const unsigned long long sid0 = (unsigned long long)(s.state->epoch * s.samples_per_epoch + s.first_sample + first);
        for (int smp = tid; smp < n_in; smp += SCHED_THREADS) {
            int u, i, third;
            mf_draw_sample(s.bpr != 0, s.seed, sid0 + (unsigned long long)smp, s.n_users, s.n_items, s.indptr, s.indices, s.data,
                           s.sample_negatives, s.quota, u, i, third);
            const long long t = first + smp;
            s.su[t] = u;
            s.si[t] = i;
            if (s.bpr) s.sj[t] = third; else s.sr[t] = __int_as_float(third);
            const int q = smp * s.per;
            K[q] = ((unsigned)u << sb) | (unsigned)q;
            K[q + 1] = ((unsigned)(s.n_users + i) << sb) | (unsigned)(q + 1);
            if (s.per == 3) K[q + 2] = ((unsigned)(s.n_users + third) << sb) | (unsigned)(q + 2);
        }
        for (int q = m + tid; q < np; q += SCHED_THREADS) K[q] = 0xFFFFFFFFu;
    } else {
        for (int q = tid; q < np; q += SCHED_THREADS) {
            unsigned key = 0xFFFFFFFFu;
            if (q < m) {
                const int smp = q / s.per, role = q - smp * s.per;
                const long long t = first + smp;
                const int entry = role == 0 ? s.su[t] : s.n_users + (role == 1 ? s.si[t] : s.sj[t]);
                key = ((unsigned)entry << sb) | (unsigned)q;
            }
            K[q] = key;
        }
    }
    __syncthreads();
    mark(1);
    // (the sort's scratch lives where the run starts / header slots go afterwards)
    switch (np / SCHED_THREADS) {
        case 1: SchedSort<1>::run(K, hpos, sb, sb + s.entry_bits); break;
        case 2: SchedSort<2>::run(K, hpos, sb, sb + s.entry_bits); break;
        case 4: SchedSort<4>::run(K, hpos, sb, sb + s.entry_bits); break;
        default: SchedSort<8>::run(K, hpos, sb, sb + s.entry_bits); break;
    }
    __syncthreads();
    mark(2);
    // run heads -> hpos[]
    const int C = np / SCHED_THREADS;
    int cnt = 0;
    for (int c = 0; c < C; ++c) {
        const int q = tid * C + c;
        cnt += q < m && (q == 0 || (K[q] >> sb) != (K[q - 1] >> sb));
    }
    int off = 0, total = 0;
    Scan().exclusive_scan(cnt, off, 0, total, scan_tmp);
    for (int c = 0; c < C; ++c) {
        const int q = tid * C + c;
        if (q < m && (q == 0 || (K[q] >> sb) != (K[q - 1] >> sb))) hpos[off++] = q;
    }
    if (tid == 0) hpos[total] = m;
    __syncthreads();
    mark(3);
    // FUSED SAMPLE TASKS (BPR).  Most rows of a mini-batch are touched by exactly one sample (users nearly always, uniformly drawn
    // negative items mostly): as separate tasks each of them gathers the sample's three rows again -- nine row reads and three
    // wavefronts per sample.  A sample whose USER row is touched once keeps one task (the user's) which also applies the update of
    // the sample's item rows that are touched once (record bits 5 / 6: positive / negative item); those rows get no task of their
    // own.  And `group` such tasks that sit next to each other in the sorted order share one wavefront (PAIR tasks, header word 3 =
    // 1): its lane groups, which walk a list's samples `group` at a time, each take one of the samples and write that sample's
    // rows -- a single-sample task leaves all but one lane group of its wavefront idle otherwise.  The arithmetic per row is
    // unchanged.  single[q] = incidence q (sample * per + role) is alone in its run.
    unsigned char *single = reinterpret_cast<unsigned char *>(sched_lds) + sizeof(unsigned) * (size_t)np + s.mid_bytes;
    const unsigned qmask = (1u << sb) - 1u;
    if (s.fuse) {
        for (int q = tid; q < np; q += SCHED_THREADS) single[q] = 0;
        __syncthreads();
        for (int t = tid; t < total; t += SCHED_THREADS)
            if (hpos[t + 1] - hpos[t] == 1) single[K[hpos[t]] & qmask] = 1;
        __syncthreads();
    }
    auto absorbed = [&](int t) -> bool {          // a once-touched item row whose sample's user row is touched once, too
        if (!s.fuse || hpos[t + 1] - hpos[t] != 1) return false;
        const int inc = (int)(K[hpos[t]] & qmask), smp = inc / s.per;
        return inc != smp * s.per && single[smp * s.per];
    };
    auto lone_user = [&](int q) -> bool {         // sorted position q is the single-sample run of a user row
        if (q >= m) return false;
        const unsigned e = K[q] >> sb;
        return e < (unsigned)s.n_users && (q == 0 || (K[q - 1] >> sb) != e) && (q + 1 == m || (K[q + 1] >> sb) != e);
    };
    auto paired = [&](int q) -> bool {            // q lies in an aligned block of `group` positions that are all such runs
        if (!s.fuse || s.group < 2) return false;
        const int q0 = q - q % s.group;
        for (int e = 0; e < s.group; ++e)
            if (!lone_user(q0 + e)) return false;
        return true;
    };
    mark(4);
    // header slots: wide tasks first (4 aligned slots each), then the others; both in row order
    const int CT = (total + SCHED_THREADS - 1) / SCHED_THREADS;
    const int t_lo = min(tid * CT, total), t_hi = min(t_lo + CT, total);
    int wcnt = 0, acnt = 0;
    // (list_is_wide, mf_plan.h: longer than two rounds of one wavefront and than 3: split over a workgroup.  No run takes more slots
    // than it has incidences, so `used` below stays within tasks_per_batch.)
    for (int t = t_lo; t < t_hi; ++t) {
        const int start = hpos[t], len = hpos[t + 1] - start;
        wcnt += list_is_wide(len, s.group);
        acnt += absorbed(t) || (len == 1 && start % s.group != 0 && paired(start));      // runs without a header of their own
    }
    int woff = 0, n_wide = 0, aoff = 0, n_abs = 0;
    Scan().exclusive_scan(wcnt, woff, 0, n_wide, scan_tmp);
    __syncthreads();
    Scan().exclusive_scan(acnt, aoff, 0, n_abs, scan_tmp);
    mark(5);
    TaskHeader *out = s.tasks + (size_t)b * s.tasks_per_batch;
    for (int t = t_lo; t < t_hi; ++t) {
        const int start = hpos[t], len = hpos[t + 1] - start;
        const bool wide = list_is_wide(len, s.group);
        const int entry = (int)(K[start] >> sb);
        // (rows without a task advance a version, too)
        if (bit_rows) atomicOr(&bits[entry >> 5], 1u << (entry & 31));
        else atomicOr(&s.touched[(size_t)entry * s.words + (b >> 5)], 1u << (b & 31));
        const bool pair = len == 1 && paired(start);
        if (absorbed(t) || (pair && start % s.group != 0)) {
            ++aoff;
            tpos[t] = SLOT_ABSORBED;
            continue;
        }
        const int slot = wide ? 4 * woff : 4 * n_wide + (t - woff - aoff);
        woff += wide;
        tpos[t] = slot | (wide ? META_WIDE : 0) | (pair ? QTASK_PAIR : 0);
        for (int part = 0; part < header_slots(len, s.group); ++part) {
            *reinterpret_cast<int4 *>(out + slot + part) =
                make_int4(entry, (pair ? s.group : len) | (wide ? META_WIDE | (part << 28) : 0), b * s.tasks_per_batch + start, pair ? 1 : 0);
            out[slot + part].rec0 = make_int4(0, 0, 0, 0);     // (a short wide list leaves its last quarters without a record)
        }
    }
    const int used = 4 * n_wide + (total - n_wide - n_abs);
    if (tid == 0) s.used[b] = used;
    const int fill_end = s.fill_all ? s.tasks_per_batch : min(s.tasks_per_batch, (used + 3) & ~3);
    for (int slot = used + tid; slot < fill_end; slot += SCHED_THREADS)
        *reinterpret_cast<int4 *>(out + slot) = make_int4(0, 0, 0, 0);          // no samples: the slot's wavefront idles
    __syncthreads();
    if (bit_rows) {                                   // the whole row, padding included, 16 bytes a lane: nothing is ever cleared
        const uint4 *src = reinterpret_cast<const uint4 *>(bits);
        uint4 *dst = reinterpret_cast<uint4 *>(s.bit_rows + (size_t)b * s.row_words);
        for (int w = tid; w < s.row_words / 4; w += SCHED_THREADS) dst[w] = src[w];
    }
    mark(6);
    for (int q = tid; q < m; q += SCHED_THREADS) {
        int lo = 0, hi = total;                       // last run starting at or before q
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (hpos[mid] <= q) lo = mid; else hi = mid;
        }
        const int inc = (int)(K[q] & qmask);
        int also = 0;                                 // the item rows a once-touched user row's task takes over (bits 16-17 here, 5-6 of the record)
        if (s.fuse && hpos[lo + 1] - hpos[lo] == 1) {
            const int smp = inc / s.per;
            if (inc == smp * s.per) also = (single[inc + 1] ? 1 : 0) | (s.per == 3 && single[inc + 2] ? 2 : 0);
        }
        // (by INCIDENCE: the emit kernel runs one thread per sample, which looks its three incidences' sorted positions up; a scattered
        // 4-byte store into the mini-batch's 12 KB here, three coalesced loads there)
        s.sorted_slot[(size_t)b * s.tasks_per_batch + inc] = q | (also << 16);
        // (the emit kernel learns where in its run the incidence sits from here, not from the header's `start`: one dependent trip less)
        const int tp = tpos[lo];
        s.qtask[(size_t)b * s.tasks_per_batch + q] = tp == SLOT_ABSORBED ? tp : tp | (min(q - hpos[lo], QTASK_OFF_MAX) << QTASK_OFF_SHIFT);
    }
    mark(7);
}
__global__ __launch_bounds__(SCHED_THREADS) void mf_sched_sort_kernel(const FastSchedParams s) { mf_sched_sort_body(s, blockIdx.x); }

// A row's bitmap of the stream's mini-batches: FAST_MAX_BATCHES bits = 32 aligned bytes, fetched as two 16-byte loads.
struct RowBits { uint4 lo, hi; };
__device__ __forceinline__ RowBits row_bits(const FastSchedParams &s, int entry) {
    const uint4 *w = reinterpret_cast<const uint4 *>(s.touched + (size_t)entry * (FAST_MAX_BATCHES / 32));
    RowBits r;
    r.lo = w[0];
    r.hi = w[1];
    return r;
}
// buffer of the row's version that mini-batch b reads = parity at stream start + number of earlier mini-batches that touch the row
__device__ __forceinline__ int version_parity(const RowBits &r, int par, int b) {
    const unsigned w[8] = {r.lo.x, r.lo.y, r.lo.z, r.lo.w, r.hi.x, r.hi.y, r.hi.z, r.hi.w};
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {     // (b is the same for the whole workgroup: the masks are scalars)
        const unsigned mask = k < (b >> 5) ? 0xFFFFFFFFu : (k == (b >> 5) ? (1u << (b & 31)) - 1u : 0u);
        cnt += __popc(w[k] & mask);
    }
    return (par + cnt) & 1;
}

// One thread per SAMPLE (until round 6: per incidence -- every sample's ids were then fetched by three threads at three unrelated
// sorted positions and the version parities of its three rows evaluated three times over: 1.08 GB fetched per 32-model epoch).  The
// sample's ids come in coalesced, each row's parity is evaluated once, and the record goes to the sample's three sorted positions.
// Two dependent trips: (1) the sample's ids and its incidences' sorted positions; (2) everything they address, requested at once --
// the three rows' bitmaps and start parities, the incidences' qtask words and those of their aligned blocks' first positions.  The
// qtask word carries what used to be read from the header (offset within the run, "first of a pair task"); only the own-row
// buffer bit of a run's first incidence still costs a third trip, the header's meta word.
// BIT_ROWS: the parity kernel has run in front; a row's buffer bit is bit x of the mini-batch's bit row -- three 4-byte loads in the second
// trip in place of six 16-byte loads, three byte loads and the popcounts.
template <bool BIT_ROWS>
__device__ __forceinline__ void mf_sched_emit_body(const FastSchedParams &s) {
    const int b = blockIdx.y, smp = blockIdx.x * 256 + threadIdx.x;
    const long long first = (long long)b * s.batch_size;
    const int n_in = (int)min((long long)s.batch_size, s.n_samples - first);
    if (smp >= n_in) return;
    const size_t base = (size_t)b * s.tasks_per_batch;
    const long long t = first + smp;
    // (straight-line on purpose: a branch on `per` around a load makes the compiler wait for the loads in front of it.  Both
    // algorithms own all four stream buffers; a role the algorithm does not have repeats role 0 and is dropped below.)
    const bool three = s.per == 3;
    const int u = s.su[t], i = s.si[t], j = s.sj[t];
    const int rating = __float_as_int(s.sr[t]);
    int where[3];
#pragma unroll
    for (int role = 0; role < 3; ++role) where[role] = s.sorted_slot[base + (size_t)smp * s.per + (role < s.per ? role : 0)];
    const int third = three ? j : rating;
    const int ej = s.n_users + (three ? j : i);          // (FunkSVD: no third row; the item's again, unused)
    RowBits bu, bi, bj;
    int su0 = 0, si0 = 0, sj0 = 0;
    unsigned wu = 0, wi = 0, wj = 0;
    if constexpr (BIT_ROWS) {
        const unsigned *row = s.bit_rows + (size_t)b * s.row_words;
        wu = row[u >> 5]; wi = row[(s.n_users + i) >> 5]; wj = row[ej >> 5];
    } else {
        bu = row_bits(s, u); bi = row_bits(s, s.n_users + i); bj = row_bits(s, ej);
        su0 = s.par[u]; si0 = s.par[s.n_users + i]; sj0 = s.par[ej];
    }
    const int gmask = s.group - 1, gshift = s.group >> 1;       // group is 1, 2 or 4 (samples_in_flight)
    int tps[3], tps0[3];
#pragma unroll
    for (int role = 0; role < 3; ++role) {
        const int q = where[role] & 0xffff;
        tps[role] = s.qtask[base + q];
        tps0[role] = s.qtask[base + (q & ~gmask)];
    }
    int pu, pi, pj;
    if constexpr (BIT_ROWS) {
        pu = (int)((wu >> (u & 31)) & 1u);
        pi = (int)((wi >> ((s.n_users + i) & 31)) & 1u);
        pj = three ? (int)((wj >> (ej & 31)) & 1u) : 0;
    } else {
        pu = version_parity(bu, su0, b);
        pi = version_parity(bi, si0, b);
        pj = three ? version_parity(bj, sj0, b) : 0;
    }
    const int par_bits = (pu << 2) | (pi << 3) | (pj << 4);
#pragma unroll
    for (int role = 0; role < 3; ++role) {
        if (role >= s.per) break;
        const int q = where[role] & 0xffff, also = where[role] >> 16;
        const size_t at = base + q;
        const int4 rec = make_int4(u, i, third, role | par_bits | (also << 5));
        s.recs[at] = rec;
        const int tp = tps[role];
        if (tp == SLOT_ABSORBED) {
            // a sample of a PAIR task other than its first (pairs are aligned blocks of `group` sorted positions, the header belongs to the
            // first): its record also goes where the mini-batch kernel finds it without having seen the header -- by header slot
            const int q0 = q & ~gmask, tp0 = tps0[role];
            if (s.fuse && q0 != q && tp0 != SLOT_ABSORBED && (tp0 & QTASK_PAIR))
                s.slot_recs[(base + (tp0 & QTASK_SLOT_MASK)) * 3 + (q - q0 - 1)] = rec;
            continue;
        }
        TaskHeader *hd = s.tasks + base + (tp & QTASK_SLOT_MASK);
        const int off = (tp >> QTASK_OFF_SHIFT) & QTASK_OFF_MAX;      // (saturated at QTASK_OFF_MAX, past every offset asked for below)
        const int own = role == 0 ? pu : (role == 1 ? pi : pj);
        int part = -1;
        if (tp & META_WIDE) {           // quarter k of a wide list starts at position k * group
            if ((off & gmask) == 0 && (off >> gshift) < 4) part = off >> gshift;      // (quarters past the end of the list stay empty)
        } else if (off == 0) {
            part = 0;
        }
        if (part >= 0) {
            hd[part].rec0 = rec;
            // (the sort kernel left the bit clear.  An atomic OR without a return value was measured instead of this read-modify-
            // write of the one thread that owns the header: 66 k device-scope atomics per epoch made the kernel 4 us slower)
            if (own) hd[part].meta |= (int)(1u << 31);
        }
    }
}

// (a scalar branch on a kernel argument in front of everything: each side stays straight-line)
__device__ __forceinline__ void mf_sched_emit_either(const FastSchedParams &s) {
    if (s.bit_rows) mf_sched_emit_body<true>(s);
    else mf_sched_emit_body<false>(s);
}
__global__ __launch_bounds__(256) void mf_sched_emit_kernel(const FastSchedParams s) { mf_sched_emit_either(s); }

// The column pass over the bit rows (mf_plan.h: parity_load / parity_store), launched BETWEEN sort and emit in place of the finish
// kernel: a workgroup is 64 word columns (a lane each: a row of 256 bytes per access) x PARITY_PARTS wavefronts, each with one part of
// the stream's mini-batches.  One trip fetches a wavefront's touch words (and, wavefront 0, the 32 start parities of every column);
// the parts' XORs meet in LDS; a second round of stores leaves the parities and par[] after the stream.  No trip depends on another
// mini-batch's.
// Thread 0 advances the epoch word for the sort kernel's workgroups, who drew from it and have all retired (this is the next launch
// in the stream); nothing in this kernel or behind it in the schedule reads the word.
constexpr int PARITY_THREADS = 64 * PARITY_PARTS;
__device__ __forceinline__ void mf_sched_parity_body(const FastSchedParams &s, const int n_batches) {
    __shared__ unsigned part_xor[PARITY_PARTS + 1][64];         // [PARITY_PARTS]: the start parities
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    if (s.advance_epoch && blockIdx.x == 0 && threadIdx.x == 0) s.state->epoch += 1;
    const int w = blockIdx.x * 64 + lane;
    const bool live = w < s.row_words;
    unsigned *col = s.bit_rows + w;
    ParityPart p;
    unsigned total = 0;
    if (live) {
        total = parity_load(col, (size_t)s.row_words, n_batches, part, p);
        if (part == 0) part_xor[PARITY_PARTS][lane] = pack_parities(s.par, s.n_entries, w);
    }
    part_xor[part][lane] = total;
    __syncthreads();
    if (!live) return;
    unsigned running = part_xor[PARITY_PARTS][lane];
    for (int q = 0; q < part; ++q) running ^= part_xor[q][lane];
    parity_store(col, (size_t)s.row_words, n_batches, part, p, running);
    if (part == PARITY_PARTS - 1) unpack_parities(s.par, s.n_entries, w, running ^ total);
}
__global__ __launch_bounds__(PARITY_THREADS) void mf_sched_parity_kernel(const FastSchedParams s, const int n_batches) { mf_sched_parity_body(s, n_batches); }

__device__ __forceinline__ void mf_sched_finish_body(const FastSchedParams &s) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    // the epoch the sort kernel's workgroups drew is done with: every one of them has retired (this is the launch after the next)
    if (s.advance_epoch && x == 0) s.state->epoch += 1;
    if (x >= s.n_entries) return;
    unsigned *w = s.touched + (size_t)x * s.words;
    int cnt = 0;
    for (int k = 0; k < s.words; ++k) {
        const unsigned v = w[k];
        if (v) { cnt += __popc(v); w[k] = 0; }
    }
    if (cnt & 1) s.par[x] ^= 1;
}
__global__ __launch_bounds__(256) void mf_sched_finish_kernel(const FastSchedParams s) { mf_sched_finish_body(s); }

// The global-bias ring is indexed by the mini-batch's position in its STREAM (a kernel knows that from its arguments: the ring
// entry is requested together with everything else, not after the global index has arrived).  A stream of n mini-batches leaves
// the newest state and terms in entry (n - 1) % 3; mini-batch 0 of the next stream looks for them in entry 2 and adds its own
// terms to entry 0.
template <class T>
__device__ __forceinline__ void ring_to_stream_start(const MfParams<T> &p, const long long n_batches, const int slot) {
    if (n_batches <= 0) return;
    const int src = (int)((n_batches - 1) % 3);
    if (src != 2) {
        if (slot == 0) p.mu_state[2] = p.mu_state[src];
        p.mu_acc[2 * MU_SLOTS + slot] = p.mu_acc[src * MU_SLOTS + slot];
    }
    p.mu_acc[slot] = (T)0;
}

template <class T>
__global__ void mf_stream_end_kernel(const MfParams<T> p, const long long n_batches) {      // one wavefront
    if (blockIdx.x != 0) return;
    if (threadIdx.x == 0) p.state->batch_base += n_batches;
    if (threadIdx.x < MU_SLOTS) ring_to_stream_start(p, n_batches, (int)threadIdx.x);
}

template <class T>
__global__ void mf_group_stream_end_kernel(const MfParams<T> *table, const int n_models, const long long n_batches) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_models) return;
    table[m].state->batch_base += n_batches;
    for (int slot = 0; slot < MU_SLOTS; ++slot) ring_to_stream_start(table[m], n_batches, slot);
}

}  // namespace
}  // namespace mi355rec
