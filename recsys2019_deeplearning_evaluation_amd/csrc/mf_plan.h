// mf_plan.h -- the host arithmetic of a BPR-MF / FunkSVD / AsySVD call: the environment's switches (MfKnobs, parsed in ONE place), the
// table "row width k -> instance of the mini-batch kernel", which schedule a stream takes and how a long stream is cut into parts, the
// numbers of the in-LDS and the radix-sort schedule, the element counts of the stream buffers, the walk over the mini-batches of a
// stream, what an epoch call replays as graphs, the group's and the exact multi-GPU mode's numbers, the accounting -- and the
// constants the kernels share with it.
// Plain C++17 on plain numbers (MfShape) -- no HIP call, no rocPRIM; the size of the block sort's LDS scratch comes in as an argument --
// so g++ builds it and tests/test_mf_plan.py runs it without a GPU.  Included by mf.hip and by the mf_*.cuh headers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "../../include/mi355rec.h"

namespace mi355rec {
namespace {

// functions the kernels call, too
#if defined(__HIPCC__)
#define MI355REC_HD __host__ __device__
#define MI355REC_UNROLL _Pragma("unroll")
#else
#define MI355REC_HD
#define MI355REC_UNROLL
#endif

// ---- constants shared with the kernels -------------------------------------------------------------------------------------------
// one L2 atomic per workgroup that carries global-bias terms: atomics on ONE address retire at about 0.2 us each (measured through
// the batch kernel: 31 per address cost 3 us per mini-batch), so the terms are spread over a wavefront's worth of addresses
constexpr int MU_SLOTS = 64;
constexpr int META_WIDE = 1 << 30;        // header.meta: bits 0-27 list length, 28-29 quarter, 30 wide, 31 buffer of the own row
constexpr int SCHED_THREADS = 1024;
constexpr int SLOT_ABSORBED = 0x3fffffff;   // qtask[] of an incidence whose row is updated by its sample's user task (no header of its own)
constexpr int FAST_MAX_BATCHES = 256, FAST_MAX_SLOTS = 8192;
// qtask[] of every other incidence: bits 0-12 the header slot (< FAST_MAX_SLOTS), bits 13-17 the incidence's offset within its run
// (saturated: the emit kernel asks for offsets 0 .. 4 * group - 1 <= 15 only), bit 29 the run is the first of a pair task, bit 30 wide
constexpr int QTASK_SLOT_MASK = FAST_MAX_SLOTS - 1, QTASK_OFF_SHIFT = 13, QTASK_OFF_MAX = 31, QTASK_PAIR = 1 << 29;
constexpr int SCHED_STAMPS = 8;           // per workgroup of the sort kernel: entry, keys, sort, run heads, once-touched flags, slot scans, headers, exit
constexpr int ASY_KMAX = 256;
constexpr int ASY_CHUNK = 1 << 16;        // steps per launch of the ordered AsySVD kernel (keeps single launches short)
// An epoch is captured into graphs of up to GRAPH_SEGMENT mini-batches.  FunkSVD's epoch at the ML-20M shape is 20 001 mini-batches:
// as plain launches the host's launch rate (8.8 us per mini-batch) was the bound, not the chain of kernels.
constexpr long long GRAPH_SEGMENT = 4096, MAX_GRAPH_BATCHES = 64 * GRAPH_SEGMENT;

// ---- the environment ------------------------------------------------------------------------------------------------------------
// The MI355REC_MF_* switches (and MI355REC_NO_GRAPH) as one ABI call sees them (TICKS: as the create call saw it): read when the call
// begins, because tests create handles under different settings in one process.  Every one of them is on as soon as the variable
// exists, whatever it holds, an empty string included.
struct MfKnobs {
    bool general_schedule = false;            // GENERAL_SCHEDULE: the radix-sort schedule for every stream
    bool no_fuse = false;                     // NO_FUSE: one task per row (no fused sample tasks, no pair tasks)
    bool whole_stream_schedule = false;       // WHOLE_STREAM_SCHEDULE: a long stream is scheduled in one piece, not FAST_MAX_BATCHES at a time
    bool ticks = false;                       // TICKS: shader-clock stamps of the mini-batch and the sort kernel's phases
    bool group_per_member_schedule = false;   // GROUP_PER_MEMBER_SCHEDULE: a group's members sample and schedule on their own streams
    bool group_no_lookahead = false;          // GROUP_NO_LOOKAHEAD: the group's next schedule does not run beside the mini-batches
    bool no_graph = false;                    // MI355REC_NO_GRAPH: plain launches only (rocprofv3 on ROCm 7.2 crashes while tracing graph replays)
    bool row_bitmap = false;                  // ROW_BITMAP: the in-LDS schedule keeps the per-row bitmap built by global atomics (no bit rows)
};

// the only place of mf.hip and its headers that reads the environment
inline MfKnobs read_mf_knobs() {
    const auto is_set = [](const char *name) { return getenv(name) != nullptr; };
    MfKnobs k;
    k.general_schedule = is_set("MI355REC_MF_GENERAL_SCHEDULE");
    k.no_fuse = is_set("MI355REC_MF_NO_FUSE");
    k.whole_stream_schedule = is_set("MI355REC_MF_WHOLE_STREAM_SCHEDULE");
    k.ticks = is_set("MI355REC_MF_TICKS");
    k.group_per_member_schedule = is_set("MI355REC_MF_GROUP_PER_MEMBER_SCHEDULE");
    k.group_no_lookahead = is_set("MI355REC_MF_GROUP_NO_LOOKAHEAD");
    k.no_graph = is_set("MI355REC_NO_GRAPH");
    k.row_bitmap = is_set("MI355REC_MF_ROW_BITMAP");
    return k;
}

// ---- what a decision needs of a handle --------------------------------------------------------------------------------------------
struct MfShape {
    int algorithm = MI355REC_MF_BPR;
    int n_users = 0, n_items = 0;
    long long nnz = 0;
    int k = 0;
    bool f64 = false;
    int batch_size = 1;
    bool sharded = false;           // inside an exact multi-GPU epoch
    // The handle's CACHED decision for the in-LDS schedule: fast_schedule_fits(.., 1) as the call that allocated the task tables saw
    // it.  fast_schedule_fits() below is a FRESH decision of every call.  Known hazard, kept as it is: when
    // MI355REC_MF_GENERAL_SCHEDULE appears between two calls on one handle the two disagree -- slot_rec_stride() stays non-zero
    // while the radix-sort schedule, which fills one mini-batch of pair records at most, runs.  Nothing toggles the switch during a
    // handle's life.
    bool fast_schedule = false;
    // The handle's CACHED decision for the bit rows of the in-LDS schedule (bit_rows_fit as the call that allocated the task tables saw
    // it); false: the per-row bitmap `touched`, global atomics and the finish kernel.
    bool bit_rows = false;
};

inline int bits_for(unsigned long long n_values) {   // bits needed for values 0 .. n_values - 1 (at least 1)
    int b = 1;
    while (b < 63 && (1ull << b) < n_values) ++b;
    return b;
}
inline int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}
inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

inline int per_sample(const MfShape &s) { return s.algorithm == MI355REC_MF_BPR ? 3 : 2; }   // rows a sample touches
inline int tasks_per_batch(const MfShape &s) { return per_sample(s) * s.batch_size; }
inline long long batches_per_epoch(const MfShape &s) {
    // .pyx:583 (BPR: n_users / B + 1) and :289 (FunkSVD: nnz / B + 1); ASY_SVD: nnz / 1 + 1 single-sample steps (.pyx:397)
    const long long B = s.batch_size;
    return (s.algorithm == MI355REC_MF_BPR ? (long long)s.n_users / B : s.nnz / B) + 1;
}

// ---- row width -> instance of the mini-batch kernel ---------------------------------------------------------------------------------
// A row of k factors is k / VEC chunks of 16 bytes (VEC = 16 / sizeof(T)).  The compiled instances of mf_batch_kernel and
// mf_group_batch_kernel, narrowest first: rows of at most MAX_CHUNKS chunks run on LPR lanes per row with KI chunks per lane, and a
// wavefront works on IN_FLIGHT samples of a task's list at a time.  Rows that are no whole number of chunks, or wider than the last
// instance, run on the any-k kernel (mf_batch_generic_kernel), which has no replica-batched form and does not split wide lists.
// (Measured and rejected, round 4: rows of 17 .. 32 chunks on 16 lanes with two chunks each instead of 32 lanes with one -- four samples
// per wavefront, twice the bytes in flight per wavefront: the row gathers of a wavefront took 3 840 cycles instead of 2 350, one model
// 140 M samples/s instead of 176 M, the 32-model group 567 M instead of 678 M.)
template <int MAX_CHUNKS, int LPR, int KI, int IN_FLIGHT>
struct Width {
    static constexpr int max_chunks = MAX_CHUNKS, lpr = LPR, ki = KI, in_flight = IN_FLIGHT;
};
template <class... W>
struct Widths {};
using RowWidths = Widths<Width<16, 16, 1, 4>, Width<32, 32, 1, 2>, Width<64, 64, 1, 1>, Width<128, 64, 2, 1>>;

struct WidthChoice {
    int klass;              // position of the instance in RowWidths; -1: the any-k kernel
    int lpr, ki, in_flight;
};
inline int vec_of(bool f64) { return f64 ? 2 : 4; }
template <class... W>
WidthChoice choose_width(Widths<W...>, int k, int vec) {
    WidthChoice c{-1, 0, 0, 1};
    if (k % vec != 0) return c;
    const int chunks = k / vec;
    int at = 0;
    (void)((chunks <= W::max_chunks ? (c = WidthChoice{at, W::lpr, W::ki, W::in_flight}, true) : (++at, false)) || ...);
    return c;
}
inline WidthChoice row_width(int k, bool f64) { return choose_width(RowWidths{}, k, vec_of(f64)); }
// the widest row (in chunks) that has an instance
template <class... W>
constexpr int widest_chunks(Widths<W...>) { return std::max({W::max_chunks...}); }

// dispatch_width() calls f(std::integral_constant<int, LPR>, std::integral_constant<int, KI>) for the instance at position `klass`
// and says whether there is one: the launch code picks its template instance this way, so the table is written once.  Head first,
// then the rest: the compiler instantiates f's bodies, and so the kernels they name, narrowest first, which is the order the kernels
// have in the code object (a fold over W... instantiates them widest first and moves every kernel's address).
template <class W0, class... W, class F>
bool dispatch_width(Widths<W0, W...>, int klass, F &&f) {
    if (klass == 0) {
        f(std::integral_constant<int, W0::lpr>{}, std::integral_constant<int, W0::ki>{});
        return true;
    }
    if constexpr (sizeof...(W) > 0) return dispatch_width(Widths<W...>{}, klass - 1, std::forward<F>(f));
    else return false;
}
template <class F>
bool dispatch_width(int klass, F &&f) { return dispatch_width(RowWidths{}, klass, std::forward<F>(f)); }

// samples of a task's list a wavefront of the mini-batch kernel works on at a time
inline int samples_in_flight(const MfShape &s) { return row_width(s.k, s.f64).in_flight; }

// ---- which schedule a stream takes ------------------------------------------------------------------------------------------------
// The in-LDS schedule holds a stream of n_batches mini-batches: (see MfShape::fast_schedule for the cached twin of this decision)
inline bool fast_schedule_fits(const MfShape &s, const MfKnobs &knobs, long long n_batches) {
    const int tpb = tasks_per_batch(s);
    return !knobs.general_schedule && n_batches <= FAST_MAX_BATCHES && tpb <= FAST_MAX_SLOTS &&
           bits_for((unsigned long long)s.n_users + s.n_items) + bits_for((unsigned long long)std::max(tpb, SCHED_THREADS)) <= 31 &&
           row_width(s.k, s.f64).klass >= 0;    // the any-k kernel does not split wide lists
}

// Mini-batches per schedule.  A stream the in-LDS schedule cannot hold at once (more than FAST_MAX_BATCHES mini-batches: FunkSVD's
// epoch at the ML-20M shape has 20 001) is scheduled and run FAST_MAX_BATCHES mini-batches at a time, each part a stream of its
// own (its end moves the global batch index and the global-bias ring on): three schedule launches per 256 mini-batch launches,
// against the radix-sort schedule of the whole stream they keep the split of long lists over a workgroup (a list of 10
// held the kernel for 14 000 cycles where the median wavefront took 7 300), headers and records in 16 MB that stay cached instead of
// 1.9 GB, and 1.5 GB of sort buffers are never allocated.  Whole stream: when it fits, when the in-LDS schedule is not available
// for this handle, and in the exact multi-GPU mode (its exchange walks one schedule).
inline long long schedule_span(const MfShape &s, const MfKnobs &knobs, long long n_batches) {
    if (!s.sharded && n_batches > FAST_MAX_BATCHES && fast_schedule_fits(s, knobs, 1) && !knobs.whole_stream_schedule) return FAST_MAX_BATCHES;
    return n_batches;
}

// A native epoch whose whole stream goes through ONE in-LDS schedule is drawn by that schedule's workgroups (FastSchedParams::draw):
// no sampler launch, no epoch-advance launch, no read-back of the stream.  Everything else keeps the sampler launch: replayed streams,
// streams scheduled FAST_MAX_BATCHES mini-batches at a time, the radix-sort schedule, the group, the exact multi-GPU mode, AsySVD.
inline bool schedule_draws(const MfShape &s, const MfKnobs &knobs) {
    const long long nb = batches_per_epoch(s);
    return s.algorithm != MI355REC_MF_ASY_SVD && !s.sharded && s.fast_schedule && fast_schedule_fits(s, knobs, nb) &&
           schedule_span(s, knobs, nb) == nb;
}
// the stream of n_batches mini-batches goes through the in-LDS schedule in one piece
inline bool runs_fast_schedule(const MfShape &s, const MfKnobs &knobs, long long n_batches) {
    return s.fast_schedule && fast_schedule_fits(s, knobs, n_batches);
}

// ---- the in-LDS schedule's numbers --------------------------------------------------------------------------------------------------
inline int sched_np(int tpb) { return std::max(SCHED_THREADS, pow2_at_least(tpb)); }      // keys a workgroup sorts: a power of two
// LDS between the keys and the once-touched flags: run starts + header slots (2 np + 1 words) | the block sort's scratch, whose size
// (sched_sort_storage_bytes(np) in mf_schedule.cuh) only rocPRIM knows
inline size_t sched_mid_bytes(int np, size_t sort_storage_bytes) {
    const size_t middle = std::max(sizeof(unsigned) * (2 * (size_t)np + 1), sort_storage_bytes);
    return (middle + 15) & ~(size_t)15;
}
// keys, middle, one byte per incidence for the once-touched flags
inline size_t sched_lds_bytes(int np, size_t sort_storage_bytes) {
    return sizeof(unsigned) * (size_t)np + sched_mid_bytes(np, sort_storage_bytes) + (size_t)np + 16;
}

// HEADER SLOTS.  A run (the incidences of one row in one mini-batch) of `len` samples is WIDE when it is longer than two rounds of one
// wavefront, which works on `group` samples at a time (samples_in_flight): it is split over the 4 wavefronts of a workgroup and takes 4
// aligned header slots, every other run takes one (absorbed rows and the later runs of a pair task: none).  A mini-batch has as many
// header slots as incidences (tasks_per_batch) and the mini-batch launch one wavefront per slot, so a run must never take more slots
// than it has incidences: header_slots(len, group) <= len.  On the instances with one sample in flight a list of 3 is therefore NOT
// wide (it runs three rounds on one wavefront) -- with `len > 2 * group` alone it took 4 slots, and FunkSVD's mini-batch of three samples
// with one item and three users 7 of its 6: the last header went into the next mini-batch's slots, where no wavefront of its launch ran.
MI355REC_HD inline bool list_is_wide(int len, int group) { return len > (2 * group > 3 ? 2 * group : 3); }
MI355REC_HD inline int header_slots(int len, int group) { return list_is_wide(len, group) ? 4 : 1; }

struct FastSchedNumbers {
    int np, slot_bits, entry_bits, mid_bytes, words, group, fuse, fill_all;
    int row_words, bit_rows;    // words of a mini-batch's bit row; 1: the schedule runs on bit rows (both 0 from fast_sched_numbers)
};
inline FastSchedNumbers fast_sched_numbers(const MfShape &s, const MfKnobs &knobs, size_t sort_storage_bytes) {
    FastSchedNumbers f{};
    f.np = sched_np(tasks_per_batch(s));
    f.slot_bits = bits_for((unsigned long long)f.np);
    f.entry_bits = std::min(32 - f.slot_bits, bits_for((unsigned long long)(s.n_users + s.n_items)) + 1);
    f.mid_bytes = (int)sched_mid_bytes(f.np, sort_storage_bytes);
    f.words = FAST_MAX_BATCHES / 32;
    f.group = samples_in_flight(s);
    // fused sample tasks: BPR only; not in the exact multi-GPU mode, whose exchange slabs hold one row per task slot
    f.fuse = s.algorithm == MI355REC_MF_BPR && !s.sharded && !knobs.no_fuse;
    f.fill_all = 1;
    return f;
}

// ---- bit rows: which buffer holds a row's version at mini-batch b, without atomics ---------------------------------------------------
// A workgroup of the sort kernel is one mini-batch, so bit b of every row is written by workgroup b alone: stored [mini-batch][row bit]
// the workgroup collects its mini-batch's touch bits in LDS and writes the row out once, coalesced.  One pass down the word columns
// (parity_load / parity_store below) turns the touch bits into version parities in place and carries par[] to the end of the
// stream; the emit kernel then reads one word per row.  The other layout -- touched[row][FAST_MAX_BATCHES / 32], one device-scope
// atomicOr per run, a finish kernel that scans and clears it, eight masked popcounts per row in the emit kernel -- remains for shapes
// whose bit row does not fit LDS and under MI355REC_MF_ROW_BITMAP.
//
// words of one mini-batch's bit row: a multiple of 4, so that rows are 16-byte aligned and move 16 bytes at a time
inline int bit_row_words(long long n_entries) { return (int)((ceil_div(n_entries, 32) + 3) / 4 * 4); }
// LDS of the sort kernel with a bit row behind the once-touched flags (sched_lds_bytes is a multiple of 16)
inline size_t sched_lds_bytes_bit_rows(int np, size_t sort_storage_bytes, long long n_entries) {
    return sched_lds_bytes(np, sort_storage_bytes) + sizeof(unsigned) * (size_t)bit_row_words(n_entries);
}
// keys + middle + flags + bit row + the kernel's static LDS stay within the device's limit per workgroup
inline bool bit_rows_fit(const MfShape &s, const MfKnobs &knobs, size_t sort_storage_bytes, size_t static_lds_bytes, size_t lds_limit) {
    if (knobs.row_bitmap) return false;
    const int np = sched_np(tasks_per_batch(s));
    return sched_lds_bytes_bit_rows(np, sort_storage_bytes, (long long)s.n_users + s.n_items) + static_lds_bytes <= lds_limit;
}
// fast_sched_numbers with the handle's cached decision (MfShape::bit_rows)
inline FastSchedNumbers fast_sched_numbers_bit_rows(const MfShape &s, const MfKnobs &knobs, size_t sort_storage_bytes) {
    FastSchedNumbers f = fast_sched_numbers(s, knobs, sort_storage_bytes);
    f.row_words = bit_row_words((long long)s.n_users + s.n_items);
    f.bit_rows = s.bit_rows ? 1 : 0;
    return f;
}

// The column pass.  Word column w of the bit rows holds rows 32 w .. 32 w + 31; down the column, the word of mini-batch b is
// replaced by `running` (the buffer of each row's version in front of b) and `running ^= touch word`.  The mini-batches of a stream
// are cut into PARITY_PARTS consecutive parts of parity_part_len() each: a part's loads are independent of one another, its XOR is
// all the later parts need of it.  The kernel gives a part to a wavefront (a lane per column, the XORs meet in LDS); parity_column()
// walks the parts in turn -- the same functions, which is what tests/test_mf_bit_rows_plan.py runs.
constexpr int PARITY_PARTS = 16, PARITY_PART_MAX = FAST_MAX_BATCHES / PARITY_PARTS;
struct ParityPart {
    unsigned t[PARITY_PART_MAX];
};
MI355REC_HD inline int parity_part_len(int n_batches) { return (n_batches + PARITY_PARTS - 1) / PARITY_PARTS; }   // <= PARITY_PART_MAX
// the touch words of part `part` of the column at `col` (row stride in words), and their XOR
MI355REC_HD inline unsigned parity_load(const unsigned *col, size_t stride, int n_batches, int part, ParityPart &p) {
    const int len = parity_part_len(n_batches), b0 = part * len;
    unsigned total = 0;
    MI355REC_UNROLL
    for (int i = 0; i < PARITY_PART_MAX; ++i) {
        const int b = b0 + i;
        p.t[i] = i < len && b < n_batches ? col[(size_t)b * stride] : 0u;
        total ^= p.t[i];
    }
    return total;
}
// ... replaced by the parities in front of each of the part's mini-batches; `running`: in front of the part's first
MI355REC_HD inline void parity_store(unsigned *col, size_t stride, int n_batches, int part, const ParityPart &p, unsigned running) {
    const int len = parity_part_len(n_batches), b0 = part * len;
    MI355REC_UNROLL
    for (int i = 0; i < PARITY_PART_MAX; ++i) {
        const int b = b0 + i;
        if (i < len && b < n_batches) col[(size_t)b * stride] = running;
        running ^= p.t[i];
    }
}
// (on the device par[] is an allocation of its own: 32 rows' bytes are 16-byte aligned and move as two 16-byte accesses)
template <class P>
MI355REC_HD inline P *parity_bytes(P *at) {
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<P *>(__builtin_assume_aligned(at, 16));
#else
    return at;
#endif
}
// par[] (one byte per row, 0 / 1) of rows 32 w .. 32 w + 31 as a word; the last word of a row is partial, the padding words are empty
MI355REC_HD inline unsigned pack_parities(const unsigned char *par, long long n_entries, int w) {
    const long long x0 = 32ll * w;
    unsigned v = 0;
    if (x0 + 32 <= n_entries) {
        unsigned q[8];                        // four bytes a word: bit 0 of each byte -> one nibble
        __builtin_memcpy(q, parity_bytes(par + x0), 32);
    MI355REC_UNROLL
        for (int k = 0; k < 8; ++k) v |= ((q[k] & 1u) | ((q[k] >> 7) & 2u) | ((q[k] >> 14) & 4u) | ((q[k] >> 21) & 8u)) << (4 * k);
    } else {
        for (int i = 0; i < 32 && x0 + i < n_entries; ++i) v |= (unsigned)(par[x0 + i] & 1) << i;
    }
    return v;
}
MI355REC_HD inline void unpack_parities(unsigned char *par, long long n_entries, int w, unsigned v) {
    const long long x0 = 32ll * w;
    if (x0 + 32 <= n_entries) {
        unsigned q[8];
    MI355REC_UNROLL
        for (int k = 0; k < 8; ++k) {
            const unsigned n = v >> (4 * k);
            q[k] = (n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21);
        }
        __builtin_memcpy(parity_bytes(par + x0), q, 32);
    } else {
        for (int i = 0; i < 32 && x0 + i < n_entries; ++i) par[x0 + i] = (unsigned char)((v >> i) & 1);
    }
}
// one column, part after part
inline void parity_column(unsigned *rows, int row_words, int n_batches, unsigned char *par, long long n_entries, int w) {
    ParityPart parts[PARITY_PARTS];
    unsigned total[PARITY_PARTS];
    for (int part = 0; part < PARITY_PARTS; ++part) total[part] = parity_load(rows + w, (size_t)row_words, n_batches, part, parts[part]);
    unsigned running = pack_parities(par, n_entries, w);
    for (int part = 0; part < PARITY_PARTS; ++part) {
        parity_store(rows + w, (size_t)row_words, n_batches, part, parts[part], running);
        running ^= total[part];
    }
    unpack_parities(par, n_entries, w, running);
}

// pair records per mini-batch the mini-batch kernel steps over (0: it reads one mini-batch of zeros, see BufferPlan::slot_recs)
inline long long slot_rec_stride(const MfShape &s) { return s.fast_schedule ? 3ll * tasks_per_batch(s) : 0; }
// the kernels read the per-batch count of header slots in use (only the replica-batched launch sizes its grid below the slot count;
// it runs whole epochs, i.e. batches_per_epoch mini-batches)
inline bool reads_used_slots(const MfShape &s, const MfKnobs &knobs) { return runs_fast_schedule(s, knobs, batches_per_epoch(s)); }

// ---- the radix-sort schedule's numbers ------------------------------------------------------------------------------------------------
struct GeneralSched {
    int batch_bits, end_bit;    // key = row << batch_bits | mini-batch; the sort runs over bits [0, end_bit)
    bool fits;                  // end_bit <= 64
    // placement of the headers inside a batch: by rank (reproducible layout) for the exact multi-GPU mode and for batches too large
    // for the in-LDS schedule; by counter for streams of many small batches (see mf_tasks_kernel)
    bool by_rank;
};
inline GeneralSched general_sched(const MfShape &s, long long n_batches) {
    GeneralSched g{};
    g.batch_bits = bits_for((unsigned long long)n_batches);
    g.end_bit = g.batch_bits + bits_for((unsigned long long)s.n_users + s.n_items);
    g.fits = g.end_bit <= 64;
    g.by_rank = s.sharded || tasks_per_batch(s) > FAST_MAX_SLOTS;
    return g;
}

// ---- buffers ------------------------------------------------------------------------------------------------------------------------
// Element counts of what a stream of n_samples in n_batches mini-batches needs.  `whole_stream`: the caller schedules the stream in
// one piece whatever its length (group members, exact multi-GPU mode).
struct BufferPlan {
    bool asy;                   // AsySVD: the four stream arrays and nothing else
    bool fast1;                 // the in-LDS schedule is available to this handle (becomes MfShape::fast_schedule)
    bool general;               // the radix-sort schedule will see this stream: its buffers are needed
    size_t incidences;          // ... of this many elements each,
    bool incidences_fit;        // which must stay below 2^31
    // headers and records: per mini-batch of a SCHEDULE (a long stream on the in-LDS schedule reuses FAST_MAX_BATCHES of them)
    long long table_batches;
    size_t tasks, recs, batch_count;
    size_t slot_recs;           // (the mini-batch kernel reads a slot's pair records whatever the schedule: without the in-LDS schedule one mini-batch of zeros)
    size_t sorted_slot, qtask, used, touched;       // in-LDS schedule only (0 without it)
    size_t bit_rows;            // in-LDS schedule on bit rows: mini-batches of one schedule x row words (`touched` is 0 then)
};
inline BufferPlan buffer_plan(const MfShape &s, const MfKnobs &knobs, size_t n_samples, long long n_batches, bool whole_stream) {
    BufferPlan b{};
    b.asy = s.algorithm == MI355REC_MF_ASY_SVD;
    if (b.asy) return b;
    b.fast1 = fast_schedule_fits(s, knobs, 1);
    whole_stream = whole_stream || knobs.whole_stream_schedule;
    b.general = !b.fast1 || (whole_stream && !fast_schedule_fits(s, knobs, n_batches));
    b.incidences = n_samples * (size_t)per_sample(s);
    b.incidences_fit = b.incidences < (1ull << 31);
    b.table_batches = b.general ? n_batches : std::min<long long>(n_batches, FAST_MAX_BATCHES);
    const size_t tpb = (size_t)tasks_per_batch(s), tb = (size_t)b.table_batches;
    b.batch_count = tb;
    b.tasks = (tb + 1) * tpb;
    b.recs = tb * tpb;              // records of batch b start at b * tpb in both schedule paths
    b.slot_recs = 3 * tpb * (b.fast1 ? tb : 1);
    if (b.fast1) {
        b.sorted_slot = b.qtask = tb * tpb;
        b.used = tb;
        b.touched = ((size_t)s.n_users + s.n_items) * (FAST_MAX_BATCHES / 32);
    }
    return b;
}
// buffer_plan with the handle's cached decision (MfShape::bit_rows): the bit rows of one schedule in place of the per-row bitmap
inline BufferPlan buffer_plan_bit_rows(const MfShape &s, const MfKnobs &knobs, size_t n_samples, long long n_batches, bool whole_stream) {
    BufferPlan b = buffer_plan(s, knobs, n_samples, n_batches, whole_stream);
    if (b.fast1 && s.bit_rows) {
        b.touched = 0;
        b.bit_rows = (size_t)std::min<long long>(b.table_batches, FAST_MAX_BATCHES) * (size_t)bit_row_words((long long)s.n_users + s.n_items);
    }
    return b;
}
inline size_t loss_slot_count(const MfShape &s) { return (size_t)tasks_per_batch(s) * 4; }
inline size_t tick_count(const MfShape &s) { return (size_t)tasks_per_batch(s) * 8; }                // mini-batch kernel: per wavefront
inline size_t sched_tick_count() { return (size_t)FAST_MAX_BATCHES * SCHED_STAMPS; }                 // sort kernel: per workgroup

// ---- the walk over a stream's mini-batches ----------------------------------------------------------------------------------------
// What goes with mini-batch b of a stream of n_samples in n_batches mini-batches that is scheduled `span` mini-batches at a time
// (schedule_span): its index inside its schedule, the schedule enqueued in front of it, the stream end behind it.
enum SchedKind { SCHED_NONE = 0, SCHED_DRAW, SCHED_WHOLE, SCHED_PART };
struct StreamStep {
    int local;                          // batch-local index: the mini-batch kernel's argument
    SchedKind sched;                    // DRAW: one span on the in-LDS schedule, which draws the samples (schedule_draws)
    long long sample_offset, sched_samples, sched_batches;      // of the schedule (PART: a stream of its own inside the buffers)
    long long end_batches;              // > 0: a stream end of that many mini-batches follows
};
inline StreamStep stream_step(long long n_samples, long long n_batches, long long span, long long batch_size, bool draw, long long b) {
    const long long part = b / span * span, local = b - part, part_batches = std::min(span, n_batches - part);
    StreamStep st{(int)local, SCHED_NONE, 0, n_samples, n_batches, local + 1 == part_batches ? part_batches : 0};
    if (local != 0) return st;
    st.sched = draw ? SCHED_DRAW : (span == n_batches ? SCHED_WHOLE : SCHED_PART);
    if (st.sched == SCHED_PART) {
        st.sample_offset = part * batch_size;
        st.sched_samples = std::min(n_samples - part * batch_size, part_batches * batch_size);
        st.sched_batches = part_batches;
    }
    return st;
}

// ---- an epoch call ------------------------------------------------------------------------------------------------------------------
// epochs whose mini-batch launches carry timing events run as plain launches, the rest replays the graph
inline long long timed_epochs(int max_timed, long long per_epoch, long long n_epochs) {
    return max_timed > 0 ? std::min<long long>(n_epochs, (max_timed + per_epoch - 1) / per_epoch) : 0;
}
inline bool use_graph(const MfShape &s, const MfKnobs &knobs, long long per_epoch, long long n_epochs, long long timed) {
    return per_epoch <= MAX_GRAPH_BATCHES && n_epochs - timed > 0 && !knobs.no_graph && s.algorithm != MI355REC_MF_ASY_SVD;
}
// the graphs of one epoch: segment i holds mini-batches [first, last)
inline long long graph_batches(const MfShape &s) { return s.algorithm == MI355REC_MF_ASY_SVD ? 1 : batches_per_epoch(s); }
inline long long graph_segments(long long nb) { return ceil_div(nb, GRAPH_SEGMENT); }
struct BatchRange {
    long long first, last;
};
inline BatchRange graph_segment(long long nb, long long i) { return {i * GRAPH_SEGMENT, std::min(nb, (i + 1) * GRAPH_SEGMENT)}; }

// The group.  Look-ahead: the schedule of epoch e + 1 runs on a second stream beside the mini-batches of epoch e (every member on
// the in-LDS schedule, more than one epoch in the call); otherwise the epoch is one graph of at most GRAPH_SEGMENT mini-batches.
inline bool group_ahead(bool all_fast, long long n_epochs, const MfKnobs &knobs) { return all_fast && n_epochs > 1 && !knobs.group_no_lookahead; }
inline bool group_use_graph(bool ahead, const MfKnobs &knobs, long long per_epoch, long long n_epochs, long long timed) {
    return !ahead && per_epoch <= GRAPH_SEGMENT && n_epochs - timed > 0 && !knobs.no_graph;
}
// a third of the slots' workgroups: the kernel loops over the slots in use (all of them when a member is on the general schedule)
inline int group_workgroups(int tpb) { return (int)ceil_div(ceil_div(tpb, 4), 3); }
// What ONE launch must share: the kernel instance and the grid; everything else is per model.
enum GroupMismatch { GROUP_OK = 0, GROUP_OTHER_INSTANCE, GROUP_OTHER_BATCHES };
inline GroupMismatch group_mismatch(const MfShape &first, const MfShape &member) {
    if (member.algorithm != first.algorithm || member.f64 != first.f64 || row_width(member.k, member.f64).klass != row_width(first.k, first.f64).klass)
        return GROUP_OTHER_INSTANCE;
    if (tasks_per_batch(member) != tasks_per_batch(first) || batches_per_epoch(member) != batches_per_epoch(first)) return GROUP_OTHER_BATCHES;
    return GROUP_OK;
}

// The exact multi-GPU mode: workgroup w of a mini-batch's `wgs` (four header slots each) runs on rank w % world.
struct ShardPlan {
    int wgs;
    int slots_per_rank;         // whole workgroups: a wide list's four quarters stay together
    int rank_wgs;               // workgroups of this rank (0 when wgs <= rank)
    size_t bytes_per_rank;      // of the exchange slabs
};
inline ShardPlan shard_plan(const MfShape &s, int tpb, int rank, int world) {
    ShardPlan p{};
    p.wgs = (int)ceil_div(tpb, 4);
    p.slots_per_rank = (int)ceil_div(p.wgs, world) * 4;
    p.rank_wgs = p.wgs > rank ? (p.wgs - rank + world - 1) / world : 0;
    p.bytes_per_rank = (size_t)p.slots_per_rank * s.k * (s.f64 ? sizeof(double) : sizeof(float));
    return p;
}

// ---- accounting -----------------------------------------------------------------------------------------------------------------
// ALGORITHMIC lower bound of DESIGN.md section 4: every row a sample touches is read once and written once
// (3 rows for BPR, 2 for FunkSVD), fp32.
inline double bytes_per_sample(const MfShape &s) {
    const double rows = s.algorithm == MI355REC_MF_BPR ? 3.0 : 2.0;   // (AsySVD: its profile-sized term is added per call)
    return rows * 2.0 * 4.0 * (double)s.k;
}
// launches of the dominant kernel: `times` streams of n_batches mini-batches -- or, AsySVD, of n_batches steps in chunks of ASY_CHUNK
inline long long n_launches(const MfShape &s, long long n_batches, long long times) {
    return s.algorithm == MI355REC_MF_ASY_SVD ? times * ceil_div(n_batches, ASY_CHUNK) : n_batches * times;
}

}  // namespace
}  // namespace mi355rec
