// extern "C" wrapper around csrc/ials_plan.h for tests/test_ials_plan.py, which compiles it with g++ and calls it through ctypes:
// no GPU, no HIP runtime.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/ials_plan.h"

#include <cstdint>
#include <cstring>

using namespace mi355rec;

// The knobs as the tests pass them around, k[6]: two_stage, system_gib set, part_rows, no_split, same_panel_wave, phases; and the
// value of system_gib.
static IalsKnobs knobs_of(const int64_t *k, double gib) {
    IalsKnobs s;
    s.two_stage = k[0] != 0;
    if (k[1]) s.system_gib = gib;
    s.part_rows = (int)k[2];
    s.no_split = k[3] != 0;
    s.same_panel_wave = k[4] != 0;
    s.phases = k[5] != 0;
    return s;
}

// the process's environment, parsed
extern "C" void ials_read_knobs(int64_t *k, double *gib) {
    const IalsKnobs s = read_ials_knobs();
    const int64_t v[6] = {s.two_stage, s.system_gib.has_value(), s.part_rows, s.no_split, s.same_panel_wave, s.phases};
    memcpy(k, v, sizeof(v));
    *gib = s.system_gib.value_or(0.0);
}

extern "C" void ials_constants(int64_t *out) {
    const int64_t v[13] = {CHUNK, GRAM_CHUNK, ROW_THREADS, ROW_WAVES, TILE_WAVES, GRAM_THREADS, GRAM_WAVES, MAX_KT, MAX_NT, MAX_SOLVE_SLOTS,
                           TP, MAX_PARTS, MIN_BATCH_ROWS};
    memcpy(out, v, sizeof(v));
}

// out[12]: KT, NT, row_slots, gram_slots, solve_slots, solve_instance_slots, two_stage_applies, LDS doubles of stage 0 / 1 / 2, slab
// doubles of a two-stage / a one-kernel epoch
extern "C" void ials_tiles(int k, const int64_t *knobs, int64_t *out) {
    const int nt = NT(k);
    const int64_t v[12] = {KT(k), nt, row_slots(nt), gram_slots(nt), solve_slots(nt), solve_instance_slots(nt),
                           two_stage_applies(k, knobs_of(knobs, 0.0)), (int64_t)lds_doubles(k, 0), (int64_t)lds_doubles(k, 1),
                           (int64_t)lds_doubles(k, 2), (int64_t)slab_doubles(k, true), (int64_t)slab_doubles(k, false)};
    memcpy(out, v, sizeof(v));
}

// is there a kernel instance with n tile slots?  which: 0 ials_row_kernel<n, 0, 512>, 1 ials_row_kernel<n, 1, 1024>, 2 ials_solve_kernel<n>
extern "C" int ials_has_instance(int which, int n) {
    int hit = 0;
    const auto note = [&](auto slots) { hit = decltype(slots)::value; };
    const bool found = which == 0 ? dispatch_slots(RowSlots{}, n, note) : (which == 1 ? dispatch_slots(GramSlots{}, n, note) : dispatch_slots(SolveSlots{}, n, note));
    return found && hit == n;
}

extern "C" double ials_system_gib(uint64_t free_bytes, const int64_t *knobs, double gib) {
    return decide_system_gib((size_t)free_bytes, knobs_of(knobs, gib));
}

extern "C" int ials_rows_per_batch(double system_gib, int k, uint64_t longest_side) { return rows_per_batch(system_gib, k, (size_t)longest_side); }

// The batches ensure_systems() tries for half-steps of `rows` rows when no allocation succeeds: per_batch[i] slabs with the buffer size
// gib[i], until halved_system_gib() says stop.  -> how many (-1: more than cap)
extern "C" int ials_halving(int rows, double system_gib, int k, uint64_t longest_side, int64_t *per_batch, double *gib, int cap) {
    for (int n = 0; n < cap; ++n) {
        per_batch[n] = std::min(std::max(1, rows), rows_per_batch(system_gib, k, (size_t)longest_side));
        gib[n] = system_gib;
        const std::optional<double> smaller = halved_system_gib((int)per_batch[n], k);
        if (!smaller) return n + 1;
        system_gib = *smaller;
    }
    return -1;
}

// counts[4]: warm rows, items, split rows, part slots.  rows_out has room for every row of `order`, items_out for cap items of 4.
// -> 0, or -1 if the items do not fit
extern "C" int ials_work_items(const int32_t *ptr, const int32_t *order, int n_order, int r0, int r1, int k, const int64_t *knobs, int32_t *rows_out,
                               int32_t *items_out, int cap, int64_t *counts, double *nnz_rows) {
    const WorkPlan w = plan_work_items(ptr, std::vector<int>(order, order + n_order), r0, r1, k, knobs_of(knobs, 0.0));
    if ((int)w.items.size() > cap) return -1;
    std::copy(w.rows.begin(), w.rows.end(), rows_out);
    static_assert(sizeof(WorkItem) == 4 * sizeof(int32_t), "four ints");
    if (!w.items.empty()) memcpy(items_out, w.items.data(), sizeof(WorkItem) * w.items.size());
    counts[0] = (int64_t)w.rows.size();
    counts[1] = (int64_t)w.items.size();
    counts[2] = w.n_split;
    counts[3] = w.part_slots;
    *nnz_rows = w.nnz_rows;
    return 0;
}

// items_out / sys_slot_out: cap items; batches_out: cap_batches x {gram_off, gram_n, solve_off, solve_n}; counts[2]: items, batches.
// -> 0, or -1 if something does not fit
extern "C" int ials_batches(const int32_t *rows, int n_rows, const int32_t *items, int n_items, int per_batch, int n_side, int32_t *items_out,
                            int32_t *sys_slot_out, int cap, int32_t *batches_out, int cap_batches, int64_t *counts) {
    std::vector<WorkItem> in((size_t)n_items);
    if (n_items) memcpy(in.data(), items, sizeof(WorkItem) * (size_t)n_items);
    const BatchPlan plan = plan_batches(std::vector<int>(rows, rows + n_rows), in, per_batch, n_side);
    if ((int)plan.items.size() > cap || (int)plan.batches.size() > cap_batches || plan.sys_slot.size() != plan.items.size()) return -1;
    if (!plan.items.empty()) memcpy(items_out, plan.items.data(), sizeof(WorkItem) * plan.items.size());
    std::copy(plan.sys_slot.begin(), plan.sys_slot.end(), sys_slot_out);
    for (size_t b = 0; b < plan.batches.size(); ++b) {
        const Batch &t = plan.batches[b];
        const int32_t v[4] = {t.gram_off, t.gram_n, t.solve_off, t.solve_n};
        memcpy(batches_out + 4 * b, v, sizeof(v));
    }
    counts[0] = (int64_t)plan.items.size();
    counts[1] = (int64_t)plan.batches.size();
    return 0;
}

extern "C" void ials_part_range(int beg, int end, int part, int n_parts, int chunk, int32_t *out) {
    const PartRange r = part_range(beg, end, part, n_parts, chunk);
    out[0] = r.beg;
    out[1] = r.end;
}

extern "C" void ials_accounting(double nnz_rows, int n_local, int n_other, int k, double *out) {
    const HalfStepWork w = half_step_work(nnz_rows, n_local, n_other, k);
    out[0] = w.flops;
    out[1] = w.bytes;
}
