// extern "C" wrapper around csrc/slim_plan.h for tests/test_slim_plan.py, which compiles it with g++ and calls it through ctypes:
// no GPU, no HIP runtime.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/slim_plan.h"

#include <cstdint>
#include <cstring>

using namespace mi355rec;

// The integer knobs as the tests pass them around, k[14]: nap, no_presched, prof, inject_abort, sym_spare_cus, sym_wgs set / value,
// sym_long_wgs set / value, owners, cus set / value, owner_min_steps, no_owner_gate.
static SlimKnobs knobs_of(const int64_t *k) {
    SlimKnobs s;
    s.nap = (int)k[0];
    s.no_presched = k[1] != 0;
    s.prof = k[2] != 0;
    s.inject_abort = k[3] != 0;
    s.sym_spare_cus = (int)k[4];
    if (k[5]) s.sym_wgs = (int)k[6];
    if (k[7]) s.sym_long_wgs = (int)k[8];
    s.owners = (int)k[9];
    if (k[10]) s.cus = (int)k[11];
    s.owner_min_steps = (int)k[12];
    s.no_owner_gate = k[13] != 0;
    return s;
}

// the process's environment, parsed: k[14] as above, the gate's wait in seconds, the lock directory
extern "C" void slim_read_knobs(int64_t *k, double *wait_s, char *dir, int cap) {
    const SlimKnobs s = read_slim_knobs();
    const int64_t v[14] = {s.nap, s.no_presched, s.prof, s.inject_abort, s.sym_spare_cus, s.sym_wgs.has_value(), s.sym_wgs.value_or(0),
                           s.sym_long_wgs.has_value(), s.sym_long_wgs.value_or(0), s.owners, s.cus.has_value(), s.cus.value_or(0),
                           s.owner_min_steps, s.no_owner_gate};
    memcpy(k, v, sizeof(v));
    *wait_s = s.gate_wait_s;
    strncpy(dir, s.lock_dir.c_str(), (size_t)cap - 1);
    dir[cap - 1] = 0;
}

extern "C" void slim_constants(int64_t *out) {
    const int64_t v[8] = {LOSS_SLOTS, FLOW_THREADS, FLOW_WAVES, FLOW_REGS, FLOW_BLOCK, MAX_OWNERS, LQ_CHUNK, LQ_RING};
    memcpy(out, v, sizeof(v));
}

extern "C" void slim_sym_launch(int cus, int per_cu, int ahead, int n, int n_short, const int64_t *k, int64_t *out) {
    const SymLaunch g = plan_sym_launch(cus, per_cu, ahead != 0, n, n_short, knobs_of(k));
    out[0] = g.long_wgs;
    out[1] = g.grid;
}

extern "C" void slim_dense_plan(int n_items, int sparse_weights, int cus, const int64_t *k, int64_t *out) {
    const DensePlan p = plan_dense_launch(n_items, sparse_weights != 0, cus, knobs_of(k));
    out[0] = p.wanted;
    out[1] = p.want_slots;
    out[2] = (int64_t)p.row_bytes;
}

extern "C" void slim_dense_grid(int slots, int cus, int blocks_per_cu_no_lds, int64_t row_bytes, const int64_t *k, int64_t *out) {
    const DenseGrid g = dense_grid(slots, cus, blocks_per_cu_no_lds, (size_t)row_bytes, knobs_of(k));
    const int64_t v[6] = {g.owners, (int64_t)g.lds, g.grid, g.max_owners, g.min_steps, g.needs_lds_attribute};
    memcpy(out, v, sizeof(v));
}

// -> number of segments (-1: more than cap); out [cap][3] = first, count, prune_after
extern "C" int slim_segments(int n, int sparse_weights, int64_t *out, int cap) {
    const std::vector<Segment> segments = sparse_segments(n, sparse_weights != 0);
    if ((int)segments.size() > cap) return -1;
    for (size_t i = 0; i < segments.size(); ++i) {
        out[3 * i] = segments[i].first;
        out[3 * i + 1] = segments[i].count;
        out[3 * i + 2] = segments[i].prune_after;
    }
    return (int)segments.size();
}

extern "C" int slim_bits_for(uint64_t n_values) { return bits_for(n_values); }

extern "C" uint64_t slim_roomy(uint64_t nnz, int n, int n_users, int64_t n_cells) { return roomy_cell_capacity((size_t)nnz, n, n_users, n_cells); }

// bit 0: flow_supported, bit 1: schedules_ahead
extern "C" int slim_flow_modes(int sparse_weights, int symmetric, int n_items, const int64_t *k) {
    return (flow_supported(symmetric != 0, n_items) ? 1 : 0) | (schedules_ahead(sparse_weights != 0, symmetric != 0, n_items, knobs_of(k)) ? 2 : 0);
}
