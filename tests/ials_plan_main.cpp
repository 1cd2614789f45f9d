// Stand-alone program around csrc/ials_plan.h: the tables of tests/test_ials_plan.py once more, straight through the header, with the
// properties that are about memory -- every index a plan hands to the kernels stays inside the buffer the plan sizes for it.  The test
// builds it with g++ -fsanitize=address,undefined and runs it as a child process; any finding or failed check ends it non-zero.
#include "../recsys2019_deeplearning_evaluation_amd/csrc/ials_plan.h"

#include <cstdint>
#include <cstdio>
#include <set>

using namespace mi355rec;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            ++failures;                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
        }                                                                   \
    } while (0)

static const char *const NAMES[6] = {"MI355REC_IALS_TWO_STAGE", "MI355REC_IALS_SYSTEM_GIB", "MI355REC_IALS_PART_ROWS",
                                     "MI355REC_IALS_NO_SPLIT", "MI355REC_IALS_SAME_PANEL_WAVE", "MI355REC_IALS_PHASES"};

// the knobs as read_ials_knobs() parses them with exactly these values in the environment (nullptr: unset)
static IalsKnobs knobs_with(const char *const values[6]) {
    for (int i = 0; i < 6; ++i) {
        if (values[i]) setenv(NAMES[i], values[i], 1);
        else unsetenv(NAMES[i]);
    }
    return read_ials_knobs();
}

static void environment() {
    const char *const unset[6] = {}, *const empty[6] = {"", "", "", "", "", ""}, *const zeros[6] = {"0", "0", "0", "0", "0", "0"};
    const char *const tails[6] = {" 7abc", "1e1x", "33", nullptr, nullptr, nullptr}, *const words[6] = {"yes", "much", "abc", nullptr, nullptr, nullptr};
    IalsKnobs k = knobs_with(unset);
    CHECK(k.two_stage && !k.system_gib && k.part_rows == 4096 && !k.no_split && !k.same_panel_wave && !k.phases);
    k = knobs_with(empty);
    CHECK(!k.two_stage && k.system_gib && *k.system_gib == 0.0 && k.part_rows == CHUNK && k.no_split && k.same_panel_wave && k.phases);
    k = knobs_with(zeros);
    CHECK(!k.two_stage && k.system_gib && *k.system_gib == 0.0 && k.part_rows == CHUNK && k.no_split && k.same_panel_wave && k.phases);
    k = knobs_with(tails);
    CHECK(k.two_stage && k.system_gib && *k.system_gib == 10.0 && k.part_rows == 32 && !k.no_split);
    k = knobs_with(words);
    CHECK(!k.two_stage && k.system_gib && *k.system_gib == 0.0 && k.part_rows == CHUNK);
    knobs_with(unset);
}

static void tiles() {
    std::set<int> ks = {1, 15, 16, 31, 47, 200, 207, 208, 224, 225, 239, 240, 255};
    for (int j = 1; j <= 16; ++j) ks.insert(16 * j - 1);
    for (int j = 1; j <= 15; ++j) ks.insert(16 * j);
    IalsKnobs on, off;
    off.two_stage = false;
    const auto nothing = [](auto) {};
    for (int k : ks) {
        const int nt = NT(k);
        CHECK(KT(k) >= 1 && KT(k) <= MAX_KT && nt <= MAX_NT);
        CHECK(row_slots(nt) * ROW_WAVES >= nt && dispatch_slots(RowSlots{}, row_slots(nt), nothing));
        CHECK(sizeof(double) * lds_doubles(k, 0) <= 160 * 1024);
        CHECK(!two_stage_applies(k, off) && two_stage_applies(k, on) == (k <= 207));
        if (!two_stage_applies(k, on)) continue;
        CHECK(gram_slots(nt) * GRAM_WAVES >= nt && dispatch_slots(GramSlots{}, gram_slots(nt), nothing));
        CHECK(solve_instance_slots(nt) * TILE_WAVES >= nt && dispatch_slots(SolveSlots{}, solve_instance_slots(nt), nothing));
        CHECK(sizeof(double) * lds_doubles(k, 1) <= 160 * 1024 && sizeof(double) * lds_doubles(k, 2) <= 160 * 1024);
        CHECK(slab_doubles(k, true) >= slab_doubles(k, false));
    }
    CHECK(sizeof(double) * lds_doubles(255, 1) > 160 * 1024 && !two_stage_applies(255, on));
}

// Stand-ins for the device buffers of one half-step: every slot the plan names is touched, so an index outside what the plan
// itself sizes is a finding of the address sanitizer.
static void touch_batches(const WorkPlan &w, int per_batch, int n_side) {
    const BatchPlan plan = plan_batches(w.rows, w.items, per_batch, n_side);
    CHECK(plan.items.size() == plan.sys_slot.size() && plan.items.size() == w.items.size() + w.rows.size());
    std::vector<int> slab_owner((size_t)std::min<size_t>((size_t)per_batch, w.rows.size()), -1);
    size_t at = 0;
    for (const Batch &b : plan.batches) {
        CHECK((size_t)b.gram_off == at && b.solve_off == b.gram_off + b.gram_n);
        at += (size_t)b.gram_n + (size_t)b.solve_n;
        std::fill(slab_owner.begin(), slab_owner.end(), -1);
        for (int i = b.gram_off; i < b.solve_off + b.solve_n; ++i) {
            int &owner = slab_owner[(size_t)plan.sys_slot[(size_t)i]];
            CHECK(owner == -1 || owner == plan.items[(size_t)i].x);
            owner = plan.items[(size_t)i].x;
        }
    }
    CHECK(at == plan.items.size());
}

static void work_items() {
    const char *const part_rows[4] = {nullptr, "32", "33", "1"};
    const int ranges[3][2] = {{0, 12}, {2, 9}, {5, 12}};
    for (const char *env : part_rows)
        for (int no_split = 0; no_split < 2; ++no_split) {
            const char *const values[6] = {nullptr, nullptr, env, no_split ? "1" : nullptr, nullptr, nullptr};
            const IalsKnobs knobs = knobs_with(values);
            const int P = knobs.part_rows;
            const int lengths[12] = {1, 2 * P + 1, 0, 64 * P, 2 * P, 1, 64 * P + 1, 2 * P + 1, 0, 3 * P, 65 * P, 2 * P};
            std::vector<int> ptr(13, 0), order(12);
            for (int r = 0; r < 12; ++r) {
                ptr[(size_t)r + 1] = ptr[(size_t)r] + lengths[r];
                order[(size_t)r] = r;
            }
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lengths[a] > lengths[b]; });
            for (const auto &range : ranges)
                for (int k : {16, 200}) {
                    const WorkPlan w = plan_work_items(ptr.data(), order, range[0], range[1], k, knobs);
                    std::vector<unsigned> part_count((size_t)w.part_slots, 0u), covered(12, 0u);
                    for (const WorkItem &it : w.items) {
                        CHECK(it.x >= range[0] && it.x < range[1] && it.y >= 0 && it.y < it.z && it.z <= MAX_PARTS);
                        if (it.z > 1) ++part_count[(size_t)(it.w + it.y)];      // (the slot of the part_buf slab this part writes)
                        for (int chunk : {CHUNK, GRAM_CHUNK}) {
                            const PartRange pr = part_range(ptr[(size_t)it.x], ptr[(size_t)it.x + 1], it.y, it.z, chunk);
                            CHECK(ptr[(size_t)it.x] <= pr.beg && pr.beg <= pr.end && pr.end <= ptr[(size_t)it.x + 1]);
                            if (chunk == CHUNK) covered[(size_t)it.x] += (unsigned)(pr.end - pr.beg);
                        }
                    }
                    for (unsigned c : part_count) CHECK(c == 1u);
                    for (int r : w.rows) CHECK(covered[(size_t)r] == (unsigned)lengths[r]);
                    const int n_local = (int)w.rows.size();
                    for (int per_batch : {1, 2, n_local - 1, n_local, n_local + 5})
                        if (per_batch >= 1 && n_local) touch_batches(w, per_batch, 12);
                }
        }
    const char *const unset[6] = {};
    knobs_with(unset);
    const PartRange last = part_range(7, 77, 4, 5, 32);     // 70 entries, 5 parts of 32: the last two are empty
    CHECK(last.beg == 77 && last.end == 77);
}

static void batch_sizing() {
    IalsKnobs knobs;
    CHECK(decide_system_gib(SIZE_MAX, knobs) == 8.0 && decide_system_gib((size_t)16 << 30, knobs) == 4.0 && decide_system_gib(1 << 20, knobs) == 0.001);
    knobs.system_gib = 0.0;
    CHECK(decide_system_gib(SIZE_MAX, knobs) == 0.001);
    for (int k : {16, 200, 207}) {
        CHECK(rows_per_batch(0.001, k, 10) >= 1 && rows_per_batch(8.0, k, 10) == 10);
        double gib = 8.0;
        int steps = 0;
        for (;; ++steps) {
            const int per_batch = std::min(138493, rows_per_batch(gib, k, 138493));
            const std::optional<double> smaller = halved_system_gib(per_batch, k);
            if (!smaller) {
                CHECK(per_batch <= MIN_BATCH_ROWS);
                break;
            }
            CHECK(*smaller < gib && steps < 40);
            if (steps >= 40) break;
            gib = *smaller;
        }
    }
    const HalfStepWork w = half_step_work(1000.0, 7, 9, 255);
    CHECK(w.flops > 0 && w.bytes > 0);
}

int main() {
    environment();
    tiles();
    work_items();
    batch_sizing();
    if (failures) {
        fprintf(stderr, "ials_plan_main: %d checks failed\n", failures);
        return 1;
    }
    puts("ials_plan_main: OK");
    return 0;
}
