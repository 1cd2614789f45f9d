// The arithmetic of ease.hip and ease_pivot.hip as they stood before ease_plan.h, copied line by line behind the interface of
// tests/ease_plan_shim.cpp, with a handle of plain numbers.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

constexpr int EASE_TILE = 128;
constexpr int TILE = EASE_TILE;
constexpr int TK = 32;
constexpr int PANEL_W = 64;
constexpr int CHUNK = 64;
constexpr int GK = 16;

struct H {
    int n, npad, block, steps;
    int64_t launches;
};

static size_t ease_bytes(int64_t n, int64_t npad, int block) {
    return (size_t)(npad * npad + 3 * npad * block + (int64_t)block * block + (npad != n ? n * n : 0)) * sizeof(float);
}
static size_t pivot_bytes(int64_t npad, int block) {
    return (size_t)(npad * npad + 4 * npad * block + 2 * (int64_t)block * block) * sizeof(double);
}

// mi355rec_ease_create up to the handle's numbers; 0: refused
static int create(H *h, int n_items, int block) {
    const int64_t npad = ((int64_t)n_items + TILE - 1) / TILE * TILE;
    if (!(npad <= INT32_MAX)) return 0;
    h->n = n_items; h->npad = (int)npad; h->block = block; h->steps = (int)(npad / block);
    h->launches = 0;
    return 1;
}

extern "C" void ep_constants(int64_t *out) {
    const int64_t v[7] = {EASE_TILE, TK, PANEL_W, CHUNK, GK, (int64_t)((size_t)256 << 20), (int64_t)((size_t)64 << 20)};
    memcpy(out, v, sizeof(v));
}

extern "C" void ep_read_knobs(uint64_t *out, char *message, int room) {
    int block = TILE;
    if (const char *v = getenv("MI355REC_EASE_BLOCK")) block = atoi(v);
    const bool ok = block == 64 || block == 128;
    snprintf(message, room, "MI355REC_EASE_BLOCK must be 64 or 128, got %d", block);
    uint64_t has = 0, cap = 0;
    if (const char *v = getenv("MI355REC_EASE_PIVOT_MAX_BYTES")) {
        has = 1;
        cap = strtoull(v, nullptr, 10);
    }
    const uint64_t r[4] = {(uint64_t)(int64_t)block, ok, has, cap};
    memcpy(out, r, sizeof(r));
}

extern "C" int ep_shape(int n, int block, int64_t *out) {
    H h;
    if (!create(&h, n, block)) return 0;
    const int NB = block;
    const size_t lds_panel = (size_t)(NB * (NB + 4) + NB * PANEL_W + PANEL_W * (NB + 4)) * sizeof(float);
    const int64_t v[5] = {h.npad, h.steps, (int64_t)ease_bytes(n, h.npad, block), (int64_t)pivot_bytes(h.npad, block), (int64_t)lds_panel};
    memcpy(out, v, sizeof(v));
    return 1;
}

extern "C" int ep_ease_fit(uint64_t bytes, uint64_t free_b) {
    const size_t need = bytes + ((size_t)256 << 20);
    return need <= free_b ? 0 : 1;
}
extern "C" int ep_pivot_fit(uint64_t need, uint64_t free_b, int has_cap, uint64_t cap) {
    if (has_cap) {
        if (need > cap) return 2;
    }
    const size_t reserve = (size_t)64 << 20;
    if (need + reserve > free_b) return 1;
    return 0;
}

extern "C" void ep_ease_step(int n, int block, int step, int64_t *out) {
    H hh; H *h = &hh;
    create(h, n, block);
    const int NB = block;
    const int tiles = h->npad / TILE;
    const int k0 = step * NB;
    const int64_t v[5] = {k0, 1, h->npad / PANEL_W, tiles, h->npad / PANEL_W};
    memcpy(out, v, sizeof(v));
}
extern "C" int64_t ep_ease_launches(int n, int block) {
    H hh; H *h = &hh;
    create(h, n, block);
    h->launches += 4 * (int64_t)h->steps;
    return h->launches;
}

// enqueue_pivoted_elimination with the launches replaced by records; `want` is the step that is recorded
static void pivoted(H *h, int want, int64_t *out, int *elim) {
    const int NB = h->block;
    const int n = h->n, npad = h->npad;
    const int tiles = npad / 128, last_chunk = (n - 1) / CHUNK;
    for (int step = 0; step < h->steps; ++step) {
        const int64_t before = h->launches;
        int load = 0, swap = 0;
        const int k0 = step * NB, cols = std::min(NB, n - k0);
        if (step == want && elim)
            for (int j = 0; j < NB; ++j) elim[j] = -1;
        if (cols > 0) {
            load = last_chunk - k0 / CHUNK + 1;
            h->launches += 1;
            for (int j = 0; j < cols; ++j) {
                const int g = k0 + j;
                h->launches += 1;
                if (step == want && elim) elim[j] = 0;
                if (j + 1 < NB && g + 1 < n) {
                    if (step == want && elim) elim[j] = last_chunk - (g + 1) / CHUNK + 1;
                    h->launches += 1;
                }
            }
            swap = npad / 128;
            h->launches += 1;
        }
        h->launches += 6;
        if (step == want && out) {
            const int64_t v[10] = {k0, cols, load, swap, npad / 32, npad / 64, NB / 64, tiles, npad / PANEL_W, h->launches - before};
            memcpy(out, v, sizeof(v));
        }
    }
}

extern "C" void ep_pivot_step(int n, int block, int step, int64_t *out, int *elim) {
    H h;
    create(&h, n, block);
    pivoted(&h, step, out, elim);
}
extern "C" int64_t ep_pivot_launches(int n, int block, int gathered) {
    H h;
    create(&h, n, block);
    h.launches = 0;
    h.launches += 2;
    pivoted(&h, -1, nullptr, nullptr);
    if (gathered) h.launches += 1;
    return h.launches;
}

extern "C" void ep_inverse_permutation(const int *piv, int n, int npad, int *out) {
    std::vector<int> order((size_t)npad), inv_perm((size_t)npad);
    for (int i = 0; i < npad; ++i) order[i] = i;
    for (int g = 0; g < n; ++g)
        if (piv[g] != g) std::swap(order[g], order[piv[g]]);
    for (int l = 0; l < npad; ++l) inv_perm[order[l]] = l;
    memcpy(out, inv_perm.data(), inv_perm.size() * sizeof(int));
}

extern "C" void ep_accounting(int n, int block, int cell_bytes, double *out) {
    H hh; H *h = &hh;
    create(h, n, block);
    double v[3];
    v[0] = 2.0 * (double)h->n * h->n * h->n;
    v[1] = cell_bytes == 4 ? 8.0 * (double)h->n * h->n * h->steps : 16.0 * (double)h->n * h->n * h->steps;
    v[2] = h->steps;
    memcpy(out, v, sizeof(v));
}
