// states_main.cpp — the record <-> array conversion and the validity check of ctf_states.h (what k_export_states / k_import_states
// run per record) on the host, as a stand-alone program under AddressSanitizer + UBSan: every buffer is a heap block of exactly
// the size the ABI promises, so a byte read or written past a row, a record or a pad is caught.
//
// For (N, G) = (2, 4), (8, 15), (16, 32) and groups of 1, 15, 16 and 17 records it checks that
//   - states_pack writes the bytes ctf_set_state's host code writes (restated below from ctf_device.h's layout: hp | pos | has_flag
//     | perm | i16 inventory | pad | misc[4], unused bytes zero; grid padded with zeros to GS; u8 maps widened into u32 [N][GS]),
//     with and without the optional arrays, as one "lane" and as 16 lanes taking strided work items;
//   - states_unpack of what was packed gives the arrays back (pack -> unpack is the identity), rows of other records untouched;
//   - states_check accepts every good row and refuses one bad value per rule.
// Exit status 0 = all of it held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctf_states.h"

static int g_fail = 0;
#define EXPECT(c)                                                            \
    do {                                                                     \
        if (!(c)) {                                                          \
            if (g_fail++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
        }                                                                    \
    } while (0)

static uint32_t g_rng = 12345u;
static uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

static int round_up(int x, int a) { return (x + a - 1) / a * a; }

// the layout, restated (ctf_device.h: the record's fields in order, RS and GS multiples of 16)
static StateShape shape_of(int N, int G, int log_metrics) {
    StateShape S;
    S.n_envs = 64, S.N = N, S.G = G, S.GG = G * G, S.GS = round_up(G * G, 16);
    S.off_pos = 8 * N, S.off_flag = 10 * N, S.off_perm = 11 * N, S.off_inv = 12 * N, S.off_misc = round_up(14 * N, 4);
    S.RS = round_up(S.off_misc + 16, 16);
    S.log_metrics = log_metrics;
    return S;
}

struct Heap {  // exactly-sized arrays of n records
    StateArrays a;
    Heap(const StateShape& S, int n, bool metrics, bool vis) {
        for (int f = 0; f < ST_FIELDS; f++) {
            const bool want = f < ST_METRICS || (f == ST_METRICS && metrics) || (f == ST_VIS && vis);
            a.arr[f] = want ? (uint8_t*)malloc((size_t)n * st_row_bytes(S, f)) : nullptr;
            if (want) memset(a.arr[f], 0xA5, (size_t)n * st_row_bytes(S, f));
        }
    }
    ~Heap() {
        for (int f = 0; f < ST_FIELDS; f++) free(a.arr[f]);
    }
};

static void fill_valid(const StateShape& S, StateArrays& a, int n) {
    const int N = S.N;
    for (int k = 0; k < n; k++) {
        for (int c = 0; c < S.GG; c++) a.arr[ST_GRID][(size_t)k * S.GG + c] = (uint8_t)(rnd() % 14);
        for (int i = 0; i < N; i++) {
            const size_t r = (size_t)k * N + i;
            ((int8_t*)a.arr[ST_POS])[2 * r] = (int8_t)(rnd() % S.G);
            ((int8_t*)a.arr[ST_POS])[2 * r + 1] = (int8_t)(rnd() % S.G);
            const double hp = (double)(rnd() % 1000) / 7.0 - 3.0;
            memcpy(a.arr[ST_HP] + 8 * r, &hp, 8);
            a.arr[ST_FLAG][r] = (uint8_t)(rnd() & 1);
            const int32_t inv = (int32_t)(rnd() % 1001);
            memcpy(a.arr[ST_INV] + 4 * r, &inv, 4);
            a.arr[ST_PERM][r] = (uint8_t)(rnd() % N);
        }
        const int32_t step = k == 0 ? (1 << 28) - 1 : (int32_t)(rnd() % 5000), caps[2] = {(int32_t)(rnd() % 9), (int32_t)(rnd() % 9)};
        memcpy(a.arr[ST_STEP] + 4 * (size_t)k, &step, 4);
        memcpy(a.arr[ST_CAPS] + 8 * (size_t)k, caps, 8);
        a.arr[ST_DONE][k] = (uint8_t)(rnd() % 3 == 0 ? 1 + rnd() % 255 : 0);
        if (a.arr[ST_METRICS])
            for (int w = 0; w < CTF_N_METRICS * N; w++) {
                const int32_t v = (int32_t)(rnd() % 100000) - 5;
                memcpy(a.arr[ST_METRICS] + 4 * ((size_t)k * CTF_N_METRICS * N + w), &v, 4);
            }
        if (a.arr[ST_VIS])
            for (int w = 0; w < N * S.GG; w++) a.arr[ST_VIS][(size_t)k * N * S.GG + w] = (uint8_t)rnd();
    }
}

// what ctf_set_state writes for row k (restated from its host code)
static void reference_bytes(const StateShape& S, const StateArrays& a, int k, std::vector<uint8_t>& rec, std::vector<uint8_t>& grid,
                            std::vector<int32_t>& met, std::vector<uint32_t>& vis) {
    const int N = S.N;
    rec.assign((size_t)S.RS, 0), grid.assign((size_t)S.GS, 0);
    memcpy(grid.data(), a.arr[ST_GRID] + (size_t)k * S.GG, (size_t)S.GG);
    for (int i = 0; i < N; i++) {
        const size_t r = (size_t)k * N + i;
        memcpy(rec.data() + 8 * i, a.arr[ST_HP] + 8 * r, 8);
        rec[S.off_pos + 2 * i] = a.arr[ST_POS][2 * r];
        rec[S.off_pos + 2 * i + 1] = a.arr[ST_POS][2 * r + 1];
        rec[S.off_flag + i] = a.arr[ST_FLAG][r];
        rec[S.off_perm + i] = a.arr[ST_PERM][r];
        int32_t inv32;
        memcpy(&inv32, a.arr[ST_INV] + 4 * r, 4);
        const int16_t inv = (int16_t)inv32;
        memcpy(rec.data() + S.off_inv + 2 * i, &inv, 2);
    }
    int32_t step, caps[2];
    memcpy(&step, a.arr[ST_STEP] + 4 * (size_t)k, 4);
    memcpy(caps, a.arr[ST_CAPS] + 8 * (size_t)k, 8);
    const bool maps = S.log_metrics && a.arr[ST_VIS];
    const int32_t misc[4] = {step, caps[0], caps[1], (a.arr[ST_DONE][k] ? CTF_F_DONE : 0) | (maps ? 0 : CTF_F_BASE_ZERO) | (int32_t)((uint32_t)step << CTF_F_FOLDED_SHIFT)};
    memcpy(rec.data() + S.off_misc, misc, 16);
    met.assign((size_t)CTF_N_METRICS * N, 0);
    if (a.arr[ST_METRICS]) memcpy(met.data(), a.arr[ST_METRICS] + 4 * (size_t)k * CTF_N_METRICS * N, met.size() * 4);
    vis.assign((size_t)N * S.GS, 0);
    if (a.arr[ST_VIS])
        for (int i = 0; i < N; i++)
            for (int c = 0; c < S.GG; c++) vis[(size_t)i * S.GS + c] = a.arr[ST_VIS][((size_t)k * N + i) * S.GG + c];
}

static bool check_all(const StateShape& S, const StateArrays& a, int k, int nt) {
    bool ok = true;
    for (int t = 0; t < nt; t++) ok = states_check(S, a, (size_t)k, t, nt) && ok;  // (every lane runs, as on the device)
    return ok;
}

static void run_shape(int N, int G, int n, bool with_metrics, bool with_vis, int log_metrics, int nt) {
    const StateShape S = shape_of(N, G, log_metrics);
    Heap in(S, n, with_metrics, with_vis);
    fill_valid(S, in.a, n);
    Heap out(S, n, log_metrics != 0, false);  // export: every array the handle can fill; never the maps
    std::vector<uint8_t> ref_rec, ref_grid;
    std::vector<int32_t> ref_met;
    std::vector<uint32_t> ref_vis;
    for (int k = 0; k < n; k++) {
        EXPECT(check_all(S, in.a, k, nt));
        // the env's blocks, exactly sized, poisoned
        uint8_t* rec = (uint8_t*)malloc((size_t)S.RS);
        uint8_t* grid = (uint8_t*)malloc((size_t)S.GS);
        int32_t* met = log_metrics ? (int32_t*)malloc((size_t)CTF_N_METRICS * N * 4) : nullptr;
        uint32_t* vis = log_metrics ? (uint32_t*)malloc((size_t)N * S.GS * 4) : nullptr;
        memset(rec, 0xEE, (size_t)S.RS), memset(grid, 0xEE, (size_t)S.GS);
        if (met) memset(met, 0xEE, (size_t)CTF_N_METRICS * N * 4);
        if (vis) memset(vis, 0xEE, (size_t)N * S.GS * 4);
        for (int t = 0; t < nt; t++) states_pack(S, in.a, (size_t)k, rec, grid, met, vis, t, nt);
        reference_bytes(S, in.a, k, ref_rec, ref_grid, ref_met, ref_vis);
        EXPECT(memcmp(rec, ref_rec.data(), (size_t)S.RS) == 0);
        EXPECT(memcmp(grid, ref_grid.data(), (size_t)S.GS) == 0);
        if (met) EXPECT(memcmp(met, ref_met.data(), ref_met.size() * 4) == 0);
        if (vis) {
            if (with_vis) EXPECT(memcmp(vis, ref_vis.data(), ref_vis.size() * 4) == 0);
            else EXPECT(((uint8_t*)vis)[0] == 0xEE && ((uint8_t*)vis)[(size_t)N * S.GS * 4 - 1] == 0xEE);  // (left alone: CTF_F_BASE_ZERO says so)
        }
        for (int t = 0; t < nt; t++) states_unpack(S, rec, grid, (const uint8_t*)met, out.a, (size_t)k, t, nt);
        free(rec), free(grid), free(met), free(vis);
    }
    // pack -> unpack is the identity (done: any non-zero byte reads back as 1; counters not given read back as zeros)
    for (int f = 0; f < ST_VIS; f++) {
        if (!out.a.arr[f]) continue;
        const size_t bytes = (size_t)n * st_row_bytes(S, f);
        if (f == ST_DONE) {
            for (int k = 0; k < n; k++) EXPECT(out.a.arr[f][k] == (in.a.arr[f][k] ? 1 : 0));
        } else if (f == ST_METRICS && !in.a.arr[f]) {
            for (size_t b = 0; b < bytes; b++) EXPECT(out.a.arr[f][b] == 0);
        } else {
            EXPECT(memcmp(out.a.arr[f], in.a.arr[f], bytes) == 0);
        }
    }
}

// one record of a group exported alone: the rows of the others keep their poison
static void run_untouched_rows(int N, int G) {
    const StateShape S = shape_of(N, G, 1);
    const int n = 3;
    Heap in(S, n, true, false), out(S, n, true, false);
    fill_valid(S, in.a, n);
    std::vector<uint8_t> rec((size_t)S.RS), grid((size_t)S.GS);
    std::vector<int32_t> met((size_t)CTF_N_METRICS * N);
    std::vector<uint32_t> vis((size_t)N * S.GS);
    states_pack(S, in.a, 1, rec.data(), grid.data(), met.data(), vis.data(), 0, 1);
    states_unpack(S, rec.data(), grid.data(), (const uint8_t*)met.data(), out.a, 1, 0, 1);
    for (int f = 0; f < ST_VIS; f++) {
        const size_t rb = (size_t)st_row_bytes(S, f);
        for (size_t b = 0; b < rb; b++) EXPECT(out.a.arr[f][b] == 0xA5 && out.a.arr[f][2 * rb + b] == 0xA5);
    }
}

static void run_rejections(int N, int G) {
    const StateShape S = shape_of(N, G, 1);
    const int n = 5, k = 3;
    struct Rule {
        int field, byte_index;
        int32_t value;
        int width;
    };
    const Rule rules[] = {
        {ST_POS, 0, G, 1},           {ST_POS, 2 * N - 1, G, 1},  {ST_POS, 1, -1, 1},        {ST_PERM, N - 1, N, 1},      {ST_PERM, 0, 255, 1},
        {ST_INV, 0, 1001, 4},        {ST_INV, 4 * (N - 1), -1, 4}, {ST_INV, 0, 65536, 4},   {ST_GRID, S.GG - 1, 14, 1},  {ST_GRID, 0, 255, 1},
        {ST_STEP, 0, -1, 4},         {ST_STEP, 0, 1 << 28, 4},
    };
    for (const Rule& r : rules)
        for (int nt : {1, 16}) {
            Heap in(S, n, true, true);
            fill_valid(S, in.a, n);
            uint8_t* p = in.a.arr[r.field] + (size_t)k * st_row_bytes(S, r.field) + r.byte_index;
            if (r.width == 4) memcpy(p, &r.value, 4);
            else *p = (uint8_t)r.value;
            for (int j = 0; j < n; j++) EXPECT(check_all(S, in.a, j, nt) == (j != k));
        }
    // the edges that are legal
    Heap in(S, n, true, true);
    fill_valid(S, in.a, n);
    const int32_t inv = 1000, step = (1 << 28) - 1;
    memcpy(in.a.arr[ST_INV] + (size_t)k * 4 * N, &inv, 4);
    memcpy(in.a.arr[ST_STEP] + (size_t)k * 4, &step, 4);
    ((int8_t*)in.a.arr[ST_POS])[(size_t)k * 2 * N] = (int8_t)(G - 1);
    in.a.arr[ST_GRID][(size_t)k * S.GG] = 13;
    in.a.arr[ST_PERM][(size_t)k * N] = (uint8_t)(N - 1);
    EXPECT(check_all(S, in.a, k, 1) && check_all(S, in.a, k, 16));
}

int main() {
    const int shapes[3][2] = {{2, 4}, {8, 15}, {16, 32}};
    for (const auto& s : shapes) {
        for (int n : {1, 15, 16, 17})
            for (int nt : {1, 16}) {
                run_shape(s[0], s[1], n, true, true, 1, nt);    // everything given
                run_shape(s[0], s[1], n, false, false, 1, nt);  // both defaults: zero counters, maps restart
                run_shape(s[0], s[1], n, false, false, 0, nt);  // a handle without counters and maps
            }
        run_shape(s[0], s[1], 3, true, false, 1, 16);
        run_shape(s[0], s[1], 3, false, true, 1, 16);
        run_untouched_rows(s[0], s[1]);
        run_rejections(s[0], s[1]);
    }
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("all state conversion cases passed\n");
    return 0;
}
