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
// The per-env host calls run the same functions on one record (ctf_state_view.h); for the same shapes, with and without log_metrics:
//   - sv_to_env of a view writes reference_bytes of the same values, into exactly-sized heap blocks, from a view that is itself a
//     heap block of sizeof(ctf_state_view) (N = 16, G = 32 fills it to its last byte);
//   - sv_from_env of those bytes gives the view back, up to the visitation member, which sv_visitation decodes from the maps and log;
//   - one refusal per rule, each leaving the destination blocks untouched;
//   - sv_visitation over a window that wraps the ring (step 700, folded 300), of 0 and of 511 entries, from CTF_F_BASE_ZERO and from
//     given base maps whose cells at 255 wrap to 0, for a log of one env (pitch N) and of env 1 of three (pitch 3 N), against the
//     definition in ctf_visitation.h restated by step number.
// Exit status 0 = all of it held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctf_state_view.h"
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

// ---- one env <-> ctf_state_view (ctf_state_view.h) ------------------------------------------------------------------------------------
static ctf_state_view* new_view() {  // exactly sizeof bytes on the heap, poisoned
    ctf_state_view* v = (ctf_state_view*)malloc(sizeof(ctf_state_view));
    memset(v, 0xA5, sizeof(*v));
    return v;
}

// row k of the arrays as a view; members past N and past G * G keep the poison (nothing may read them)
static ctf_state_view* view_of(const StateShape& S, const StateArrays& a, int k) {
    ctf_state_view* v = new_view();
    const int N = S.N;
    memcpy(v->grid, a.arr[ST_GRID] + (size_t)k * S.GG, (size_t)S.GG);
    memcpy(v->pos, a.arr[ST_POS] + (size_t)k * 2 * N, 2 * (size_t)N);
    memcpy(v->hp, a.arr[ST_HP] + (size_t)k * 8 * N, 8 * (size_t)N);
    memcpy(v->has_flag, a.arr[ST_FLAG] + (size_t)k * N, (size_t)N);
    memcpy(v->inventory, a.arr[ST_INV] + (size_t)k * 4 * N, 4 * (size_t)N);
    memcpy(v->perm, a.arr[ST_PERM] + (size_t)k * N, (size_t)N);
    memcpy(&v->step_count, a.arr[ST_STEP] + (size_t)k * 4, 4);
    memcpy(v->team_captures, a.arr[ST_CAPS] + (size_t)k * 8, 8);
    v->done = a.arr[ST_DONE][k] ? 7 * (int32_t)a.arr[ST_DONE][k] + 249 : 0;  // (any non-zero int32, multiples of 256 among them: 7 * 1 + 249)
    for (int m = 0; m < CTF_N_METRICS; m++) memcpy(v->metrics[m], a.arr[ST_METRICS] + 4 * (((size_t)k * CTF_N_METRICS + m) * N), 4 * (size_t)N);
    for (int i = 0; i < N; i++) memcpy(v->visitation[i], a.arr[ST_VIS] + ((size_t)k * N + i) * S.GG, (size_t)S.GG);
    return v;
}

struct EnvBlocks {  // the env's blocks, exactly sized, poisoned; counters and maps only where the handle keeps them
    size_t rs, gs, ms, vs;
    uint8_t *rec, *grid;
    int32_t* met;
    uint32_t* vis;
    EnvBlocks(const StateShape& S) : rs((size_t)S.RS), gs((size_t)S.GS), ms((size_t)CTF_N_METRICS * S.N * 4), vs((size_t)S.N * S.GS * 4) {
        rec = (uint8_t*)malloc(rs), grid = (uint8_t*)malloc(gs);
        met = S.log_metrics ? (int32_t*)malloc(ms) : nullptr, vis = S.log_metrics ? (uint32_t*)malloc(vs) : nullptr;
        memset(rec, 0xEE, rs), memset(grid, 0xEE, gs);
        if (met) memset(met, 0xEE, ms), memset(vis, 0xEE, vs);
    }
    bool untouched() const {
        size_t bad = 0;
        for (size_t b = 0; b < rs; b++) bad += rec[b] != 0xEE;
        for (size_t b = 0; b < gs; b++) bad += grid[b] != 0xEE;
        for (size_t b = 0; met && b < ms; b++) bad += ((uint8_t*)met)[b] != 0xEE;
        for (size_t b = 0; vis && b < vs; b++) bad += ((uint8_t*)vis)[b] != 0xEE;
        return bad == 0;
    }
    ~EnvBlocks() { free(rec), free(grid), free(met), free(vis); }
};

static void run_view(int N, int G, int log_metrics) {
    const StateShape S = shape_of(N, G, log_metrics);
    const int n = 3;
    Heap in(S, n, true, true);
    fill_valid(S, in.a, n);
    StateArrays kept = in.a;  // what a handle of this kind takes of a view: counters and maps exactly when it keeps them
    if (!log_metrics) kept.arr[ST_METRICS] = kept.arr[ST_VIS] = nullptr;
    std::vector<uint8_t> ref_rec, ref_grid;
    std::vector<int32_t> ref_met;
    std::vector<uint32_t> ref_vis;
    int8_t start[CTF_MAX_AGENTS][2];
    for (auto& p : start) p[0] = (int8_t)(rnd() % G), p[1] = (int8_t)(rnd() % G);
    for (int k = 0; k < n; k++) {
        ctf_state_view* view = view_of(S, in.a, k);
        EnvBlocks env(S);
        EXPECT(sv_to_env(S, view, env.rec, env.grid, env.met, env.vis));
        reference_bytes(S, kept, k, ref_rec, ref_grid, ref_met, ref_vis);
        EXPECT(memcmp(env.rec, ref_rec.data(), env.rs) == 0);
        EXPECT(memcmp(env.grid, ref_grid.data(), env.gs) == 0);
        if (log_metrics) EXPECT(memcmp(env.met, ref_met.data(), env.ms) == 0 && memcmp(env.vis, ref_vis.data(), env.vs) == 0);
        // back: the same view, zero wherever the env holds nothing, done as 0 / 1
        ctf_state_view* back = new_view();
        ctf_state_view* want = new_view();
        int32_t misc[4];
        sv_from_env(S, env.rec, env.grid, env.met, back, misc);
        memset(want, 0, sizeof(*want));
        memcpy(want->grid, view->grid, (size_t)S.GG), memcpy(want->pos, view->pos, 2 * (size_t)N), memcpy(want->hp, view->hp, 8 * (size_t)N);
        memcpy(want->has_flag, view->has_flag, (size_t)N), memcpy(want->inventory, view->inventory, 4 * (size_t)N), memcpy(want->perm, view->perm, (size_t)N);
        want->step_count = view->step_count, want->done = view->done != 0, memcpy(want->team_captures, view->team_captures, 8);
        for (int m = 0; log_metrics && m < CTF_N_METRICS; m++) memcpy(want->metrics[m], view->metrics[m], 4 * (size_t)N);
        EXPECT(memcmp(back, want, sizeof(*want)) == 0);
        EXPECT(misc[0] == view->step_count && misc[1] == view->team_captures[0] && misc[2] == view->team_captures[1]);
        EXPECT((uint32_t)misc[3] == ((view->done ? (uint32_t)CTF_F_DONE : 0u) | (log_metrics ? 0u : (uint32_t)CTF_F_BASE_ZERO) | (uint32_t)view->step_count << CTF_F_FOLDED_SHIFT));
        EXPECT(sv_log_count(misc) == 0);
        if (log_metrics) {  // the maps that were handed in come back through the decode: the log is empty
            std::vector<uint16_t> ring((size_t)CTF_VIS_LOG * N, (uint16_t)0);
            sv_visitation(S, start, misc, env.vis, ring.data(), (size_t)N, back);
            for (int i = 0; i < N; i++) memcpy(want->visitation[i], view->visitation[i], (size_t)S.GG);
            EXPECT(memcmp(back, want, sizeof(*want)) == 0);
        }
        free(view), free(back), free(want);
    }
}

static void run_view_refusals(int N, int G, int log_metrics) {
    const StateShape S = shape_of(N, G, log_metrics);
    Heap in(S, 2, true, true);
    fill_valid(S, in.a, 2);
    int made = 0;
    const auto refused = [&](void (*breakit)(ctf_state_view*, int, int)) {
        ctf_state_view* view = view_of(S, in.a, 1);
        breakit(view, N, G);
        EnvBlocks env(S);
        EXPECT(!sv_to_env(S, view, env.rec, env.grid, env.met, env.vis));
        EXPECT(env.untouched());
        free(view);
        made++;
    };
    refused([](ctf_state_view* v, int, int g) { v->pos[1][0] = (int8_t)g; });
    refused([](ctf_state_view* v, int, int) { v->pos[0][1] = -1; });
    refused([](ctf_state_view* v, int n, int) { v->perm[0] = (uint8_t)n; });
    refused([](ctf_state_view* v, int, int) { v->inventory[1] = 1001; });
    refused([](ctf_state_view* v, int, int) { v->inventory[1] = -1; });
    refused([](ctf_state_view* v, int, int) { v->grid[3] = 14; });
    refused([](ctf_state_view* v, int, int) { v->step_count = -1; });
    refused([](ctf_state_view* v, int, int) { v->step_count = 1 << 28; });
    EXPECT(made == 8);
    // the legal side of every bound
    ctf_state_view* view = view_of(S, in.a, 1);
    view->pos[1][0] = (int8_t)(G - 1), view->perm[0] = (uint8_t)(N - 1), view->inventory[0] = 0, view->inventory[1] = 1000, view->grid[3] = 13;
    view->step_count = (1 << 28) - 1;
    EnvBlocks env(S);
    EXPECT(sv_to_env(S, view, env.rec, env.grid, env.met, env.vis));
    free(view);
}

// sv_visitation against the definition (ctf_visitation.h), by step number: base (zeros + 1 at the start cell, or the given maps), + 1
// at the cell of slot s & 511 for every step s in (folded, step], an entry >= G * G skipped; & 0xFF
static void run_log_window(int N, int G, int step, int folded, bool base_zero, int E, int e) {
    const StateShape S = shape_of(N, G, 1);
    const size_t pitch = (size_t)E * N;
    uint16_t* log = (uint16_t*)malloc((size_t)CTF_VIS_LOG * pitch * 2);  // u16 [512][E][N], exactly
    for (size_t w = 0; w < (size_t)CTF_VIS_LOG * pitch; w++) log[w] = rnd() % 9 == 0 ? (uint16_t)(S.GG + rnd() % 70000) : (uint16_t)(rnd() % S.GG);
    int8_t start[CTF_MAX_AGENTS][2];
    for (auto& p : start) p[0] = (int8_t)(rnd() % G), p[1] = (int8_t)(rnd() % G);
    uint32_t* v = (uint32_t*)malloc((size_t)N * S.GS * 4);
    for (size_t w = 0; w < (size_t)N * S.GS; w++) v[w] = base_zero ? 0xEEEEEEEEu : (rnd() % 3 ? 255u : rnd() % 256);  // (base-zero: not to be read)
    if (!base_zero && step > folded) {  // agent 0's cell 0 stands at 255 and takes exactly one entry of the window: it must show 0
        v[0] = 255;
        for (int s = folded + 1; s <= step; s++) {
            uint16_t& cell = log[((size_t)(s & 511) * E + e) * N];
            cell = s == step ? (uint16_t)0 : (cell == 0 ? (uint16_t)1 : cell);
        }
    }
    std::vector<uint32_t> want((size_t)N * S.GG);
    for (int i = 0; i < N; i++) {
        for (int c = 0; c < S.GG; c++) want[(size_t)i * S.GG + c] = base_zero ? (c == start[i][0] * G + start[i][1] ? 1u : 0u) : v[(size_t)i * S.GS + c];
        for (int s = folded + 1; s <= step; s++) {
            const uint16_t cell = log[((size_t)(s & 511) * E + e) * N + i];
            if (cell < S.GG) want[(size_t)i * S.GG + cell]++;
        }
    }
    const int32_t misc[4] = {step, 0, 0, (base_zero ? CTF_F_BASE_ZERO : 0) | (folded << CTF_F_FOLDED_SHIFT)};
    EXPECT(sv_log_count(misc) == step - folded && sv_log_slot(misc, 0) == ((folded + 1) & 511));
    ctf_state_view* out = new_view();
    sv_visitation(S, start, misc, v, log + (size_t)e * N, pitch, out);
    for (int i = 0; i < CTF_MAX_AGENTS; i++)
        for (int c = 0; c < CTF_MAX_CELLS; c++) {
            const bool inside = i < N && c < S.GG;
            EXPECT(out->visitation[i][c] == (inside ? (uint8_t)(want[(size_t)i * S.GG + c] & 0xFFu) : 0xA5));
            if (inside) EXPECT(v[(size_t)i * S.GS + c] == want[(size_t)i * S.GG + c]);  // the true counts are left in v
        }
    if (!base_zero && step > folded) EXPECT(want[0] == 256 && out->visitation[0][0] == 0);
    EXPECT(out->grid[0] == 0xA5 && out->step_count == (int32_t)0xA5A5A5A5 && out->metrics[CTF_N_METRICS - 1][CTF_MAX_AGENTS - 1] == (int32_t)0xA5A5A5A5);
    free(out), free(v), free(log);
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
        for (int log_metrics : {1, 0}) {
            run_view(s[0], s[1], log_metrics);
            run_view_refusals(s[0], s[1], log_metrics);
        }
        for (int e_of : {0, 1})  // the log of a handle of one env, and of env 1 of three
            for (bool base_zero : {true, false}) {
                run_log_window(s[0], s[1], 700, 300, base_zero, e_of ? 3 : 1, e_of);  // wraps the ring: slots 301..511, 0..188
                run_log_window(s[0], s[1], 300, 300, base_zero, e_of ? 3 : 1, e_of);  // 0 entries
                run_log_window(s[0], s[1], 611, 100, base_zero, e_of ? 3 : 1, e_of);  // 511 entries
            }
    }
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("all state conversion cases passed\n");
    return 0;
}
