// The dirty lines of the retained observation render as a wave of k_observe_delta marks them since round 17
// (marl-ctf-development_amd/csrc/ctf_obs_delta.h, ctf_obs_chunk.h), on the CPU: a lane per (changed cell, viewer) pair with the cell
// flipped from its row and column (obsc_flip_rc, obsd_pair_changed_at), a lane per moved viewer with both cells taken from the
// position bytes' rows and columns (obsd_viewer_moved_rc) — no division anywhere, every small product through OBSD_MUL.  A
// stand-alone program (built with AddressSanitizer + UBSan by tests/test_obs_moves_cpu.py):
//
//   obs_moves_main CONFIGS.bin PLANTED.bin [STEPS]
//     CONFIGS.bin  ctf_config structs back to back: played by the oracle, STEPS steps of random actions with resets in between
//     PLANTED.bin  blocks of [ctf_config][int32 n][n x (grid u8[GG], pos i8[2N])]: consecutive states of a planted table, each pair
//                  of neighbours one transition
//
// 1. obsd_viewer_moved_rc marks exactly obsd_viewer_moved's lines: all four flip axes, every pair of cells of an 11 x 11 and a
//    15 x 15 grid, lead 0, 16 .. 112, the view reversed and not.
// 2. Per transition, reverse mask and lead, the wave's work items — one per (changed cell, viewer) and one per moved viewer — mark
//    into a mask of exactly the span's dwords, in forward and in a seeded shuffled order (the lanes' ORs commute).  The mask must
//    be obsd_env_dirty's, bit for bit: no line missed, none marked that the rule does not name, none outside the span.
// A unit test of a rule the device code shares, not a CPU path of the product.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../marl-ctf-development_amd/csrc/ctf_obs_chunk.h"
#include "../../oracle/ctf_oracle.h"

static uint64_t g_rng = 0xD1B54A32D192ED03ull;
static uint32_t rnd(uint32_t n) {  // xorshift64*: the test's own stream
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (uint32_t)(((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

// the channel LUT as the library derives it (ctf_derive.h; tests/obs_delta/obs_delta_main.cpp has the same)
static ObsDeltaShape shape_of(const ctf_config& c) {
    ObsDeltaShape s;
    s.N = c.n_agents; s.G = c.grid_size; s.GG = s.G * s.G; s.CGG = c.n_channels * s.GG; s.obs_bytes = s.N * s.CGG;
    s.flip_axis = c.flip_axis;
    s.team_mask = 0;
    for (int i = 0; i < s.N; i++) s.team_mask |= (uint32_t)(c.agent_team[i] & 1) << i;
    for (int t = 0; t < 2; t++) {
        uint64_t lut = 0;
        for (int v = 0; v < 16; v++) {
            int tile = v;
            if (t == 1) {
                if (v >= 4 && v <= 7) tile = v + 4;
                else if (v >= 8 && v <= 11) tile = v - 4;
                else if (v == 12) tile = 13;
                else if (v == 13) tile = 12;
            }
            uint64_t code = 15;
            if (v >= 1 && v <= 13)
                for (int k = 1; k < c.n_channels; k++)
                    if (c.tile_of_channel[k] == tile) code = (uint64_t)k;
            lut |= code << (4 * v);
        }
        s.chan_lut[t] = lut;
    }
    return s;
}

// ---- 1. the viewer's move from rows and columns
static bool viewer_moves() {
    long checked = 0;
    static const int flips[] = {-1, 0, 1, 2}, grids[] = {11, 15}, viewers[] = {0, 3};
    for (int flip : flips)
        for (int G : grids) {
            ObsDeltaShape s;
            s.N = 4; s.G = G; s.GG = G * G; s.CGG = 7 * s.GG; s.obs_bytes = s.N * s.CGG; s.flip_axis = flip;
            s.team_mask = 0xAu; s.chan_lut[0] = s.chan_lut[1] = ~0ull;
            for (int lead = 0; lead < CTF_OBS_LINE; lead += 16)
                for (int oc = 0; oc < s.GG; oc++)
                    for (int nc = 0; nc < s.GG; nc++)
                        for (int i : viewers)
                            for (uint32_t rm = 0; rm < 16; rm += 15) {
                                int want[2], got[2], nw = 0, ng = 0;
                                obsd_viewer_moved(s, rm, lead, i, oc, nc, [&](int l) { if (nw < 2) want[nw] = l; nw++; });
                                obsd_viewer_moved_rc(s, rm, lead, i, oc / G, oc % G, nc / G, nc % G, [&](int l) { if (ng < 2) got[ng] = l; ng++; });
                                if (nw != 2 || ng != 2 || want[0] != got[0] || want[1] != got[1]) {
                                    fprintf(stderr, "FAIL viewer move: flip %d G %d lead %d viewer %d mask %#x cells %d -> %d\n", flip, G, lead, i, rm, oc, nc);
                                    return false;
                                }
                                checked++;
                            }
        }
    printf("ok viewer moves: %ld (flip, grid, lead, cells, viewer, reversed) cases mark obsd_viewer_moved's lines\n", checked);
    return true;
}

// ---- 2. the lanes' marks against the whole rule
struct Item {  // what one lane does: a (changed cell, viewer) pair or a moved viewer
    int viewer, cell;  // cell < 0: the viewer moved
};

struct Tally {
    long transitions = 0, items = 0, lines = 0, most = 0;
};

static bool mark_once(const ObsDeltaShape& s, uint32_t rm, int lead, const uint8_t* g0, const int8_t* p0, const uint8_t* g1, const int8_t* p1,
                      const std::vector<Item>& items, const std::vector<int>& order, const std::vector<uint32_t>& want, const char* what) {
    const int nl = obsd_lines(s.obs_bytes, lead);
    std::vector<uint32_t> mask((size_t)(nl + 31) / 32, 0u);  // exactly the span's dwords: the sanitizer sees a mark outside it
    bool outside = false;
    auto mark = [&](int line) {  // the kernel's mark
        if ((uint32_t)line < (uint32_t)nl) mask[(size_t)line >> 5] |= 1u << (line & 31);
        else outside = true;
    };
    for (int k : order) {
        const Item& it = items[(size_t)k];
        if (it.cell >= 0) {
            const int r = it.cell / s.G, c = it.cell % s.G;
            const int shown = ((rm >> it.viewer) & 1u) ? obsc_flip_rc(s, it.cell, r, c) : it.cell;  // as the kernel's lane has it
            obsd_pair_changed_at(s, lead, shown, it.viewer, g0[it.cell], g1[it.cell], mark);
        } else {
            obsd_viewer_moved_rc(s, rm, lead, it.viewer, p0[2 * it.viewer], p0[2 * it.viewer + 1], p1[2 * it.viewer], p1[2 * it.viewer + 1], mark);
        }
    }
    if (outside) { fprintf(stderr, "FAIL %s: a line outside the env's span was marked\n", what); return false; }
    if (mask != want) { fprintf(stderr, "FAIL %s: the lanes' marks are not obsd_env_dirty's mask\n", what); return false; }
    return true;
}

static bool transition(const ObsDeltaShape& s, uint32_t rm, int lead, const uint8_t* g0, const int8_t* p0, const uint8_t* g1, const int8_t* p1,
                       const char* what, Tally& tally) {
    const int nl = obsd_lines(s.obs_bytes, lead);
    std::vector<uint32_t> want((size_t)(nl + 31) / 32);
    obsd_env_dirty(s, rm, lead, g0, p0, g1, p1, want.data());
    std::vector<Item> items;
    for (int cell = 0; cell < s.GG; cell++)
        if (g0[cell] != g1[cell])
            for (int i = 0; i < s.N; i++) items.push_back(Item{i, cell});
    for (int i = 0; i < s.N; i++)
        if (p0[2 * i] != p1[2 * i] || p0[2 * i + 1] != p1[2 * i + 1]) items.push_back(Item{i, -1});
    std::vector<int> order(items.size());
    for (size_t k = 0; k < order.size(); k++) order[k] = (int)k;
    if (!mark_once(s, rm, lead, g0, p0, g1, p1, items, order, want, what)) return false;
    for (size_t k = order.size(); k > 1; k--) std::swap(order[k - 1], order[rnd((uint32_t)k)]);
    if (!mark_once(s, rm, lead, g0, p0, g1, p1, items, order, want, what)) return false;
    long pop = 0;
    for (uint32_t m : want) pop += __builtin_popcount(m);
    tally.transitions++; tally.items += (long)items.size(); tally.lines += pop;
    if (pop > tally.most) tally.most = pop;
    return true;
}

static uint32_t resolved(const ObsDeltaShape& s, int which) {  // none, all, the default (team 1 reversed), every other agent
    const uint32_t all = (1u << s.N) - 1u;
    return which == 0 ? 0u : which == 1 ? all : which == 2 ? (s.team_mask & all) : (0x5555u & all);
}

static bool played(const ctf_config& cfg, size_t k, int steps) {
    const ObsDeltaShape s = shape_of(cfg);
    Tally tally;
    for (int run = 0; run < 4; run++) {
        const uint32_t rm = resolved(s, (int)((run + k) % 4));
        octf_env* env = octf_create(&cfg);
        octf_seed(env, 3000 + 11 * k + run, 4000 + 11 * k + run);
        ctf_state_view* a = new ctf_state_view;
        ctf_state_view* b = new ctf_state_view;
        octf_get_state(env, a);
        int8_t actions[CTF_MAX_AGENTS];
        double rewards[CTF_MAX_AGENTS];
        uint8_t done = 0;
        bool ok = true;
        for (int t = 0; t < steps && ok; t++) {
            if (done || rnd(29) == 0) { octf_reset(env); done = 0; }  // seen by the render as one change with the step
            for (int i = 0; i < s.N; i++) actions[i] = (int8_t)rnd(9);
            const uint32_t status = octf_step(env, actions, rewards, &done);
            octf_get_state(env, b);
            const int lead = 16 * (int)((t + 3 * run + k) % 8);
            char what[128];
            snprintf(what, sizeof(what), "config %zu (N %d, G %d, flip %d) mask %#x lead %d step %d", k, s.N, s.G, s.flip_axis, rm, lead, t);
            ok = transition(s, rm, lead, a->grid, &a->pos[0][0], b->grid, &b->pos[0][0], what, tally);
            std::swap(a, b);
            if (status & (CTF_ST_NO_RESPAWN | CTF_ST_SPAWN_EDGE)) { octf_reset(env); done = 0; }
        }
        delete a; delete b;
        octf_destroy(env);
        if (!ok) return false;
    }
    printf("ok config %zu: N %d G %d flip %d; %ld transitions x 2 orders, %.1f work items and %.1f dirty lines each, most %ld\n", k, s.N, s.G, s.flip_axis,
           tally.transitions, (double)tally.items / tally.transitions, (double)tally.lines / tally.transitions, tally.most);
    return true;
}

static bool planted(FILE* f, int* blocks) {
    ctf_config cfg;
    while (fread(&cfg, sizeof(cfg), 1, f) == 1) {
        int32_t n = 0;
        if (fread(&n, sizeof(n), 1, f) != 1 || n < 2) { fprintf(stderr, "planted block %d: no states\n", *blocks); return false; }
        const ObsDeltaShape s = shape_of(cfg);
        std::vector<std::vector<uint8_t>> grids((size_t)n, std::vector<uint8_t>((size_t)s.GG));
        std::vector<std::vector<int8_t>> pos((size_t)n, std::vector<int8_t>((size_t)(2 * s.N)));
        for (int q = 0; q < n; q++)
            if (fread(grids[(size_t)q].data(), 1, (size_t)s.GG, f) != (size_t)s.GG || fread(pos[(size_t)q].data(), 1, (size_t)(2 * s.N), f) != (size_t)(2 * s.N)) {
                fprintf(stderr, "planted block %d: short read\n", *blocks);
                return false;
            }
        Tally tally;
        for (int q = 0; q + 1 < n; q++)
            for (int which = 0; which < 4; which++) {
                const uint32_t rm = resolved(s, which);
                const int lead = 16 * ((q + 3 * which + *blocks) % 8);
                char what[128];
                snprintf(what, sizeof(what), "planted block %d (N %d, G %d, flip %d) mask %#x lead %d states %d -> %d", *blocks, s.N, s.G, s.flip_axis, rm, lead, q, q + 1);
                if (!transition(s, rm, lead, grids[(size_t)q].data(), pos[(size_t)q].data(), grids[(size_t)q + 1].data(), pos[(size_t)q + 1].data(), what, tally))
                    return false;
            }
        printf("ok planted %d: N %d G %d flip %d; %ld transitions x 2 orders, %.1f work items and %.1f dirty lines each, most %ld\n", *blocks, s.N, s.G,
               s.flip_axis, tally.transitions, (double)tally.items / tally.transitions, (double)tally.lines / tally.transitions, tally.most);
        (*blocks)++;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s CONFIGS.bin PLANTED.bin [STEPS]\n", argv[0]); return 2; }
    const int steps = argc > 3 ? atoi(argv[3]) : 60;
    if (!viewer_moves()) return 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<ctf_config> cfgs;
    ctf_config c;
    while (fread(&c, sizeof(c), 1, f) == 1) cfgs.push_back(c);
    fclose(f);
    if (cfgs.empty()) { fprintf(stderr, "no configs in %s\n", argv[1]); return 2; }
    for (size_t k = 0; k < cfgs.size(); k++) {
        if (cfgs[k].abi_version != CTF_ABI_VERSION) { fprintf(stderr, "config %zu: abi_version %d\n", k, cfgs[k].abi_version); return 2; }
        if (!played(cfgs[k], k, steps)) return 1;
    }
    f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    int blocks = 0;
    const bool ok = planted(f, &blocks);
    fclose(f);
    if (!ok) return 1;
    printf("all obs-moves cases passed: %zu configs, %d planted blocks\n", cfgs.size(), blocks);
    return 0;
}
