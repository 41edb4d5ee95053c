// The rules round 13 added to the retained observation render (marl-ctf-development_amd/csrc/ctf_obs_chunk.h, ctf_obs_delta.h) on
// the CPU, against the oracle's own renders.  A stand-alone program (built with AddressSanitizer + UBSan by
// tests/test_obs_images_cpu.py):
//
//   obs_images_main CONFIGS.bin [STEPS]     CONFIGS.bin = ctf_config structs back to back (the golden cases' and random 2..16-agent ones)
//
// Per config and FLIP_AXIS value (-1, 0, 1, 2): STEPS steps of random actions with resets, the slot images CARRIED from step to
// step under each of five reverse masks (none, all, alternating, team 0 only, team 1 only).  After every step:
//   (a) the images carried forward with obsc_update_cell over the cells that changed equal obsc_env_images of the new grid, dword
//       for dword, in the slots in use;
//   (b) every chunk taken from the carried images is the oracle's render;
//   (c) for every changed cell, at leads 0, 16 and 112, the union over the viewers of obsd_pair_changed's marks is
//       obsd_cell_changed's set of marks;
// and once, (d): the list that a wave's lanes make of a mask of nl bits (64 per pass, two dwords of the mask as the ballot,
// obsd_rank as the place — the kernel gathers the changed cells so) is the ascending list of the set bits, for nl = 1, 63, 64, 65,
// 197 and 2048.
// This is a unit test of rules the device code shares, not a CPU path of the product.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../../marl-ctf-development_amd/csrc/ctf_obs_chunk.h"
#include "../../oracle/ctf_oracle.h"

static uint64_t g_rng = 0xD1B54A32D192ED03ull;
static uint64_t rnd64() {  // xorshift64*: the test's own stream
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}
static uint32_t rnd(uint32_t n) { return (uint32_t)((rnd64() >> 33) % n); }

// the channel LUT as the library derives it (ctf_derive.h; gridworld_ctf.py:987-994: a team-1 viewer sees own / opponent agent
// tiles 4..7 <-> 8..11 and the flags 12 <-> 13 swapped)
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

// (d) what a wave does with the mask (64 lanes x one dword), on the host: lane L of pass p stands for line 64p + L
static bool compaction_is_ascending() {
    const int sizes[6] = {1, 63, 64, 65, 197, 2048};
    for (int nl : sizes) {
        for (int trial = 0; trial < 40; trial++) {
            uint32_t m[64] = {0};
            std::vector<uint16_t> want;
            const uint32_t density = trial == 0 ? 0u : trial == 1 ? 100u : 1u + rnd(99);  // none, all, in between
            for (int l = 0; l < nl; l++)
                if (rnd(100) < density) { m[l >> 5] |= 1u << (l & 31); want.push_back((uint16_t)l); }
            std::vector<uint16_t> list((size_t)nl + 1, 0xFFFFu);
            int total = 0;
            for (int pp = 0; 64 * pp < nl; pp++) {
                const uint64_t bal = ((uint64_t)m[2 * pp + 1] << 32) | (uint64_t)m[2 * pp];
                if (bal) {
                    for (int lane = 0; lane < 64; lane++)
                        if ((bal >> lane) & 1ull) {
                            const int at = total + obsd_rank(bal, lane);
                            if (at >= nl) { fprintf(stderr, "FAIL compaction nl %d: place %d\n", nl, at); return false; }
                            list[(size_t)at] = (uint16_t)(64 * pp + lane);
                        }
                    total += __builtin_popcountll(bal);
                }
            }
            if ((size_t)total != want.size() || !std::equal(want.begin(), want.end(), list.begin()) || list[want.size()] != 0xFFFFu) {
                fprintf(stderr, "FAIL compaction nl %d trial %d: %d lines listed, %zu set\n", nl, trial, total, want.size());
                return false;
            }
        }
    }
    return true;
}

struct Counts {
    long steps = 0, changed = 0, moved_bits = 0, pair_marks = 0;
};

struct Carried {  // what the shadow holds for one reverse mask
    std::vector<uint32_t> images;
    bool valid = false;
};

static bool check(const octf_env* env, const ObsDeltaShape& s, uint32_t rmask, const uint8_t* grid_old, Carried& cd, const char* what, int step,
                  Counts& n) {
    const int W = obsc_image_dwords(s.CGG);
    const uint32_t used = obsc_slots_used(s, rmask);
    std::vector<uint8_t> want((size_t)s.obs_bytes);
    std::vector<uint32_t> fresh((size_t)4 * W, 0xEEEEEEEEu);
    uint16_t self[CTF_MAX_AGENTS];
    ctf_state_view* st = new ctf_state_view;
    octf_get_state(env, st);
    octf_observe(env, want.data(), nullptr, rmask);
    obsc_env_images(s, rmask, st->grid, &st->pos[0][0], fresh.data(), self);
    bool ok = true;
    if (!cd.valid) {  // an unknown key: built from all cells
        cd.images = fresh;
        cd.valid = true;
    } else {
        uint32_t* im = cd.images.data();
        for (int cell = 0; ok && cell < s.GG; cell++) {
            const uint32_t a = grid_old[cell], b = st->grid[cell];
            if (a == b) continue;
            n.changed++;
            obsc_update_cell(
                s, used, cell, cell / s.G, cell % s.G, a, b,
                [&](int slot, int bit) {
                    if (!((im[slot * W + (bit >> 5)] >> (bit & 31)) & 1u)) { fprintf(stderr, "FAIL %s: clears a bit that is not set\n", what); ok = false; }
                    im[slot * W + (bit >> 5)] &= ~(1u << (bit & 31));
                    n.moved_bits++;
                },
                [&](int slot, int bit) {
                    if ((im[slot * W + (bit >> 5)] >> (bit & 31)) & 1u) { fprintf(stderr, "FAIL %s: sets a bit that is set\n", what); ok = false; }
                    im[slot * W + (bit >> 5)] |= 1u << (bit & 31);
                    n.moved_bits++;
                });
            // (c) the pair rule against the cell rule
            const int leads[3] = {0, 16, 112};
            for (int lead : leads) {
                std::set<int> by_cell, by_pair;
                obsd_cell_changed(s, rmask, lead, cell, a, b, [&](int line) { by_cell.insert(line); });
                for (int i = 0; i < s.N; i++) obsd_pair_changed(s, rmask, lead, cell, i, a, b, [&](int line) { by_pair.insert(line); });
                n.pair_marks += (long)by_pair.size();
                if (by_cell != by_pair) {
                    fprintf(stderr, "FAIL %s mask %#x step %d: cell %d %u -> %u lead %d: the pairs mark %zu lines, the cell rule %zu\n", what, rmask,
                            step, cell, a, b, lead, by_pair.size(), by_cell.size());
                    ok = false;
                }
            }
        }
        // (a) dword for dword in the slots in use
        for (int slot = 0; ok && slot < 4; slot++)
            if ((used & (1u << slot)) && memcmp(im + slot * W, fresh.data() + slot * W, (size_t)W * 4) != 0) {
                fprintf(stderr, "FAIL %s mask %#x step %d: the carried image of slot %d is not the image of the new grid\n", what, rmask, step, slot);
                ok = false;
            }
    }
    // (b) every chunk from the carried images
    for (int k = 0; ok && 16 * k + 16 <= s.obs_bytes; k++) {
        uint8_t got[16];
        obsc_chunk_images(s, rmask, cd.images.data(), self, k, got);
        if (memcmp(got, want.data() + 16 * k, 16) != 0) {
            fprintf(stderr, "FAIL %s mask %#x step %d: chunk %d from the carried images differs from the oracle's render\n", what, rmask, step, k);
            ok = false;
        }
    }
    delete st;
    return ok;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CONFIGS.bin [STEPS]\n", argv[0]); return 2; }
    const int steps = argc > 2 ? atoi(argv[2]) : 50;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<ctf_config> cfgs;
    ctf_config c;
    while (fread(&c, sizeof(c), 1, f) == 1) cfgs.push_back(c);
    fclose(f);
    if (cfgs.empty()) { fprintf(stderr, "no configs in %s\n", argv[1]); return 2; }
    if (!compaction_is_ascending()) return 1;
    printf("ok compaction: nl 1, 63, 64, 65, 197, 2048\n");
    for (size_t k = 0; k < cfgs.size(); k++) {
        if (cfgs[k].abi_version != CTF_ABI_VERSION) { fprintf(stderr, "config %zu: abi_version %d\n", k, cfgs[k].abi_version); return 2; }
        Counts n;
        const ObsDeltaShape s0 = shape_of(cfgs[k]);
        for (int flip = -1; flip <= 2; flip++) {
            ctf_config cfg = cfgs[k];
            cfg.flip_axis = flip;
            const ObsDeltaShape s = shape_of(cfg);
            const uint32_t all = (1u << s.N) - 1u;
            const uint32_t masks[5] = {0u, all, 0x5555u & all, ~s.team_mask & all, s.team_mask};
            char what[96];
            snprintf(what, sizeof(what), "config %zu (N %d, G %d, C %d) flip %d", k, s.N, s.G, cfg.n_channels, flip);
            octf_env* env = octf_create(&cfg);
            octf_seed(env, 5000 + 13 * k + (uint64_t)(flip + 1), 6000 + 13 * k + (uint64_t)(flip + 1));
            octf_reset(env);
            int8_t actions[CTF_MAX_AGENTS];
            double rewards[CTF_MAX_AGENTS];
            uint8_t done = 0;
            bool ok = true;
            Carried carried[5];
            std::vector<uint8_t> grid_old((size_t)s.GG);
            ctf_state_view* st = new ctf_state_view;
            for (int t = 0; ok && t <= steps; t++) {  // t = 0: the reset state, the images built from all cells
                if (t > 0) {
                    if (done || rnd(23) == 0) { octf_reset(env); done = 0; }
                    for (int i = 0; i < s.N; i++) actions[i] = (int8_t)rnd(9);
                    const uint32_t status = octf_step(env, actions, rewards, &done);
                    if (status & (CTF_ST_NO_RESPAWN | CTF_ST_SPAWN_EDGE)) { octf_reset(env); done = 0; }
                }
                for (int m = 0; ok && m < 5; m++) ok = check(env, s, masks[m], grid_old.data(), carried[m], what, t, n);
                octf_get_state(env, st);
                memcpy(grid_old.data(), st->grid, (size_t)s.GG);
                n.steps++;
            }
            delete st;
            octf_destroy(env);
            if (!ok) return 1;
        }
        if (n.changed == 0 || n.moved_bits == 0 || n.pair_marks == 0) {
            fprintf(stderr, "FAIL config %zu: %ld changed cells, %ld image bits moved, %ld pair marks: the run shows nothing\n", k, n.changed,
                    n.moved_bits, n.pair_marks);
            return 1;
        }
        printf("ok config %zu: N %d G %d C %d; %ld states, %ld changed cells, %ld image bits moved, %ld lines marked by pairs\n", k, s0.N, s0.G,
               cfgs[k].n_channels, n.steps, n.changed, n.moved_bits, n.pair_marks);
    }
    printf("all obs-images cases passed\n");
    return 0;
}
