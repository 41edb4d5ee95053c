// The dirty-line rule of the retained observation render (marl-ctf-development_amd/csrc/ctf_obs_delta.h) on the CPU, against the
// oracle's own consecutive renders.  A stand-alone program (built with AddressSanitizer + UBSan by tests/test_obs_delta_cpu.py):
//
//   obs_delta_main CONFIGS.bin [STEPS]      CONFIGS.bin = ctf_config structs back to back (written by the test from the golden
//                                           cases' kwargs and from random 2..16-agent configurations)
//
// Per config, reverse mask and lead (the offset of the env's block inside its first 128-byte line, i.e. e * obs_bytes mod 128 for
// the envs of a batch): STEPS steps of random actions with resets, episode ends and hand-planted states in between.  After
// every change of state
//   - the dirty set must hold every line in which the oracle's render before and after differ, and
//   - the render before, with only the dirty lines' bytes (of this env's block) taken from the render after, must BE the
//     render after, byte for byte.
// The excess of the dirty set over the truly changed lines is reported, not gated.
// This is a unit test of a rule the device code shares, not a CPU path of the product.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../marl-ctf-development_amd/csrc/ctf_obs_delta.h"
#include "../../oracle/ctf_oracle.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {  // xorshift64*: the test's own stream
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (uint32_t)(((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

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

struct Tally {
    long checks = 0, dirty = 0, truly = 0, max_dirty = 0;
};

struct Runner {
    const ctf_config& cfg;
    ObsDeltaShape s;
    uint32_t rmask;
    int lead;
    octf_env* env;
    std::vector<uint8_t> before, after, patched;
    ctf_state_view* st_before;
    ctf_state_view* st_after;
    std::vector<uint32_t> mask;
    Tally tally;

    Runner(const ctf_config& c, uint32_t rm, int ld) : cfg(c), s(shape_of(c)), rmask(rm), lead(ld) {
        env = octf_create(&cfg);
        before.resize((size_t)s.obs_bytes); after.resize((size_t)s.obs_bytes); patched.resize((size_t)s.obs_bytes);
        st_before = new ctf_state_view; st_after = new ctf_state_view;
        mask.resize((size_t)(obsd_lines(s.obs_bytes, lead) + 31) / 32);
        octf_get_state(env, st_before);
        octf_observe(env, before.data(), nullptr, rmask);
    }
    ~Runner() { octf_destroy(env); delete st_before; delete st_after; }

    // the env's state has changed since `before` was rendered: check the rule, then make the new render the old one
    bool check(const char* what, int step) {
        octf_get_state(env, st_after);
        octf_observe(env, after.data(), nullptr, rmask);
        // (the library resolves CTF_REVERSE_DEFAULT to the team bits before any kernel sees the mask: resolve_reverse, ctf_abi.hip)
        const uint32_t resolved = rmask == CTF_REVERSE_DEFAULT ? s.team_mask : rmask;
        obsd_env_dirty(s, resolved, lead, st_before->grid, &st_before->pos[0][0], st_after->grid, &st_after->pos[0][0], mask.data());
        const int nl = obsd_lines(s.obs_bytes, lead);
        long dirty = 0, truly = 0;
        patched = before;
        for (int l = 0; l < nl; l++) {
            const int lo = l * CTF_OBS_LINE - lead < 0 ? 0 : l * CTF_OBS_LINE - lead;
            const int hi = (l + 1) * CTF_OBS_LINE - lead > s.obs_bytes ? s.obs_bytes : (l + 1) * CTF_OBS_LINE - lead;
            const bool differs = memcmp(before.data() + lo, after.data() + lo, (size_t)(hi - lo)) != 0;
            const bool is_dirty = (mask[(size_t)l >> 5] >> (l & 31)) & 1u;
            truly += differs;
            dirty += is_dirty;
            if (differs && !is_dirty) {
                fprintf(stderr, "FAIL %s step %d: line %d of the env's span differs between the renders and is not in the dirty set\n", what, step, l);
                return false;
            }
            if (is_dirty) memcpy(patched.data() + lo, after.data() + lo, (size_t)(hi - lo));
        }
        if (memcmp(patched.data(), after.data(), (size_t)s.obs_bytes) != 0) {
            fprintf(stderr, "FAIL %s step %d: the old render with the dirty lines applied is not the new render\n", what, step);
            return false;
        }
        tally.checks++; tally.dirty += dirty; tally.truly += truly;
        if (dirty > tally.max_dirty) tally.max_dirty = dirty;
        before.swap(after);
        std::swap(st_before, st_after);
        return true;
    }

    // a hand-planted state: random tiles in a few cells, every agent somewhere else (only rendered, never stepped)
    void plant() {
        ctf_state_view* v = new ctf_state_view;
        octf_get_state(env, v);
        const int cells = 1 + (int)rnd(12);
        for (int k = 0; k < cells; k++) v->grid[rnd((uint32_t)s.GG)] = (uint8_t)rnd(14);
        for (int i = 0; i < s.N; i++)
            if (rnd(2)) { v->pos[i][0] = (int8_t)rnd((uint32_t)s.G); v->pos[i][1] = (int8_t)rnd((uint32_t)s.G); }
        octf_set_state(env, v);
        delete v;
    }

    bool run(int steps, const char* what) {
        int8_t actions[CTF_MAX_AGENTS];
        double rewards[CTF_MAX_AGENTS];
        uint8_t done = 0;
        for (int t = 0; t < steps; t++) {
            if (done || rnd(41) == 0) {  // auto-reset / a reset out of turn, seen by the render as one change with the step
                octf_reset(env);
                done = 0;
                if (rnd(2) && !check(what, t)) return false;
            }
            for (int i = 0; i < s.N; i++) actions[i] = (int8_t)rnd(9);
            const uint32_t status = octf_step(env, actions, rewards, &done);
            if (!check(what, t)) return false;
            if (status & (CTF_ST_NO_RESPAWN | CTF_ST_SPAWN_EDGE)) { octf_reset(env); if (!check(what, t)) return false; }
            if (rnd(23) == 0) {
                plant();
                if (!check(what, t)) return false;
                octf_reset(env);  // the planted state is not one the rules would reach
                done = 0;
                if (!check(what, t)) return false;
            }
        }
        return true;
    }
};

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CONFIGS.bin [STEPS]\n", argv[0]); return 2; }
    const int steps = argc > 2 ? atoi(argv[2]) : 200;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<ctf_config> cfgs;
    ctf_config c;
    while (fread(&c, sizeof(c), 1, f) == 1) cfgs.push_back(c);
    fclose(f);
    if (cfgs.empty()) { fprintf(stderr, "no configs in %s\n", argv[1]); return 2; }
    static const int leads[] = {0, 16, 48, 80, 112};  // blocks are whole 16-byte chunks: every lead is a multiple of 16
    for (size_t k = 0; k < cfgs.size(); k++) {
        const ctf_config& cfg = cfgs[k];
        if (cfg.abi_version != CTF_ABI_VERSION) { fprintf(stderr, "config %zu: abi_version %d\n", k, cfg.abi_version); return 2; }
        const ObsDeltaShape s = shape_of(cfg);
        const uint32_t all = (1u << cfg.n_agents) - 1u;
        const uint32_t masks[] = {CTF_REVERSE_DEFAULT, 0u, all, 0x5555u & all, (uint32_t)rnd(all + 1u)};
        Tally sum;
        for (int li = 0; li < 5; li++) {
            const uint32_t rm = masks[(li + k) % 5];
            char what[96];
            snprintf(what, sizeof(what), "config %zu (N %d, G %d, C %d, flip %d) mask %#x lead %d", k, cfg.n_agents, cfg.grid_size, cfg.n_channels,
                     cfg.flip_axis, rm, leads[li]);
            Runner r(cfg, rm, leads[li]);
            octf_seed(r.env, 1000 + 7 * k + li, 2000 + 7 * k + li);
            if (!r.run(steps, what)) return 1;
            sum.checks += r.tally.checks; sum.dirty += r.tally.dirty; sum.truly += r.tally.truly;
            if (r.tally.max_dirty > sum.max_dirty) sum.max_dirty = r.tally.max_dirty;
        }
        printf("ok config %zu: N %d G %d C %d flip %d, %d bytes (%.3f lines) per env; %ld checks; lines per check: dirty %.2f, truly changed %.2f "
               "(excess %.2f), most dirty %ld\n",
               k, cfg.n_agents, cfg.grid_size, cfg.n_channels, cfg.flip_axis, s.obs_bytes, s.obs_bytes / 128.0, sum.checks,
               (double)sum.dirty / sum.checks, (double)sum.truly / sum.checks, (double)(sum.dirty - sum.truly) / sum.checks, sum.max_dirty);
    }
    printf("all obs-delta cases passed\n");
    return 0;
}
