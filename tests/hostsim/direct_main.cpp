// direct_main.cpp — the step kernel's logic in CTF_RNG_COUNTER_DIRECT mode (marl-ctf-development_amd/csrc/ctf_step_core.h: env_step
// with PyDirect / NpDirect, the windows' set-up and the on-demand blocks) compiled for the host with one lane per env (W = 1)
// and stepped against the oracle in CTF_RNG_COUNTER mode, which reads the same tape.
//
// A stand-alone program (its own main) so that the sanitizer runtimes are linked in: tests/test_counter_direct_cpu.py builds
// it with -fsanitize=address,undefined next to oracle/ctf_oracle.c and runs it.  Every buffer the step touches — the "HBM"
// arrays and the "LDS" slot — is a heap allocation of exactly the size the library gives it, and the ring / digest / position
// pointers are NULL: no code of this mode may touch them.  Built twice: with the shipped window sizes and with
// -DNP_DIRECT_BYTES=8 -DPY_DIRECT_BYTES=4, where nearly every draw computes its block on demand.
//
//   direct_main <config file>...      each file: the raw bytes of one ctf_config (rng_mode is set here)
//   direct_main --ties <config file>  the tie sweep on that config (run_ties, below): the tag compare where the draw equals the threshold
//
// TEST INFRASTRUCTURE ONLY (see hostsim.cpp): a unit test of device code, not a CPU path of the product.
#define CTF_HOSTSIM 1
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "ctf_step_core.h"

extern "C" {
#include "../../oracle/ctf_oracle.h"
}

static char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#include "ctf_derive.h"

template <typename T>
static std::unique_ptr<T[]> exactly(size_t n) {  // value-initialised, no slack behind it
    return std::unique_ptr<T[]>(new T[n]());
}

struct Sim {
    DevCfg d;
    DevPtrs p;
    std::unique_ptr<uint8_t[]> grid, rec, init_grid;
    std::unique_ptr<unsigned long long[]> rngctr;
    std::unique_ptr<int32_t[]> metrics;
    std::unique_ptr<uint32_t[]> vis, status, lds;
    std::unique_ptr<uint16_t[]> vislog;
};

static bool sim_create(Sim& h, const ctf_config* cfg, int n_envs) {
    if (derive(cfg, n_envs, &h.d)) return false;
    const DevCfg& d = h.d;
    const size_t E = (size_t)n_envs;
    h.grid = exactly<uint8_t>(E * d.GS);
    h.rec = exactly<uint8_t>(E * d.RS);
    h.init_grid = exactly<uint8_t>((size_t)d.GS);
    memcpy(h.init_grid.get(), cfg->init_grid, (size_t)d.GG);
    h.rngctr = exactly<unsigned long long>(E * 4);
    h.metrics = exactly<int32_t>(d.log_metrics ? E * CTF_N_METRICS * d.N : 1);
    h.vis = exactly<uint32_t>(d.log_metrics ? E * d.N * d.GS : 1);
    h.vislog = exactly<uint16_t>(d.log_metrics ? (size_t)CTF_VIS_LOG * E * d.N : 1);
    h.status = exactly<uint32_t>(1);
    h.lds = exactly<uint32_t>((size_t)step_slot_bytes(d.GS, d.RS, d.N, d.log_metrics != 0) / 4);
    memset(&h.p, 0, sizeof(h.p));  // mt_py, mt_np, py_top, np_hit, np_nib, rngpos, rngready, rngage: NULL
    h.p.grid = h.grid.get(); h.p.rec = h.rec.get(); h.p.rngctr = h.rngctr.get();
    h.p.metrics = h.metrics.get(); h.p.vis = h.vis.get(); h.p.vislog = h.vislog.get();
    h.p.init_grid = h.init_grid.get(); h.p.status = h.status.get();
    for (size_t e = 0; e < E; e++) {  // k_reset with init_perm
        memcpy(h.grid.get() + e * d.GS, h.init_grid.get(), (size_t)d.GS);
        uint8_t* sr = h.rec.get() + e * d.RS;
        reset_record(d, sr);
        for (int i = 0; i < d.N; i++) sr[d.off_perm + i] = (uint8_t)i;
    }
    return true;
}

// k_step_direct<METRICS, 1> for one env: staging, group_step, write-back
template <bool METRICS>
static void step_env(Sim& h, int e, const int8_t* actions, double* rw64, uint8_t* done, uint32_t flags) {
    const DevCfg& d = h.d;
    const int GW = d.GS / 4, RW = d.RS / 4, AW = 4, WW = STEP_RNG_WORDS, N = d.N;
    uint32_t* lds = h.lds.get();
    GroupRngDirect R;
    group_issue_loads(R, d, h.p, e);
    memcpy(lds, h.grid.get() + (size_t)e * d.GS, (size_t)d.GS);
    memcpy(lds + GW, h.rec.get() + (size_t)e * d.RS, (size_t)d.RS);
    memset(lds + GW + RW, 0, 16);
    memcpy(lds + GW + RW, actions + (size_t)e * N, (size_t)N);
    memset(lds + GW + RW + AW, 0xA5, (size_t)WW * 4);  // the windows: garbage until parked
    if (METRICS) memset(lds + GW + RW + AW + WW, 0, (size_t)((CTF_N_METRICS * N + 3) & ~3));
    uint32_t left_ring = 0;
    group_step<METRICS, 1>(R, d, h.p, (uint8_t*)lds, e, 0, 0, flags, (float*)nullptr, rw64, done, left_ring);
    memcpy(h.grid.get() + (size_t)e * d.GS, lds, (size_t)d.GS);
    memcpy(h.rec.get() + (size_t)e * d.RS, lds + GW, (size_t)d.RS);
    if (METRICS) {
        const uint8_t* dl = (const uint8_t*)(lds + GW + RW + AW + WW);
        for (int w = 0; w < CTF_N_METRICS * N; w++) h.metrics[(size_t)e * CTF_N_METRICS * N + w] += dl[w];
    }
}

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            printf("MISMATCH %s env %d step %d: ", name, e, t); \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
            return false;                                 \
        }                                                 \
    } while (0)

// one env's outputs and state after a step against the oracle's, bit for bit (nothing but the status where the oracle reports one)
static bool same_as_oracle(const char* name, int e, int t, Sim& h, octf_env* o, ctf_state_view* view, const double* rw64, const uint8_t* done,
                           const double* orw, uint8_t odone, uint32_t ost, const uint64_t* after) {
    const DevCfg& d = h.d;
    const int N = d.N;
    CHECK(h.status[0] == ost, "status %u, oracle %u", h.status[0], ost);
    if (ost) return true;
    CHECK(h.rngctr[4 * e] == after[0] && h.rngctr[4 * e + 1] == after[1], "words consumed (%llu, %llu), oracle (%llu, %llu)",
          h.rngctr[4 * e], h.rngctr[4 * e + 1], (unsigned long long)after[0], (unsigned long long)after[1]);
    CHECK(done[e] == odone, "done %d, oracle %d", done[e], odone);
    for (int i = 0; i < N; i++) CHECK(memcmp(&rw64[(size_t)e * N + i], &orw[i], 8) == 0, "reward of agent %d: %.17g, oracle %.17g", i, rw64[(size_t)e * N + i], orw[i]);
    octf_get_state(o, view);
    const uint8_t* rec = h.rec.get() + (size_t)e * d.RS;
    CHECK(memcmp(view->grid, h.grid.get() + (size_t)e * d.GS, (size_t)d.GG) == 0, "grid");
    for (int i = 0; i < N; i++) {
        int16_t inv;
        memcpy(&inv, rec + d.off_inv + 2 * i, 2);
        CHECK(memcmp(&view->hp[i], rec + 8 * i, 8) == 0, "hp of agent %d", i);
        CHECK(view->pos[i][0] == (int8_t)rec[d.off_pos + 2 * i] && view->pos[i][1] == (int8_t)rec[d.off_pos + 2 * i + 1], "pos of agent %d", i);
        CHECK(view->has_flag[i] == rec[d.off_flag + i] && view->perm[i] == rec[d.off_perm + i] && view->inventory[i] == inv,
              "has_flag / perm / inventory of agent %d", i);
    }
    int32_t misc[4];
    memcpy(misc, rec + d.off_misc, 16);
    CHECK(view->step_count == misc[0] && view->team_captures[0] == misc[1] && view->team_captures[1] == misc[2] &&
              view->done == ((misc[3] & CTF_F_DONE) ? 1 : 0), "step count / captures / done");
    if (d.log_metrics)
        for (int k = 0; k < CTF_N_METRICS; k++)
            for (int i = 0; i < N; i++)
                CHECK(view->metrics[k][i] == h.metrics[((size_t)e * CTF_N_METRICS + k) * N + i], "metric %d of agent %d", k, i);
    return true;
}

static bool run_config(const char* name, ctf_config cfg, int n_envs, int steps) {
    ctf_config ocfg = cfg;
    cfg.rng_mode = CTF_RNG_COUNTER_DIRECT;
    ocfg.rng_mode = CTF_RNG_COUNTER;
    Sim h;
    if (!sim_create(h, &cfg, n_envs)) { printf("%s: derive failed: %s\n", name, g_err); return false; }
    const DevCfg& d = h.d;
    const int N = d.N;
    auto actions = exactly<int8_t>((size_t)n_envs * N);
    auto rw64 = exactly<double>((size_t)n_envs * N);
    auto done = exactly<uint8_t>((size_t)n_envs);
    auto orw = exactly<double>((size_t)N);
    auto view = std::unique_ptr<ctf_state_view>(new ctf_state_view());
    long long tags = 0, respawns = 0, py_words = 0, np_words = 0, env_steps = 0, py_beyond = 0, np_beyond = 0;
    bool ok = true;
    for (int e = 0; e < n_envs && ok; e++) {
        const uint64_t py_seed = 0x9E3779B97F4A7C15ull * (uint64_t)(e + 1) + 77, np_seed = py_seed ^ 0xABCDEF0123456789ull;
        octf_env* o = octf_create(&ocfg);
        if (!o) { printf("%s: octf_create failed\n", name); return false; }
        octf_seed(o, py_seed, np_seed);
        h.rngctr[4 * e] = 0; h.rngctr[4 * e + 1] = 0; h.rngctr[4 * e + 2] = py_seed; h.rngctr[4 * e + 3] = np_seed;  // k_seed
        if (e == 1) {  // one env far along its tapes: the high counter word
            const uint64_t far[2] = {(5ull << 32) - 9, (3ull << 32) + 2};
            octf_set_rng_counters(o, far);
            h.rngctr[4 * e] = far[0]; h.rngctr[4 * e + 1] = far[1];
        }
        ok = [&]() -> bool {
            for (int t = 0; t < steps; t++) {
                octf_get_state(o, view.get());
                if (view->done) octf_reset(o);
                octf_philox_actions(actions.get() + (size_t)e * N, N, 0xD1CEull, (uint32_t)t, (uint32_t)e);
                uint8_t odone = 0;
                uint64_t before[2], after[2];
                octf_get_rng_counters(o, before);
                const uint32_t ost = octf_step(o, actions.get() + (size_t)e * N, orw.get(), &odone);
                octf_get_rng_counters(o, after);
                h.status[0] = 0;
                if (d.log_metrics) step_env<true>(h, e, actions.get(), rw64.get(), done.get(), CTF_STEP_AUTO_RESET);
                else step_env<false>(h, e, actions.get(), rw64.get(), done.get(), CTF_STEP_AUTO_RESET);
                if (!same_as_oracle(name, e, t, h, o, view.get(), rw64.get(), done.get(), orw.get(), odone, ost, after)) return false;
                if (ost) return true;  // (no respawn cell: the reference raises there; nothing further to compare for this env)
                env_steps++;
                py_words += (long long)(after[0] - before[0]); np_words += (long long)(after[1] - before[1]);
                // (the windows start at the block of the first unconsumed word and end at their byte caps)
                py_beyond += (before[0] & 3) + (after[0] - before[0]) > (uint64_t)PY_DIRECT_BYTES;
                np_beyond += (before[1] & 3) + (after[1] - before[1]) > (uint64_t)NP_DIRECT_BYTES;
            }
            return true;
        }();
        if (ok && d.log_metrics)
            for (int i = 0; i < N; i++) {
                tags += h.metrics[((size_t)e * CTF_N_METRICS + CTF_M_TAG_COUNT) * N + i];
                respawns += h.metrics[((size_t)e * CTF_N_METRICS + CTF_M_RESPAWN_TAG_COUNT) * N + i];
            }
        octf_destroy(o);
    }
    if (ok)
        printf("OK %s: N %d, %lld env-steps, words per step py %.1f np %.1f, beyond the window caps py %lld np %lld, tags %lld respawns %lld\n", name, N,
               env_steps, env_steps ? (double)py_words / env_steps : 0.0, env_steps ? (double)np_words / env_steps : 0.0, py_beyond, np_beyond, tags,
               respawns);
    return ok;
}

// The tie sweep (tests/_tie_cases.py): np.random.rand() < TAG_PROBABILITY with the threshold chosen from the tape.  For the draw that
// starts at word n* = 2000 + r of the np.random tape, X = (w0 >> 5) << 26 | w1 >> 6, and TAG_PROBABILITY is X / 2^53 (the draw misses
// on equality), (X + 1) / 2^53 (it hits through hi == th && lo < tl) or the next multiple of 2^26 over 2^53 (it hits through hi < th).
// The env's np.random tape starts at n* - 2 k, so the step's k-th rand() is that draw; nobody moves; one step of the direct core
// against the oracle per (r, k, variant).  A k is deciding where the oracle's hp differs between the first two variants; which k are
// depends on the shuffled order, i.e. on the position py_n of the `random` tape.
static bool run_ties(const char* name, ctf_config cfg, uint64_t py_n) {
    const uint64_t py_seed = 77, np_seed = 77ull ^ 0xABCDEF0123456789ull, n_first = 2000;
    ctf_config ocfg = cfg;
    cfg.rng_mode = CTF_RNG_COUNTER_DIRECT;
    ocfg.rng_mode = CTF_RNG_COUNTER;
    DevCfg d0;
    if (derive(&cfg, 1, &d0)) { printf("%s: derive failed: %s\n", name, g_err); return false; }
    const int N = d0.N, pairs = d0.np_pairs;
    auto actions = exactly<int8_t>((size_t)N);
    for (int i = 0; i < N; i++) actions[i] = 4;
    auto rw64 = exactly<double>((size_t)N);
    auto orw = exactly<double>((size_t)N);
    auto done = exactly<uint8_t>(1);
    auto view = std::unique_ptr<ctf_state_view>(new ctf_state_view());
    auto hp = exactly<double>((size_t)3 * N);
    for (uint64_t r = 0; r < 4; r++) {
        const uint64_t n_star = n_first + r;
        uint32_t o0[4], o1[4];
        ctr_block(np_seed, n_star >> 2, 1u, o0);
        ctr_block(np_seed, (n_star + 1) >> 2, 1u, o1);
        const uint64_t X = ((uint64_t)(o0[n_star & 3] >> 5) << 26) | (o1[(n_star + 1) & 3] >> 6);
        const uint64_t thr[3] = {X, X + 1, ((X >> 26) + 1) << 26};
        int deciding = 0, inside = 0, edge = 0, beyond = 0;
        for (int k = 0; k < pairs; k++) {
            const uint64_t n0 = n_star - 2 * (uint64_t)k;
            const int e = 0, t = (int)(4 * k + r);  // (CHECK's labels)
            for (int v = 0; v < 3; v++) {
                cfg.tag_probability = ocfg.tag_probability = (double)thr[v] / 9007199254740992.0;
                Sim h;
                if (!sim_create(h, &cfg, 1)) { printf("%s: derive failed: %s\n", name, g_err); return false; }
                CHECK((((uint64_t)h.d.tag_th << 26) | h.d.tag_tl) == thr[v], "variant %d: threshold %llu, derived (%u, %u)", v,
                      (unsigned long long)thr[v], h.d.tag_th, h.d.tag_tl);
                octf_env* o = octf_create(&ocfg);
                if (!o) { printf("%s: octf_create failed\n", name); return false; }
                const uint64_t at[2] = {py_n, n0};
                octf_seed(o, py_seed, np_seed);
                octf_set_rng_counters(o, at);
                h.rngctr[0] = py_n; h.rngctr[1] = n0; h.rngctr[2] = py_seed; h.rngctr[3] = np_seed;
                uint8_t odone = 0;
                uint64_t after[2];
                const uint32_t ost = octf_step(o, actions.get(), orw.get(), &odone);
                octf_get_rng_counters(o, after);
                h.status[0] = 0;
                if (h.d.log_metrics) step_env<true>(h, 0, actions.get(), rw64.get(), done.get(), 0);
                else step_env<false>(h, 0, actions.get(), rw64.get(), done.get(), 0);
                const bool same = same_as_oracle(name, e, t, h, o, view.get(), rw64.get(), done.get(), orw.get(), odone, ost, after);
                for (int i = 0; i < N; i++) hp[(size_t)v * N + i] = view->hp[i];
                const bool whole = ost == 0 && after[1] - n0 == 2 * (uint64_t)pairs;
                octf_destroy(o);
                if (!same) { printf("  (tie sweep: n* %llu, k %d, variant %d)\n", (unsigned long long)n_star, k, v); return false; }
                CHECK(whole, "the step must draw its 2 * %d np.random words and nothing else (status %u)", pairs, ost);
            }
            CHECK(memcmp(&hp[(size_t)N], &hp[(size_t)2 * N], sizeof(double) * N) == 0, "the X + 1 and the next-hi thresholds must decide alike");
            if (memcmp(&hp[0], &hp[(size_t)N], sizeof(double) * N) == 0) continue;
            // the draw's first byte in the window, and what group_rng_setup parks of it
            const uint32_t off = (uint32_t)n0 & 3u, b = off + 2u * (uint32_t)k;
            uint32_t nb = (off + 2u * (uint32_t)pairs + NP_DIRECT_SLACK + 3u) >> 2;
            nb = nb < NP_DIRECT_BYTES / 4 ? nb : NP_DIRECT_BYTES / 4;
            const uint32_t fill = 4u * nb;
            deciding++;
            if (b + 1u < fill) inside++;
            else if (b == fill - 1u) edge++;
            else beyond++;
        }
        printf("TIES %s: py %d, r %d, deciding %d of %d k, b + 1 < fill %d, b == fill - 1 %d, b >= fill %d\n", name, (int)py_n, (int)r, deciding, pairs, inside, edge, beyond);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: direct_main [<config file> | --ties <config file>]...\n"); return 2; }
    printf("windows: NP_DIRECT_BYTES %d PY_DIRECT_BYTES %d\n", NP_DIRECT_BYTES, PY_DIRECT_BYTES);
    for (int a = 1; a < argc; a++) {
        const bool ties = strcmp(argv[a], "--ties") == 0;
        if (ties && ++a == argc) { printf("--ties needs a config file\n"); return 2; }
        ctf_config cfg;
        FILE* f = fopen(argv[a], "rb");
        if (!f) { printf("cannot open %s\n", argv[a]); return 2; }
        const size_t n = fread(&cfg, 1, sizeof(cfg), f);
        const bool whole = n == sizeof(cfg) && fgetc(f) == EOF;
        fclose(f);
        if (!whole) { printf("%s: not %zu bytes of ctf_config\n", argv[a], sizeof(cfg)); return 2; }
        // (`random` tape positions 3 and 20: two shuffles; the second puts deciding draws into the first bytes of the window)
        if (!(ties ? run_ties(argv[a], cfg, 3) && run_ties(argv[a], cfg, 20) : run_config(argv[a], cfg, 5, 80))) return 1;
    }
    printf("all direct-mode cases passed\n");
    return 0;
}
