// The metadata values and rows of marl-ctf-development_amd/csrc/ctf_meta.h on the CPU, against the oracle's get_env_metadata.
// A stand-alone program (built with AddressSanitizer + UBSan by tests/test_step_meta_cpu.py):
//
//   meta_main CASES.bin      CASES.bin = records back to back: a ctf_config, an int32 count K, K ctf_state_view structs.
//                            K = 0: the program makes the config's states itself, by random play on the oracle.
//
// 1. f64_to_f16 on every binary16 value, on every midpoint between two neighbours and on the doubles next to each midpoint (every
//    class of the rounding: exact, down, up, ties to even and to odd, the carry into the exponent, the largest finite value, overflow
//    by rounding, subnormals, the carry into the smallest normal, underflow), on zeros, infinities, NaNs, subnormal doubles and
//    negative values, against what the value's position says and against the oracle's own conversion; meta_u8_to_f16 on 0 .. 255
//    against f64_to_f16; meta_hp_u8 at the uint8 wrap.
// 2. Per config, every state's rows made BOTH ways must be the oracle's, bit for bit:
//    - the step kernels' way (step_block with W = 1, 64 envs per wave): the records laid out in the wave's slots, the lanes 0 .. 63
//      running meta_park_fracs, meta_park_agents and meta_gather_store one phase after the other, into a buffer with guard bands.
//      The states are laid out three times over, rotated, so that blocks start at other envs than 0 and end ragged;
//    - the renders' way (obs_build_env, phase A and B): a value per lane from the header's rules, then the table.
// A unit test of code the device shares, not a CPU path of the product.
#define CTF_HOSTSIM 1
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../marl-ctf-development_amd/csrc/ctf_meta.h"

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    fputc('\n', stderr);
    va_end(ap);
    return code;
}
#include "../../marl-ctf-development_amd/csrc/ctf_derive.h"
#include "../../oracle/ctf_oracle.h"

static const int LANES = 64;  // the wave; W = 1: a lane per env
static const uint16_t GUARD = 0xBEEF;
static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad++ < 20) { fprintf(stderr, "FAIL: " __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static double half_value(uint32_t h) {  // 0 <= h <= 0x7C00 (0x7C00: 65536, the first value past the format, for the midpoints)
    const int e = (int)(h >> 10), m = (int)(h & 0x3FF);
    return e == 0 ? ldexp((double)m, -24) : ldexp((double)(1024 + m), e - 25);
}

static void conversion_checks() {
    long n = 0;
    auto both = [&](double d, uint32_t want, const char* what) {
        n++;
        CHECK(f64_to_f16(d) == want, "f64_to_f16(%a) = %#x, expected %#x (%s)", d, f64_to_f16(d), want, what);
        CHECK(octf_f64_to_f16(d) == want, "the oracle's conversion of %a = %#x, expected %#x (%s)", d, octf_f64_to_f16(d), want, what);
        CHECK(f64_to_f16(-d) == (want | 0x8000u), "f64_to_f16(%a) = %#x, expected %#x (%s, negative)", -d, f64_to_f16(-d), want | 0x8000u, what);
    };
    for (uint32_t h = 0; h < 0x7C00; h++) {
        const double v = half_value(h), up = half_value(h + 1), mid = 0.5 * (v + up);  // exact: a half has 11 significant bits
        const uint32_t next = h + 1;  // (0x7BFF + 1 = 0x7C00: infinity, "overflow by rounding"; 0x03FF + 1: the smallest normal)
        both(v, h, "exact");
        both(mid, (h & 1u) ? next : h, "tie");
        both(nextafter(mid, 0.0), h, "below the tie");
        both(nextafter(mid, 1e300), next, "above the tie");
        both(nextafter(up, 0.0), next, "just below the next value");
        if (h) both(nextafter(v, 1e300), h, "just above the value");
    }
    both(65536.0, 0x7C00, "overflow");
    both(2147483647.0, 0x7C00, "overflow");
    both(1e300, 0x7C00, "overflow");
    both(INFINITY, 0x7C00, "infinity");
    both(ldexp(1.0, -26), 0, "underflow");
    both(ldexp(1.0, -60), 0, "underflow");
    both(4.9406564584124654e-324, 0, "subnormal double");
    both(2.2250738585072009e-308, 0, "largest subnormal double");
    CHECK(f64_to_f16(0.0) == 0 && f64_to_f16(-0.0) == 0x8000, "zeros");
    CHECK(f64_to_f16((double)NAN) == octf_f64_to_f16((double)NAN) && (f64_to_f16((double)NAN) & 0x7C00) == 0x7C00 && (f64_to_f16((double)NAN) & 0x3FF),
          "NaN: %#x, the oracle %#x", f64_to_f16((double)NAN), octf_f64_to_f16((double)NAN));
    // the integer path: exact on all of its domain
    for (uint32_t v = 0; v < 256; v++)
        CHECK(meta_u8_to_f16(v) == f64_to_f16((double)v), "meta_u8_to_f16(%u) = %#x, f64_to_f16 gives %#x", v, meta_u8_to_f16(v), f64_to_f16((double)v));
    CHECK(meta_u8_to_f16(0) == 0 && meta_u8_to_f16(1) == 0x3C00 && meta_u8_to_f16(2) == 0x4000 && meta_u8_to_f16(255) == 0x5BF8 && meta_u8_to_f16(128) == 0x5800,
          "meta_u8_to_f16 at 0, 1, 2, 128, 255: %#x %#x %#x %#x %#x", meta_u8_to_f16(0), meta_u8_to_f16(1), meta_u8_to_f16(2), meta_u8_to_f16(128), meta_u8_to_f16(255));
    printf("ok conversions: %ld doubles (and their negatives) through f64_to_f16, 256 integers through meta_u8_to_f16\n", n);
}

// the record of a state: what the metadata reads of it (hp, has_flag, the four misc words); everything else poisoned
static void record_of(const DevCfg& d, const ctf_state_view& v, uint8_t* rec) {
    memset(rec, 0xA5, (size_t)d.RS);
    memcpy(rec, v.hp, 8 * (size_t)d.N);
    for (int i = 0; i < d.N; i++) rec[d.off_flag + i] = v.has_flag[i];
    const int32_t misc[4] = {v.step_count, v.team_captures[0], v.team_captures[1], (int32_t)(0x7F00 | (v.done ? CTF_F_DONE : 0))};
    memcpy(rec + d.off_misc, misc, 16);
}

// the renders' way: obs_build_env's phases A and B
static void rows_render_way(const DevCfg& d, const uint8_t* srec, const uint8_t* lut, uint16_t* out) {
    uint16_t mv[64];
    for (int k = 0; k < 64; k++) mv[k] = 0xEEEE;
    const int32_t* misc = (const int32_t*)(srec + d.off_misc);
    const int N = d.N;
    for (int lane = 0; lane < 36; lane++) {
        double val = 0.0;
        if (lane == META_MV_STEP) val = meta_step_fraction(misc[0], d.game_steps);
        else if (lane < META_MV_RATIO + 2) val = meta_capture_ratio(misc[lane], misc[3 - lane]);
        else if (lane >= META_MV_HP && lane < META_MV_HP + N) val = (double)meta_hp_u8(d, srec, lane - META_MV_HP);
        else if (lane >= META_MV_FLAG && lane < META_MV_FLAG + N) val = (double)srec[d.off_flag + lane - META_MV_FLAG];
        mv[lane] = f64_to_f16(val);
    }
    mv[META_MV_ONE] = 0x3C00;
    mv[META_MV_ZERO] = 0;
    for (int idx = 0; idx < N * d.M; idx++) out[idx] = mv[lut[idx]];
}

// the step kernels' way for `count` envs whose records are recs[e]: step blocks of 64 envs, -> rows [count][N][M]
static void rows_step_way(const DevCfg& d, const std::vector<std::vector<uint8_t>>& recs, const uint8_t* lut, std::vector<uint16_t>& rows,
                          const char* what) {
    const int count = (int)recs.size(), NM = d.N * d.M, band = 64;
    const int SLB = step_slot_bytes(d.GS, d.RS, d.N, true);
    std::vector<uint16_t> buf((size_t)count * NM + 2 * band, GUARD);  // (operator new: 16-byte aligned, as a caller's 8-byte aligned buffer may be)
    std::vector<uint32_t> lds((size_t)LANES * SLB / 4);
    const uint32_t chunk_div = meta_chunk_div(d.N, d.M);
    for (int q = 0, D = NM / 4; q < LANES * D; q++)
        CHECK((int)(((uint32_t)q * chunk_div) >> 24) == q / D, "%s: chunk %d / %d by the reciprocal is %u", what, q, D, ((uint32_t)q * chunk_div) >> 24);
    for (int env0 = 0; env0 < count; env0 += LANES) {
        const int nvalid = count - env0 < LANES ? count - env0 : LANES;
        memset(lds.data(), 0x5A, lds.size() * 4);  // whatever the step left in the slots
        for (int el = 0; el < nvalid; el++) memcpy((uint8_t*)lds.data() + (size_t)el * SLB + d.GS, recs[env0 + el].data(), (size_t)d.RS);
        const MetaSlots ms = {(uint8_t*)lds.data(), SLB, d.GS, d.GS + d.RS};
        for (int lane = 0; lane < LANES; lane++) meta_park_fracs(d, ms, nvalid, lane, LANES);
        for (int lane = 0; lane < LANES; lane++) meta_park_agents(d, ms, nvalid, lane, LANES);
        for (int el = 0; el < nvalid; el++) {  // the parked values stay inside the slot's dead bytes and leave the record alone
            CHECK(memcmp((uint8_t*)lds.data() + (size_t)el * SLB + d.GS, recs[env0 + el].data(), (size_t)d.RS) == 0, "%s: env %d: the record changed", what, env0 + el);
            const uint8_t* after = (uint8_t*)lds.data() + (size_t)el * SLB + d.GS + d.RS + 2 * META_MV_COUNT;
            for (int k = 0; k < 16 + NP_NIB_BYTES + PY_TOP_BYTES - 2 * META_MV_COUNT; k++) CHECK(after[k] == 0x5A, "%s: env %d: byte %d behind the parked values", what, env0 + el, k);
        }
        for (int lane = 0; lane < LANES; lane++) meta_gather_store(d, ms, lut, chunk_div, nvalid, lane, LANES, buf.data() + band + (size_t)env0 * NM);
    }
    for (int k = 0; k < band; k++) CHECK(buf[k] == GUARD && buf[buf.size() - 1 - k] == GUARD, "%s: a guard band was written", what);
    rows.assign(buf.begin() + band, buf.end() - band);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (uint32_t)(((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s CASES.bin\n", argv[0]); return 2; }
    conversion_checks();
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    ctf_config* cfg = new ctf_config;
    int n_cfg = 0;
    bool wrap_seen = false;
    while (fread(cfg, sizeof(*cfg), 1, f) == 1) {
        int32_t K = 0;
        if (fread(&K, 4, 1, f) != 1 || K < 0 || K > 4096) { fprintf(stderr, "config %d: bad count\n", n_cfg); return 2; }
        std::vector<ctf_state_view> states((size_t)K);
        if (K && fread(states.data(), sizeof(ctf_state_view), (size_t)K, f) != (size_t)K) { fprintf(stderr, "config %d: short file\n", n_cfg); return 2; }
        octf_env* env = octf_create(cfg);
        if (!env) { fprintf(stderr, "config %d: octf_create failed\n", n_cfg); return 2; }
        const bool played = K == 0;
        if (played) {  // random play with resets: 70 states
            octf_seed(env, 5000 + 7 * (uint64_t)n_cfg, 6000 + 7 * (uint64_t)n_cfg);
            octf_reset(env);
            uint8_t done = 0;
            for (int t = 0; t < 70; t++) {
                int8_t actions[CTF_MAX_AGENTS];
                double rewards[CTF_MAX_AGENTS];
                if (done || rnd(29) == 0) { octf_reset(env); done = 0; }
                for (int i = 0; i < cfg->n_agents; i++) actions[i] = (int8_t)rnd(9);
                if (octf_step(env, actions, rewards, &done) & (CTF_ST_NO_RESPAWN | CTF_ST_SPAWN_EDGE)) { octf_reset(env); done = 0; }
                states.emplace_back();
                octf_get_state(env, &states.back());
            }
            K = (int)states.size();
        }
        DevCfg d;
        if (derive(cfg, 3 * K, &d)) return 2;
        std::vector<uint8_t> lut((size_t)round_up(d.N * d.M, 16), 0xFF);
        host_meta_lut(d, lut.data());
        const int NM = d.N * d.M;
        char what[96];
        snprintf(what, sizeof(what), "config %d (N %d, M %d)", n_cfg, d.N, d.M);
        // the oracle's rows of every state
        std::vector<uint16_t> want((size_t)K * NM);
        std::vector<uint8_t> planes((size_t)d.obs_bytes);
        for (int k = 0; k < K; k++) {
            octf_set_state(env, &states[k]);
            octf_observe(env, planes.data(), want.data() + (size_t)k * NM, 0);
        }
        // three times over, rotated by 0, 7 and 29 states
        std::vector<std::vector<uint8_t>> recs;
        std::vector<int> src;
        const int rot[3] = {0, 7, 29};
        for (int rep = 0; rep < 3; rep++)
            for (int k = 0; k < K; k++) {
                src.push_back((k + rot[rep]) % K);
                recs.emplace_back((size_t)d.RS);
                record_of(d, states[src.back()], recs.back().data());
            }
        std::vector<uint16_t> rows, one((size_t)NM);
        rows_step_way(d, recs, lut.data(), rows, what);
        long diff_step = 0, diff_render = 0;
        for (size_t e = 0; e < recs.size(); e++) {
            const uint16_t* w = want.data() + (size_t)src[e] * NM;
            for (int k = 0; k < NM; k++) diff_step += rows[e * NM + k] != w[k];
            if (e < (size_t)K) {
                rows_render_way(d, recs[e].data(), lut.data(), one.data());
                for (int k = 0; k < NM; k++) diff_render += one[k] != w[k];
            }
        }
        CHECK(diff_step == 0, "%s: %ld elements of the step kernels' rows differ from the oracle's", what, diff_step);
        CHECK(diff_render == 0, "%s: %ld elements of the renders' rows differ from the oracle's", what, diff_render);
        if (n_cfg == 0) {
            // the cast to uint8 wraps: quotients 256, 300 and 511.5 show 0, 44 and 255 (planted into the record alone: the reference's
            // own cast is undefined there, so no oracle is asked)
            const double qs[3] = {256.0, 300.0, 511.5};
            const uint32_t shown[3] = {0, 44, 255};
            for (int j = 0; j < d.N; j++) {
                const int tv = d.type[j];
                if (tv >= d.N) continue;
                for (int k = 0; k < 3; k++) {
                    std::vector<uint8_t> rec(recs[0]);
                    const double hp = qs[k] * d.type_hp[tv];
                    memcpy(rec.data() + 8 * tv, &hp, 8);
                    CHECK(meta_hp_u8(d, rec.data(), j) == shown[k], "%s: hp quotient %g of agent %d shows %u, expected %u", what, qs[k], j, meta_hp_u8(d, rec.data(), j), shown[k]);
                    wrap_seen = true;
                }
            }
        }
        if (g_bad) { fprintf(stderr, "FAIL %s\n", what); return 1; }
        printf("ok config %d: N %d, %d states%s, %zu envs in %zu step blocks the step kernels' way, %d the renders' way\n", n_cfg, d.N, K,
               played ? " (played)" : "", recs.size(), (recs.size() + LANES - 1) / LANES, K);
        octf_destroy(env);
        n_cfg++;
    }
    fclose(f);
    delete cfg;
    if (g_bad || !n_cfg || !wrap_seen) { fprintf(stderr, "FAIL: %d checks failed, %d configs, wrap seen %d\n", g_bad, n_cfg, (int)wrap_seen); return 1; }
    printf("all step-meta cases passed\n");
    return 0;
}
