// ctf_meta.h — the one definition of an env's metadata values (get_env_metadata, gridworld_ctf.py:1027-1069) and of the two ways
// the kernels make the f16 [N][M] rows from them.
//
// Every element of an env's N x M block shows one of at most 36 distinct values and two constants; mv[] holds them as binary16
// bits, and the table of ctf_derive.h (host_meta_lut, DevPtrs.meta_lut) says which one each element shows:
//   mv[META_MV_STEP]        env_step_count / GAME_STEPS
//   mv[META_MV_RATIO + t]   (captures[t] + 1) / (captures[1 - t] + 1): what a viewer of team t sees
//   mv[META_MV_HP + j]      the uint8-truncated hp quotient of agent j — with the reference's quirk (:1039-1041): the hp of the agent
//                           whose INDEX is type(j), over the full hp of type(j)
//   mv[META_MV_FLAG + j]    has_flag[j]
//   mv[META_MV_ONE / ZERO]  1.0 and 0.0 (the one-hot type columns, the padding)
// The renders make them one env per wave (obs_build_env, ctf_render_dev.h: a value per lane, then f64_to_f16).  The step kernels
// make them for all the envs of a wave at once (step_block, ctf_step_block.h), from the final records they hold in LDS:
// meta_park_fracs and meta_park_agents lay the (env, value) pairs flat over the lanes and park each env's mv[] in its slot,
// meta_gather_store then writes the wave's rows as flat 8-byte chunks.  The small integers (hp quotients, flags) take the exact
// meta_u8_to_f16 there instead of the general conversion.
//
// Compiled for the device by ctf_kernels.hip / ctf_observe_delta.hip / ctf_step_direct.hip and, with CTF_HOSTSIM defined, for the host by
// tests/hostsim/meta_main.cpp, which holds both ways to the oracle's metadata without a GPU.
#pragma once
#include "ctf_step_core.h"

#define META_MV_STEP 0
#define META_MV_RATIO 1
#define META_MV_HP 4
#define META_MV_FLAG 20
#define META_MV_ONE 40
#define META_MV_ZERO 41
#define META_MV_COUNT 42  // halfwords of an env's mv[]: 84 bytes

// NumPy npy_double_to_half: direct round-to-nearest-even f64 -> binary16 bits
CTF_DEV uint16_t f64_to_f16(double d) {
    uint64_t b = ctf_double_bits(d);
    uint32_t sign = (uint32_t)((b >> 48) & 0x8000u);
    int32_t be = (int32_t)((b >> 52) & 0x7FF);
    uint64_t m = b & 0xFFFFFFFFFFFFFull;
    if (be == 0x7FF) return (uint16_t)(sign | 0x7C00u | (m ? (0x200u | (uint32_t)(m >> 42)) : 0u));
    if (be == 0) return (uint16_t)sign;
    int32_t E = be - 1023;
    if (E > 15) return (uint16_t)(sign | 0x7C00u);
    if (E >= -14) {
        uint32_t h = (uint32_t)((E + 15) << 10) | (uint32_t)(m >> 42);
        uint64_t rem = m & ((1ull << 42) - 1), half = 1ull << 41;
        if (rem > half || (rem == half && (h & 1u))) h++;
        return (uint16_t)(sign | h);
    }
    if (E < -25) return (uint16_t)sign;
    uint64_t full = m | (1ull << 52);
    int shift = 28 - E;
    uint64_t h = full >> shift, rem = full & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (h & 1u))) h++;
    return (uint16_t)(sign | (uint32_t)h);
}
// the same for an integer 0 <= v < 256: eight significant bits at most, so the conversion is exact and needs no rounding
CTF_DEV uint16_t meta_u8_to_f16(uint32_t v) {
    // with e = floor(log2 v) = 31 - lz: exponent e + 15, the leading one shifted to bit 10 (by 10 - e) and masked off — written in
    // lz itself, so that the instructions do not depend on how the compiler happens to fold the two subtractions
    const int lz = ctf_clz(v | 1u);  // 24 .. 31; (v | 1: defined at 0, whose result the select below replaces)
    const uint32_t h = ((uint32_t)(46 - lz) << 10) | ((v << (lz - 21)) & 0x3FFu);
    return (uint16_t)(v ? h : 0u);
}

// ---- the values, as the reference computes them (f64 throughout)
CTF_DEV double meta_quotient(int32_t num, int32_t den) { return (double)num / (double)den; }
CTF_DEV double meta_step_fraction(int32_t step_count, int32_t game_steps) { return meta_quotient(step_count, game_steps); }
// what a viewer sees whose own team has `own` captures (the sums are int32, as the device's always were)
CTF_DEV double meta_capture_ratio(int32_t own, int32_t other) { return meta_quotient(own + 1, other + 1); }
// the hp element of agent j from the env's record `srec` (hp: f64 [N] at offset 0): the quirk at :1039-1041 and the cast to uint8
template <typename BytePtr>
CTF_DEV uint32_t meta_hp_u8(const DevCfg& cfg, BytePtr srec, int j) {
    const int tv = cfg_type(cfg, j);
    double q = 0.0;
    if (tv < cfg.N) {
        const uint32_t* hq = (const uint32_t*)(srec + 8 * tv);
        q = ctf_hilo2double(hq[1], hq[0]) / sel4(cfg.type_hp, tv);
    }
    return (uint32_t)(uint8_t)(long long)q;
}

// ---- the step kernels' way: the final records of a wave's envs sit in slots `stride` bytes apart, the record `rec_off` bytes
// into its slot; `park_off`: META_MV_COUNT halfwords of the slot that nothing needs any more (4-byte aligned).  `lane` of `wave`
// lanes does its share; the envs are 0 .. nvalid-1.
struct MetaSlots {
    uint8_t* base;
    int stride, rec_off, park_off;
};
CTF_DEV uint16_t* meta_parked(const MetaSlots& s, int el) { return (uint16_t*)(s.base + el * s.stride + s.park_off); }

// the step fraction and the two capture ratios of every env, one division sequence per pass of `wave` (env, value) pairs; the lane
// of an env's step fraction also parks the two constants
CTF_DEV void meta_park_fracs(const DevCfg& cfg, const MetaSlots& s, int nvalid, int lane, int wave) {
    for (int t = lane; t < 3 * nvalid; t += wave) {
        const int el = t / 3, k = t - 3 * el;
        const int32_t* misc = (const int32_t*)(s.base + el * s.stride + s.rec_off + cfg.off_misc);
        const int32_t a = misc[k], b = misc[3 - k];  // (k = 0: b is the flags word and goes unused)
        const double val = meta_quotient(k ? a + 1 : a, k ? b + 1 : cfg.game_steps);
        uint16_t* mv = meta_parked(s, el);
        mv[k] = f64_to_f16(val);  // META_MV_STEP, META_MV_RATIO + 0 / 1
        if (k == 0) *(uint32_t*)(mv + META_MV_ONE) = 0x00003C00u;  // 1.0, then 0.0
    }
}
// the hp element and the flag of every (env, agent)
CTF_DEV void meta_park_agents(const DevCfg& cfg, const MetaSlots& s, int nvalid, int lane, int wave) {
    const int N = cfg.N;
    for (int t = lane; t < nvalid * N; t += wave) {
        const int el = (int)fdiv((uint32_t)t, cfg.div_n), j = t - el * N;
        const uint8_t* srec = s.base + el * s.stride + s.rec_off;
        uint16_t* mv = meta_parked(s, el);
        mv[META_MV_HP + j] = meta_u8_to_f16(meta_hp_u8(cfg, srec, j));
        mv[META_MV_FLAG + j] = meta_u8_to_f16(srec[cfg.off_flag + j]);
    }
}
// The rows of the wave's envs are consecutive in the caller's buffer: nvalid * N * M halfwords from `dst` on.  An env's block is
// 4 N (N + 3) bytes, always whole 8-byte chunks (and the callers' buffers are 8-byte aligned, no more: ctf_abi.hip), so chunk q
// of the flat run belongs to one env, el = q / D with D = N * M / 4 chunks per env.  q stays below 64 * 152 and D below 2**8, so
// el is (q * ceil(2**24 / D)) >> 24 exactly: the product errs by less than q * D / 2**24 < 1 / D of a unit and stays below 2**31.
static inline uint32_t meta_chunk_div(int N, int M) { return (uint32_t)(((1u << 24) + (uint32_t)(N * M / 4) - 1u) / (uint32_t)(N * M / 4)); }
CTF_DEV void meta_gather_store(const DevCfg& cfg, const MetaSlots& s, const uint8_t* lut, uint32_t chunk_div, int nvalid, int lane, int wave,
                               uint16_t* dst) {
    const int D = cfg.N * cfg.M / 4;
    for (int q = lane; q < nvalid * D; q += wave) {
        const int el = (int)(((uint32_t)q * chunk_div) >> 24), r = q - el * D;
        const uint32_t l4 = ((const uint32_t*)lut)[r];  // which value each of the chunk's four elements shows
        const uint16_t* mv = meta_parked(s, el);
        const uint32_t lo = (uint32_t)mv[l4 & 0xFFu] | ((uint32_t)mv[(l4 >> 8) & 0xFFu] << 16);
        const uint32_t hi = (uint32_t)mv[(l4 >> 16) & 0xFFu] | ((uint32_t)mv[l4 >> 24] << 16);
        ((unsigned long long*)dst)[q] = (unsigned long long)lo | ((unsigned long long)hi << 32);
    }
}
