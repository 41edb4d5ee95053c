// ctf_snapshot.h — the snapshot record of ONE env (ctf_save_states / ctf_load_states) and the config fingerprint that says which
// handles may exchange records.  Shared by the host code (ctf_abi.hip) and the gather / scatter kernels (ctf_snapshot.hip).
//
// A record is the env's device form copied as it is (ctf_device.h has the arrays), S bytes, S a multiple of 256:
//   header   64 B   u32 magic 'CTFS' | u32 layout version | u64 fingerprint | u32 S | u32 N | zeros
//   rec      RS     grid  GS
//   mt_py    u32 [2][624]   mt_np  u32 [2][624]      both rings of both streams, stale ones included
//   py_top   u32 [2][176]   np_hit u32 [2][26]   np_nib u32 [2][92]   (digests and mirrors)
//   rng      16 B   u32 rngpos[2] | u8 rngready[2], u8 rngage[2] | zeros
//   rngctr   u64 [6]                                  (counter mode only)
// (CTF_RNG_COUNTER_DIRECT: the five ring / digest segments and the rng segment are absent; rngctr u64 [4] is the RNG segment)
//   metrics  i32 [13][N], padded to 16 B              (log_metrics only)
//   vis      u32 [N][GS]                              (log_metrics only)
//   vislog   u16 [512][N], slot order                 (log_metrics only)
// then zeros up to S.  Every segment starts 16-byte aligned.  Nothing is converted: a ring that is stale (or waits for its tail
// block) is stale again after a restore, with its age, so a restored env replays bit for bit.  k_step_observe's sync words, the
// status word and the scratch buffers are not per-env state and are not part of the record.
#pragma once
#include <stdint.h>
#include <string.h>

#include "ctf_device.h"

#define CTF_SNAP_MAGIC 0x53465443u  // "CTFS" in memory order
#define CTF_SNAP_VERSION 1u
#define CTF_SNAP_HEADER 64
#define CTF_SNAP_ALIGN 256
#define CTF_SNAP_MAX_SEGS 11

// how a body segment moves: 16-byte vectors (its per-env stride is a multiple of 16), 32-bit words (the last 16-byte unit may be
// partial: the record side is zero-padded), or the packed 16-byte rng segment
enum { CTF_SNAP_VEC = 0, CTF_SNAP_WORDS = 1, CTF_SNAP_RNG = 2 };

struct SnapSeg {
    uint8_t* base;  // device array; env e's bytes start at base + e * bytes
    int32_t off;    // record offset (16-byte aligned)
    int32_t bytes;  // bytes per env
    int32_t kind;
    int32_t unit0;  // first 16-byte unit of the segment among the body's units
};

// everything the kernels need, computed on the host from the handle (snap_layout)
struct SnapLayout {
    uint64_t fingerprint;
    int32_t n_envs, N;
    int32_t bytes;       // S
    int32_t n_segs;      // body segments (all but the vislog column)
    int32_t body_units;  // 16-byte units of the body
    int32_t off_vislog;  // record offset of the vislog column, 0 = none (log_metrics off)
    SnapSeg seg[CTF_SNAP_MAX_SEGS];
    uint32_t* rngpos;
    uint8_t* rngready;
    uint8_t* rngage;
    uint16_t* vislog;
    uint32_t* status;
};

static inline int32_t snap_up16(int64_t x) { return (int32_t)((x + 15) / 16 * 16); }

static inline SnapLayout snap_layout(const DevCfg& d, const DevPtrs& p, uint64_t fingerprint) {
    SnapLayout L;
    memset(&L, 0, sizeof(L));
    L.fingerprint = fingerprint;
    L.n_envs = d.n_envs;
    L.N = d.N;
    int32_t off = CTF_SNAP_HEADER, units = 0;
    auto add = [&](void* base, int32_t bytes, int32_t kind) {
        SnapSeg& s = L.seg[L.n_segs++];
        s.base = (uint8_t*)base;
        s.off = off;
        s.bytes = bytes;
        s.kind = kind;
        s.unit0 = units;
        off += snap_up16(bytes);
        units += snap_up16(bytes) / 16;
    };
    add(p.rec, d.RS, CTF_SNAP_VEC);
    add(p.grid, d.GS, CTF_SNAP_VEC);
    if (d.rng_mode == CTF_RNG_COUNTER_DIRECT) {
        add(p.rngctr, 4 * 8, CTF_SNAP_VEC);
    } else {
        add(p.mt_py, 2 * CTF_MT_N * 4, CTF_SNAP_VEC);
        add(p.mt_np, 2 * CTF_MT_N * 4, CTF_SNAP_VEC);
        add(p.py_top, 2 * CTF_P8_DW * 4, CTF_SNAP_VEC);
        add(p.np_hit, 2 * CTF_HB_DW * 4, CTF_SNAP_VEC);
        add(p.np_nib, 2 * CTF_NB_DW * 4, CTF_SNAP_VEC);
        add(nullptr, 16, CTF_SNAP_RNG);
        if (d.rng_mode == CTF_RNG_COUNTER) add(p.rngctr, 6 * 8, CTF_SNAP_VEC);
    }
    if (d.log_metrics) {
        const int32_t mb = CTF_N_METRICS * d.N * 4;
        add(p.metrics, mb, mb % 16 == 0 ? CTF_SNAP_VEC : CTF_SNAP_WORDS);
        add(p.vis, d.N * d.GS * 4, CTF_SNAP_VEC);
        L.off_vislog = off;
        off += CTF_VIS_LOG * d.N * 2;  // a multiple of 16
    }
    L.body_units = units;
    L.bytes = (off + CTF_SNAP_ALIGN - 1) / CTF_SNAP_ALIGN * CTF_SNAP_ALIGN;
    L.rngpos = p.rngpos;
    L.rngready = p.rngready;
    L.rngage = p.rngage;
    L.vislog = p.vislog;
    L.status = p.status;
    return L;
}

// 64-bit FNV-1a over a canonical serialisation of what gives an env's state its meaning and its layout: every rule and constant of
// the config (only the entries in use: N agents, the teams' opponent lists, C - 1 channel tiles, G x G cells), the derived strides
// GS / RS, rng_mode and log_metrics, and the record's layout version.  Not the env count, the device, the seeds or the CTF_*
// environment switches.
struct Fnv64 {
    uint64_t h = 0xcbf29ce484222325ull;
    void bytes(const void* p, size_t n) {
        const uint8_t* b = (const uint8_t*)p;
        for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    }
    void i32(int32_t v) {
        const uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
        bytes(b, 4);
    }
    void f64(double v) {
        uint64_t u;
        memcpy(&u, &v, 8);
        i32((int32_t)(uint32_t)u);
        i32((int32_t)(uint32_t)(u >> 32));
    }
};

static inline uint64_t snap_fingerprint(const ctf_config* c, const DevCfg& d) {
    Fnv64 f;
    f.i32((int32_t)CTF_SNAP_MAGIC);
    f.i32((int32_t)CTF_SNAP_VERSION);
    const int32_t dims[] = {d.N, d.G, d.GS, d.RS, d.C, c->rng_mode, c->log_metrics ? 1 : 0, c->game_steps, c->flip_axis,
                            c->home_flag_capture, c->use_adjusted_rewards, c->drop_flag_when_no_hp, c->n_opponents[0], c->n_opponents[1]};
    for (int32_t v : dims) f.i32(v);
    const double rules[] = {c->heal_per_step, c->tag_probability, c->guardian_damage_multiplier, c->vault_hp_cost, c->vault_min_hp,
                            c->reward_capture, c->reward_step, c->reward_tag, c->win_margin_scalar, c->loss_margin_scalar,
                            c->opp_capture_punishment};
    for (double v : rules) f.f64(v);
    for (int t = 0; t < 4; t++) f.f64(c->type_hp[t]);
    for (int t = 0; t < 4; t++) f.f64(c->type_damage[t]);
    f.bytes(c->agent_team, (size_t)d.N);
    f.bytes(c->agent_type, (size_t)d.N);
    for (int t = 0; t < 2; t++) f.bytes(c->opponents[t], (size_t)c->n_opponents[t]);
    f.bytes(c->flag_pos, sizeof(c->flag_pos));
    f.bytes(c->capture_pos, sizeof(c->capture_pos));
    f.bytes(c->spawn_pos, sizeof(c->spawn_pos));
    f.bytes(c->start_pos, (size_t)d.N * 2);
    f.bytes(c->tile_of_channel + 1, (size_t)(d.C - 1));
    f.bytes(c->init_grid, (size_t)d.GG);
    return f.h;
}
