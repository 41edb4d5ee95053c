// ctf_scatter.h — RANDOMISED EPISODE STARTS (ctf_reset_scattered; kernel in ctf_scatter.hip): the placement rule stated once, as plain
// inline functions that compile for the host and the device.  The kernel calls the pieces with one wave per env and sixteen cells per
// lane; sct_env_reset below walks the same pieces over one env cell by cell (the host test, tests/scatter/scatter_main.cpp).  The
// reference has no such reset: ctf_reset and the step's auto-reset still go to the config's start cells.
//
// The env becomes what ctf_reset leaves (ctf_step_core.h reset_record; `perm` and the generators untouched), except that the agents
// of agent_mask are placed, for i = 0 .. N - 1 in ascending order, s_i = start_pos[i]:
//   C_i     {s_i} and every cell c with init_grid[c] == 0 (OPEN), cheb(c, s_i) <= radius, c not taken by an earlier agent of this call
//           and — under CTF_SCATTER_OWN_SIDE — cheb(c, flag_pos[t]) <= cheb(c, flag_pos[1 - t]), t the agent's team.  s_i holds an
//           agent tile in the init grid, so it is never OPEN: nobody but i can draw it and n = |C_i| >= 1.  There is no failure case
//   r       round + (episode_dev ? episode_dev[e] : 0), a u32 add that wraps
//   w       Philox4x32-10(key = (seed lo, seed hi), counter = (env_offset + e, r, i, "SCT1")) — ctf_mt.h's, ctf_random_actions' generator
//   k       (w[0] * n) >> 32; the agent's cell is the (k + 1)-th element of C_i in ascending row-major cell index
//   then    pos[i] = cell, grid[s_i] = 0, grid[cell] = init_grid[s_i].  (No edit meets another: a start cell is never OPEN in the
//           init grid, so no agent lands on one but its own, and a drawn cell leaves the later agents' sets.)
// An agent outside agent_mask stands on s_i.  Visitation (log_metrics): when every agent stands on its s_i the env is exactly
// ctf_reset's (CTF_F_BASE_ZERO); otherwise the base maps are written out — zeros, 1 at each agent's cell, pad cells zero —
// CTF_F_BASE_ZERO is clear and the log is empty: the device form ctf_import_states gives those maps at step 0 (ctf_states.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ctf_device.h"
#include "ctf_effects.h"  // eff_cheb, eff_pack_row / eff_pack_col: the Chebyshev distance and the packed team cells

#define CTF_SCATTER_TAG 0x53435431u  // "SCT1": word 3 of the placement's counter

struct ScatterArgs {
    uint8_t* grid;             // u8 [E][GS]
    uint8_t* rec;              // u8 [E][RS]
    const uint8_t* init_grid;  // u8 [GS]
    int32_t* metrics;          // i32 [E][13][N] (log_metrics)
    uint32_t* vis;             // u32 [E][N][GS] (log_metrics)
    int32_t n_envs, N, G, GG, GS, RS, off_pos, off_flag, off_inv, off_misc, log_metrics;
    uint32_t team_mask;        // bit i = team(i)
    uint32_t type_pack;        // 2 bits per agent
    uint32_t flag_pack;        // the two teams' flag cells: row 0 | col 0 << 8 | row 1 << 16 | col 1 << 24
    uint64_t type_hp_bits[4];  // AGENT_TYPE_HP as f64 bits
    int8_t start_pos[CTF_MAX_AGENTS][2];
};

static inline ScatterArgs scatter_args(const DevCfg& d, const DevPtrs& p) {
    ScatterArgs A;
    A.grid = p.grid; A.rec = p.rec; A.init_grid = p.init_grid; A.metrics = p.metrics; A.vis = p.vis;
    A.n_envs = d.n_envs; A.N = d.N; A.G = d.G; A.GG = d.GG; A.GS = d.GS; A.RS = d.RS;
    A.off_pos = d.off_pos; A.off_flag = d.off_flag; A.off_inv = d.off_inv; A.off_misc = d.off_misc; A.log_metrics = d.log_metrics;
    A.team_mask = d.team_mask; A.type_pack = d.type_pack; A.flag_pack = d.flag_pack;
    for (int t = 0; t < 4; t++) __builtin_memcpy(&A.type_hp_bits[t], &d.type_hp[t], 8);
    __builtin_memcpy(A.start_pos, d.start_pos, sizeof(A.start_pos));
    return A;
}

// ---- the candidate predicate, in its three parts (the kernel keeps the first two as per-lane bit masks) -----------------------------
CTF_HD bool sct_open(int tile) { return tile == 0; }
// the cell is no further from team's own flag than from the other one
CTF_HD bool sct_own_side(uint32_t flag_pack, int team, int r, int c) {
    return eff_cheb(r, c, eff_pack_row(flag_pack, team), eff_pack_col(flag_pack, team)) <=
           eff_cheb(r, c, eff_pack_row(flag_pack, 1 - team), eff_pack_col(flag_pack, 1 - team));
}
CTF_HD bool sct_near(int r, int c, int sr, int sc, int32_t radius) { return eff_cheb(r, c, sr, sc) <= radius; }
// sct_near for sixteen consecutive cells base .. base + 15 at once (bit j = cell base + j; cells past the grid's last row: 0), row by
// row instead of cell by cell: the near cells of row rr are one run of columns.  row0 = base / G, row1 = (base + 15) / G (the caller
// keeps them: they do not depend on the agent).  tests/scatter/scatter_main.cpp holds it to sct_near on every cell
CTF_HD uint32_t sct_near16(int G, int base, int row0, int row1, int sr, int sc, int32_t radius) {
    const int R = radius < CTF_MAX_GRID ? radius : CTF_MAX_GRID;  // any radius >= G - 1 is the whole grid
    const int rlo = sr - R > 0 ? sr - R : 0, rhi = sr + R < G - 1 ? sr + R : G - 1;
    const int clo = sc - R > 0 ? sc - R : 0, chi = sc + R < G - 1 ? sc + R : G - 1;
    const int first = row0 > rlo ? row0 : rlo, last = row1 < rhi ? row1 : rhi;
    uint32_t bits = 0;
    for (int rr = first; rr <= last; rr++) {
        int a = rr * G + clo - base, z = rr * G + chi - base;  // the row's near cells, counted from the sixteen's first
        a = a > 0 ? a : 0;
        z = z < 15 ? z : 15;
        if (a <= z) bits |= (0xFFFFu >> (15 - z)) & (0xFFFFu << a);
    }
    return bits & 0xFFFFu;
}
// c = (r, c) belongs to C_i, `taken` aside: s_i itself, or OPEN in the init grid, within the radius and on the own side when asked
CTF_HD bool sct_candidate(const ScatterArgs& A, int init_tile, int r, int c, int i, int32_t radius, uint32_t flags) {
    const int sr = A.start_pos[i][0], sc = A.start_pos[i][1];
    if (r == sr && c == sc) return true;
    return sct_open(init_tile) && sct_near(r, c, sr, sc, radius) &&
           (!(flags & CTF_SCATTER_OWN_SIDE) || sct_own_side(A.flag_pack, (int)((A.team_mask >> i) & 1u), r, c));
}

// ---- the draw ---------------------------------------------------------------------------------------------------------------------
CTF_HD uint32_t sct_round(uint32_t round, uint32_t episode) { return round + episode; }  // wraps
// word 0 of agent i's Philox block; `env` is the env's GLOBAL index (env_offset + e).  It does not depend on the candidates: the
// kernel draws the agents' words side by side, one lane each, before it places anyone
CTF_HD uint32_t sct_word(uint64_t seed, uint32_t env, uint32_t r, uint32_t i) {
    uint32_t w[4];
    philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), env, r, i, CTF_SCATTER_TAG, w);
    return w[0];
}
// k among n candidates
CTF_HD uint32_t sct_pick(uint32_t w0, uint32_t n) { return (uint32_t)(((uint64_t)w0 * n) >> 32); }
CTF_HD uint32_t sct_draw(uint64_t seed, uint32_t env, uint32_t r, uint32_t i, uint32_t n) { return sct_pick(sct_word(seed, env, r, i), n); }

// ---- the record -------------------------------------------------------------------------------------------------------------------
// agent i's part of the reset record with the agent on `cell` (reset_record's bytes with another position)
template <typename BytePtr>
CTF_HD void sct_record_agent(const ScatterArgs& A, BytePtr sr, int i, int cell) {
    const uint64_t hb = A.type_hp_bits[(A.type_pack >> (2 * i)) & 3u];
    ((uint32_t*)(sr))[2 * i] = (uint32_t)hb;
    ((uint32_t*)(sr))[2 * i + 1] = (uint32_t)(hb >> 32);
    const int r = cell / A.G;
    sr[A.off_pos + 2 * i] = (uint8_t)r;
    sr[A.off_pos + 2 * i + 1] = (uint8_t)(cell - r * A.G);
    sr[A.off_flag + i] = 0;
    *(uint16_t*)(sr + A.off_inv + 2 * i) = 0;
}
// ... and the env's part: step count, captures, and misc[3] — not done, the log empty, base maps implicit unless somebody moved
template <typename BytePtr>
CTF_HD void sct_record_misc(const ScatterArgs& A, BytePtr sr, bool moved) {
    int32_t* misc = (int32_t*)(sr + A.off_misc);
    misc[0] = 0;
    misc[1] = 0;
    misc[2] = 0;
    misc[3] = moved ? 0 : CTF_F_BASE_ZERO;
}

// ---- one env, cell by cell (the host form) ------------------------------------------------------------------------------------------
// grid: GS bytes, rec: RS bytes, metrics: 13 N words or NULL, vis: N * GS words or NULL (both only with log_metrics).  `env` is the
// env's GLOBAL index, r = sct_round(round, episode).  cells[i] := agent i's cell.
static inline void sct_env_reset(const ScatterArgs& A, uint8_t* grid, uint8_t* rec, int32_t* metrics, uint32_t* vis, uint32_t agent_mask, int32_t radius,
                                 uint32_t flags, uint64_t seed, uint32_t env, uint32_t r, int* cells) {
    uint8_t taken[CTF_MAX_CELLS];
    for (int c = 0; c < A.GS; c++) grid[c] = A.init_grid[c];
    for (int c = 0; c < A.GG; c++) taken[c] = 0;
    bool moved = false;
    for (int i = 0; i < A.N; i++) {
        const int s = A.start_pos[i][0] * A.G + A.start_pos[i][1];
        int cell = s;
        if ((agent_mask >> i) & 1u) {
            uint32_t n = 0;
            for (int c = 0; c < A.GG; c++) n += (!taken[c] && sct_candidate(A, A.init_grid[c], c / A.G, c % A.G, i, radius, flags)) ? 1u : 0u;
            uint32_t k = sct_draw(seed, env, r, (uint32_t)i, n);
            for (int c = 0; c < A.GG; c++) {
                if (taken[c] || !sct_candidate(A, A.init_grid[c], c / A.G, c % A.G, i, radius, flags)) continue;
                if (k-- == 0) {
                    cell = c;
                    break;
                }
            }
        }
        taken[cell] = 1;
        moved = moved || cell != s;
        cells[i] = cell;
        grid[s] = 0;
        grid[cell] = A.init_grid[s];
        sct_record_agent(A, rec, i, cell);
    }
    sct_record_misc(A, rec, moved);
    if (A.log_metrics && metrics)
        for (int w = 0; w < CTF_N_METRICS * A.N; w++) metrics[w] = 0;
    if (A.log_metrics && vis && moved)
        for (int i = 0; i < A.N; i++)
            for (int c = 0; c < A.GS; c++) vis[(size_t)i * A.GS + c] = c == cells[i] ? 1u : 0u;
}
