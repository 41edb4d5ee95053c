// ctf_scripted.h — the scripted opponents (ctf_scripted_actions, ctf_scripted.hip): the policy, defined once as plain inline
// functions that compile for the host and the device.  The kernel calls them with one lane per grid ROW; scr_env_actions below walks
// the same functions over an array of rows, one env at a time (the host test, tests/scripted/scripted_main.cpp).
//
// CTF_SCRIPT_RUNNER, agent a of team t, a pure function of the env state (grid, positions, has_flag) and the config:
//   target   T = flag_pos[t] if has_flag[a], else flag_pos[1 - t]: standing next to T is what the pickup and capture rules test
//   goals    the cells inside the grid within Chebyshev distance 1 of T whose tile is OPEN (0)
//   d        BFS distance over OPEN cells, 4-neighbour unit moves, goals at 0; every other tile is a wall — blocks, destructibles,
//            flags and agents (agents are tiles of the grid, the asking agent's own cell included)
//   action   the lowest-numbered of 0..3 (deltas (-1,0), (1,0), (0,1), (0,-1)) whose neighbour is inside the grid and has the
//            minimum finite d; none: 4 (stay).  5..8 are never chosen: every agent type's action mask is respected
//   explore  w = Philox4x32-10(key = seed, counter = (global env, step, a, "BOT1")); w[0] < epsilon_q32 replaces the action by
//            mulhi(w[1], 5), uniform on 0..4.  epsilon_q32 == 0 computes no Philox block.
// These are ENV actions (the state is read, not a flipped observation): they go to ctf_step as they are.
//
// BIT-PARALLEL FORM.  G <= 32: a grid is 32 row masks (bit c of row r = cell (r, c)), and one BFS step is
//   next = (f << 1 | f >> 1 | f[r - 1] | f[r + 1]) & open & ~seen.
// The four terms are also the four NEIGHBOURS of every cell of row r, so the row that holds an asking agent sees, in the very
// iteration n in which a neighbour joins the frontier, that this neighbour has d = n: the first iteration in which any of the four
// terms covers the agent's bit decides its action (lowest term first), and nothing but three masks per row (decided, action bit 0,
// action bit 1) is kept — no distance array.  A FIELD is (team, carrying or not): agents of one field that share a cell share the
// answer, so a row mask of askers per field is all the bookkeeping.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ctf_device.h"

#define CTF_SCRIPT_TAG 0x424F5431u  // "BOT1": word 3 of the exploration counter

struct ScriptArgs {
    const uint8_t* grid;  // u8 [E][GS]
    const uint8_t* rec;   // u8 [E][RS]: i8 pos[N][2] at off_pos, u8 has_flag[N] at off_flag
    int32_t n_envs, N, G, GS, RS, off_pos, off_flag;
    uint32_t team_mask;   // bit i = team(i)
    uint32_t flag_pack;   // flag cells: row 0 | col 0 << 8 | row 1 << 16 | col 1 << 24
};

static inline ScriptArgs script_args(const DevCfg& d, const DevPtrs& p) {
    return ScriptArgs{p.grid, p.rec, d.n_envs, d.N, d.G, d.GS, d.RS, d.off_pos, d.off_flag, d.team_mask, d.flag_pack};
}
// bit t = some agent of agent_mask plays for team t
static inline uint32_t script_teams(const ScriptArgs& A, uint32_t agent_mask) {
    uint32_t teams = 0;
    for (int i = 0; i < A.N; i++)
        if ((agent_mask >> i) & 1u) teams |= 1u << ((A.team_mask >> i) & 1u);
    return teams;
}

// bit b = (byte b of v == 0)
CTF_HD uint32_t scr_zero_bytes(uint32_t v) {
    const uint32_t z = ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);  // 0x80 in every zero byte, no carry between bytes
    return (((z >> 7) * 0x00204081u) >> 21) & 15u;                             // bits 0, 8, 16, 24 -> 21, 22, 23, 24
}
// row r of the OPEN mask of one env's grid (GS bytes, 4-byte aligned, GS a multiple of 4); 0 for r >= G.  Whole dwords on clamped
// indices: a row starts at any byte, so nine dwords cover its G <= 32 bytes wherever it lies; what they hold past the row (the next
// row, the pad bytes GG..GS, the last dword again) lands at columns >= G and is masked off.
CTF_HD uint32_t scr_row_open(const uint8_t* grid, int G, int GS, int r) {
    const int rr = r < G ? r : G - 1;
    const int b0 = rr * G, w0 = b0 >> 2, last = (GS >> 2) - 1;
    const uint32_t* words = (const uint32_t*)grid;
    uint32_t v[9];
#pragma unroll
    for (int j = 0; j < 9; j++) v[j] = words[(size_t)(w0 + j < last ? w0 + j : last)];  // all in flight together
    uint64_t acc = 0;
#pragma unroll
    for (int j = 0; j < 9; j++) acc |= (uint64_t)scr_zero_bytes(v[j]) << (4 * j);
    const uint32_t bits = (uint32_t)(acc >> (b0 & 3)) & (G >= 32 ? 0xFFFFFFFFu : (1u << G) - 1u);
    return r < G ? bits : 0u;
}
// the target cell of field (team, carrying)
CTF_HD void scr_target(uint32_t flag_pack, int team, int carrying, int& tr, int& tc) {
    const int t = carrying ? team : 1 - team;
    tr = (int)((flag_pack >> (16 * t)) & 0xFFu);
    tc = (int)((flag_pack >> (16 * t + 8)) & 0xFFu);
}
// row r of the goal cells: the 3 x 3 window round the target, clipped by the grid, open cells only
CTF_HD uint32_t scr_goal_row(uint32_t open, int r, int tr, int tc) {
    const uint32_t cols = (uint32_t)((7ull << tc) >> 1);
    return (r >= tr - 1 && r <= tr + 1) ? open & cols : 0u;
}
// one BFS step of a row: up / down = the frontier of rows r - 1 / r + 1 (0 outside the grid)
CTF_HD uint32_t scr_step(uint32_t f, uint32_t up, uint32_t down, uint32_t open, uint32_t seen) { return ((f << 1) | (f >> 1) | up | down) & open & ~seen; }

// what a row keeps of its askers: who is decided, and the two bits of the action
struct ScrPick {
    uint32_t dec, b0, b1;
};
// frontier f of this iteration against the askers P of the row: an asker whose neighbour (-1,0) / (1,0) / (0,1) / (0,-1) is in the
// frontier for the first time takes that action, the lowest-numbered one
CTF_HD void scr_pick(ScrPick& k, uint32_t P, uint32_t f, uint32_t up, uint32_t down) {
    const uint32_t a0 = up, a1 = down, a2 = f >> 1, a3 = f << 1;
    const uint32_t now = (a0 | a1 | a2 | a3) & P & ~k.dec;
    k.b0 |= now & ~a0 & (a1 | ~a2);  // 1: a1; 3: neither a1 nor a2
    k.b1 |= now & ~a0 & ~a1;         // 2 or 3
    k.dec |= now;
}
CTF_HD int scr_action(uint32_t dec, uint32_t b0, uint32_t b1, int pc) {
    return ((dec >> pc) & 1u) ? (int)(((b1 >> pc) & 1u) * 2u + ((b0 >> pc) & 1u)) : 4;
}
CTF_HD int scr_explore(int act, uint32_t epsilon_q32, uint64_t seed, uint32_t env, uint32_t step, uint32_t agent) {
    if (!epsilon_q32) return act;
    uint32_t w[4];
    philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), env, step, agent, CTF_SCRIPT_TAG, w);
    return w[0] < epsilon_q32 ? (int)(((uint64_t)w[1] * 5u) >> 32) : act;
}
// is agent i of this env an asker of `team`, and where: row | col << 8 | carrying << 16 | 1 << 17, or 0
CTF_HD uint32_t scr_asker(const ScriptArgs& A, const uint8_t* rec, int i, uint32_t agent_mask, int team) {
    const int pr = (int8_t)rec[A.off_pos + 2 * i], pc = (int8_t)rec[A.off_pos + 2 * i + 1];
    const uint32_t fl = rec[A.off_flag + i] ? 1u : 0u;
    const bool mine = ((agent_mask >> i) & 1u) && (int)((A.team_mask >> i) & 1u) == team && pr >= 0 && pr < A.G && pc >= 0 && pc < A.G;
    return mine ? (uint32_t)pr | (uint32_t)pc << 8 | fl << 16 | 1u << 17 : 0u;
}

// One env, rows as an array: out[i] for the agents of agent_mask, every other byte of out untouched.  `env` is the env's GLOBAL
// index (env_offset + e).  An asker outside the grid (no valid state has one) stays.
static inline void scr_env_actions(const ScriptArgs& A, const uint8_t* grid, const uint8_t* rec, uint32_t agent_mask, uint32_t epsilon_q32,
                                   uint64_t seed, uint32_t step, uint32_t env, int8_t* out) {
    uint32_t open[32];
    for (int r = 0; r < 32; r++) open[r] = scr_row_open(grid, A.G, A.GS, r);
    for (int team = 0; team < 2; team++) {
        uint32_t ask[CTF_MAX_AGENTS];
        for (int i = 0; i < A.N; i++) ask[i] = scr_asker(A, rec, i, agent_mask, team);
        for (int carrying = 0; carrying < 2; carrying++) {
            uint32_t P[32] = {0}, f[32], seen[32];
            ScrPick k[32];
            bool any = false;
            for (int i = 0; i < A.N; i++)
                if ((ask[i] >> 17) && (int)((ask[i] >> 16) & 1u) == carrying) P[ask[i] & 0xFFu] |= 1u << ((ask[i] >> 8) & 0xFFu), any = true;
            if (!any) continue;
            int tr, tc;
            scr_target(A.flag_pack, team, carrying, tr, tc);
            for (int r = 0; r < 32; r++) seen[r] = f[r] = scr_goal_row(open[r], r, tr, tc), k[r] = ScrPick{0, 0, 0};
            for (int n = 0; n < A.G * A.G; n++) {
                uint32_t next[32], left = 0, alive = 0;
                for (int r = 0; r < 32; r++) {
                    const uint32_t up = r > 0 ? f[r - 1] : 0u, down = r < 31 ? f[r + 1] : 0u;
                    scr_pick(k[r], P[r], f[r], up, down);
                    left |= P[r] & ~k[r].dec;
                    next[r] = scr_step(f[r], up, down, open[r], seen[r]);
                }
                if (!left) break;
                for (int r = 0; r < 32; r++) seen[r] |= next[r], f[r] = next[r], alive |= next[r];
                if (!alive) break;
            }
            for (int i = 0; i < A.N; i++)
                if ((ask[i] >> 17) && (int)((ask[i] >> 16) & 1u) == carrying) {
                    const ScrPick& q = k[ask[i] & 0xFFu];
                    out[i] = (int8_t)scr_action(q.dec, q.b0, q.b1, (int)((ask[i] >> 8) & 0xFFu));
                }
        }
        for (int i = 0; i < A.N; i++)
            if (((agent_mask >> i) & 1u) && (int)((A.team_mask >> i) & 1u) == team) {
                const int base = (ask[i] >> 17) ? out[i] : 4;
                out[i] = (int8_t)scr_explore(base, epsilon_q32, seed, env, step, (uint32_t)i);
            }
    }
}
