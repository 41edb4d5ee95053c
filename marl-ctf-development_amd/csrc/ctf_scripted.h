// ctf_scripted.h — the scripted opponents (ctf_scripted_actions, ctf_scripted.hip; ctf_scripted_roles, ctf_scripted_roles.hip;
// ctf_scripted_abilities, ctf_scripted_abilities.hip): the policies, defined once as plain inline functions that compile for the host
// and the device.  The kernels call them with one lane per grid ROW; scr_env_actions / scr_env_roles / scr_env_abilities below walk
// the same functions over an array of rows, one env at a time (the host tests, tests/scripted/scripted_main.cpp, roles_main.cpp and
// abilities_main.cpp).  The runner first; the ROLES (runner, chaser, guard per agent) further down; the ABILITIES (a miner digs, a
// vaulter jumps) last.
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

// the searches of one field over an array of rows: askers P, goal cells f (taken over as the first frontier) -> what every row keeps
static inline void scr_rows_search(const uint32_t* open, int G, const uint32_t* P, uint32_t* f, ScrPick* k) {
    uint32_t seen[32];
    for (int r = 0; r < 32; r++) seen[r] = f[r], k[r] = ScrPick{0, 0, 0};
    for (int n = 0; n < G * G; n++) {
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
            uint32_t P[32] = {0}, f[32];
            ScrPick k[32];
            bool any = false;
            for (int i = 0; i < A.N; i++)
                if ((ask[i] >> 17) && (int)((ask[i] >> 16) & 1u) == carrying) P[ask[i] & 0xFFu] |= 1u << ((ask[i] >> 8) & 0xFFu), any = true;
            if (!any) continue;
            int tr, tc;
            scr_target(A.flag_pack, team, carrying, tr, tc);
            for (int r = 0; r < 32; r++) f[r] = scr_goal_row(open[r], r, tr, tc);
            scr_rows_search(open, A.G, P, f, k);
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

// ---- ROLES (ctf_scripted_roles, ctf_scripted_roles.hip): nibble i of role_pack is agent i's role ------------------------------------
// For agent a of team t; opp(t) = every agent of the other team inside the grid (the team bits, whatever agent_mask says), dil(S) = the
// cells inside the grid within Chebyshev distance 1 of a member of S; "search with goals Q" is the runner's search and pick with Q for
// the goal cells.  An agent that carries a flag acts as the runner does, whatever its role.
//   CTF_ROLE_RUNNER  as above
//   CTF_ROLE_CHASER  S = opp(t).  a's cell in dil(S): 4 (it tags already: tagging hits every opponent within Chebyshev distance 1,
//                    gridworld_ctf.py:796-837).  Otherwise search with goals dil(S) & open: the opponent nearest by PATH wins.
//   CTF_ROLE_GUARD   S = the carriers of opp(t); if there are none, the members of opp(t) within Chebyshev distance CTF_GUARD_ZONE of
//                    flag_pos[t] (gridworld_ctf.py:87 DEFENSIVE_ZONE_DISTANCE, :226 and :808-810 GUARDIAN_DEFENSE_DISTANCE).  S not
//                    empty: the chaser's rule on S.  S empty: within Chebyshev distance 1 of flag_pos[t] 4, else the runner's search
//                    towards flag_pos[t].
// Exploration is the runner's, applied last.  A (env, team) has up to four FIELDS, each a goal mask per row:
//   0  own-flag window    carriers and posted guards (S empty); a posted guard next to the flag is decided before the search: 4
//   1  other-flag window  runners that do not carry
//   2  dil(opp)           chasers, minus those that stand in it
//   3  dil(S)             guards when S is not empty, minus those that stand in it
// "decided before the search" = the bit is taken out of the field's asker mask: an asker no search decides stays.
#define SCR_FIELDS 4

// what a row knows of the agents after one pass over them
struct ScrRoles {
    uint32_t carry, run, chase, guard;  // the asked agents of the team in this row: carrying; not carrying, by role
    uint32_t opp, opp_carry, opp_zone;  // the opponents in this row: all; carrying; within CTF_GUARD_ZONE of the team's flag
    uint32_t any;                       // the same in every row: bit 0 some opponent carries, bit 1 some opponent is in the zone
};
// agent i of this env, whoever it plays for: row | col << 8 | carrying << 16 | 1 << 17, or 0 outside the grid
CTF_HD uint32_t scr_agent(const ScriptArgs& A, const uint8_t* rec, int i) {
    const int pr = (int8_t)rec[A.off_pos + 2 * i], pc = (int8_t)rec[A.off_pos + 2 * i + 1];
    const uint32_t fl = rec[A.off_flag + i] ? 1u : 0u;
    return (pr >= 0 && pr < A.G && pc >= 0 && pc < A.G) ? (uint32_t)pr | (uint32_t)pc << 8 | fl << 16 | 1u << 17 : 0u;
}
CTF_HD uint32_t scr_role_of(uint64_t role_pack, int i) { return (uint32_t)(role_pack >> (4 * i)) & 15u; }
// agent j (word v of scr_agent) as row r of `team` sees it
CTF_HD void scr_roles_add(ScrRoles& m, const ScriptArgs& A, uint32_t v, int j, int r, int team, uint32_t agent_mask, uint64_t role_pack) {
    const int pr = (int)(v & 0xFFu), pc = (int)((v >> 8) & 0xFFu);
    const uint32_t in = v >> 17, carrying = (v >> 16) & 1u;
    const uint32_t bit = (in && pr == r) ? 1u << (pc & 31) : 0u;
    const bool theirs = (int)((A.team_mask >> j) & 1u) != team;
    const bool asked = !theirs && ((agent_mask >> j) & 1u);
    const int fr = (int)((A.flag_pack >> (16 * team)) & 0xFFu), fc = (int)((A.flag_pack >> (16 * team + 8)) & 0xFFu);
    const int dr = pr > fr ? pr - fr : fr - pr, dc = pc > fc ? pc - fc : fc - pc;
    const uint32_t zone = (in && dr <= CTF_GUARD_ZONE && dc <= CTF_GUARD_ZONE) ? 1u : 0u;
    const uint32_t role = scr_role_of(role_pack, j);
    const uint32_t obit = theirs ? bit : 0u, abit = asked ? bit : 0u, free_ = carrying ? 0u : abit;
    m.opp |= obit;
    m.opp_carry |= carrying ? obit : 0u;
    m.opp_zone |= zone ? obit : 0u;
    m.any |= theirs ? ((in & carrying) | zone << 1) : 0u;
    m.carry |= carrying ? abit : 0u;
    m.run |= role == CTF_ROLE_RUNNER ? free_ : 0u;
    m.chase |= role == CTF_ROLE_CHASER ? free_ : 0u;
    m.guard |= role == CTF_ROLE_GUARD ? free_ : 0u;
}
// the guards' set S, as a row mask
CTF_HD uint32_t scr_guard_set(const ScrRoles& m) { return (m.any & 1u) ? m.opp_carry : m.opp_zone; }
// row r of dil(S) from rows r - 1, r, r + 1 of S (0 outside the grid): h(up) | h(mid) | h(down), h(x) = x | x << 1 | x >> 1
CTF_HD uint32_t scr_dil(uint32_t up, uint32_t mid, uint32_t down, int G, int r) {
    const uint32_t x = up | mid | down;
    return r < G ? (x | (x << 1) | (x >> 1)) & (G >= 32 ? 0xFFFFFFFFu : (1u << G) - 1u) : 0u;
}
// the askers P and goal cells `goal` of row r, per field
CTF_HD void scr_role_fields(const ScrRoles& m, uint32_t open, int r, uint32_t flag_pack, int team, uint32_t dil_opp, uint32_t dil_set, uint32_t* P,
                            uint32_t* goal) {
    int fr, fc, tr, tc;
    scr_target(flag_pack, team, 1, fr, fc);
    scr_target(flag_pack, team, 0, tr, tc);
    const uint32_t window = (r >= fr - 1 && r <= fr + 1) ? (uint32_t)((7ull << fc) >> 1) : 0u;  // next to the own flag (or on it)
    const bool posted = (m.any & 3u) == 0u;                                                      // S is empty
    P[0] = m.carry | (posted ? m.guard & ~window : 0u);
    P[1] = m.run;
    P[2] = m.chase & ~dil_opp;
    P[3] = posted ? 0u : m.guard & ~dil_set;
    goal[0] = scr_goal_row(open, r, fr, fc);
    goal[1] = scr_goal_row(open, r, tr, tc);
    goal[2] = dil_opp & open;
    goal[3] = dil_set & open;
}
// the field agent (word v, role) asks
CTF_HD int scr_role_field(uint32_t v, uint32_t role, uint32_t any) {
    if ((v >> 16) & 1u) return 0;
    return role == CTF_ROLE_RUNNER ? 1 : role == CTF_ROLE_CHASER ? 2 : (any & 3u) ? 3 : 0;
}

// scr_env_actions with roles
static inline void scr_env_roles(const ScriptArgs& A, const uint8_t* grid, const uint8_t* rec, uint32_t agent_mask, uint64_t role_pack,
                                 uint32_t epsilon_q32, uint64_t seed, uint32_t step, uint32_t env, int8_t* out) {
    uint32_t open[32], word[CTF_MAX_AGENTS];
    for (int r = 0; r < 32; r++) open[r] = scr_row_open(grid, A.G, A.GS, r);
    for (int i = 0; i < A.N; i++) word[i] = scr_agent(A, rec, i);
    for (int team = 0; team < 2; team++) {
        if (!((script_teams(A, agent_mask) >> team) & 1u)) continue;
        ScrRoles m[32];
        uint32_t P[SCR_FIELDS][32], goal[SCR_FIELDS][32];
        for (int r = 0; r < 32; r++) {
            m[r] = ScrRoles{0, 0, 0, 0, 0, 0, 0, 0};
            for (int j = 0; j < A.N; j++) scr_roles_add(m[r], A, word[j], j, r, team, agent_mask, role_pack);
        }
        for (int r = 0; r < 32; r++) {
            const uint32_t o_up = r > 0 ? m[r - 1].opp : 0u, o_down = r < 31 ? m[r + 1].opp : 0u;
            const uint32_t s_up = r > 0 ? scr_guard_set(m[r - 1]) : 0u, s_down = r < 31 ? scr_guard_set(m[r + 1]) : 0u;
            uint32_t p[SCR_FIELDS], g[SCR_FIELDS];
            scr_role_fields(m[r], open[r], r, A.flag_pack, team, scr_dil(o_up, m[r].opp, o_down, A.G, r),
                            scr_dil(s_up, scr_guard_set(m[r]), s_down, A.G, r), p, g);
            for (int f = 0; f < SCR_FIELDS; f++) P[f][r] = p[f], goal[f][r] = g[f];
        }
        for (int i = 0; i < A.N; i++)
            if (((agent_mask >> i) & 1u) && (int)((A.team_mask >> i) & 1u) == team) out[i] = 4;
        for (int f = 0; f < SCR_FIELDS; f++) {
            uint32_t any = 0;
            for (int r = 0; r < 32; r++) any |= P[f][r];
            if (!any) continue;
            ScrPick k[32];
            scr_rows_search(open, A.G, P[f], goal[f], k);
            for (int i = 0; i < A.N; i++)
                if (((agent_mask >> i) & 1u) && (int)((A.team_mask >> i) & 1u) == team && (word[i] >> 17) &&
                    scr_role_field(word[i], scr_role_of(role_pack, i), m[0].any) == f) {
                    const ScrPick& q = k[word[i] & 0xFFu];
                    out[i] = (int8_t)scr_action(q.dec, q.b0, q.b1, (int)((word[i] >> 8) & 0xFFu));
                }
        }
        for (int i = 0; i < A.N; i++)
            if (((agent_mask >> i) & 1u) && (int)((A.team_mask >> i) & 1u) == team)
                out[i] = (int8_t)scr_explore(out[i], epsilon_q32, seed, env, step, (uint32_t)i);
    }
}

// ---- ABILITIES (ctf_scripted_abilities, ctf_scripted_abilities.hip): bit i of ability_mask = agent i moves with its type's ability ----
// Roles, goal sets Q, who is decided before the search and the exploration are those of the ROLES above.  What changes is how an agent
// moves towards Q, by its CLASS, decided from the state the call reads:
//   SCR_DIGGER   ability bit and type 3 (miner).  Passable: OPEN, DESTRUCTIBLE_TILE1 (2), DESTRUCTIBLE_TILE2 (3); blocks, flags and
//                agents are walls.  Entering a cell costs w = 1 (OPEN), 2 (tile 3: one hit, then the move), 3 (tile 2: two hits, then
//                the move): mine_block and movement_handler (gridworld_ctf.py:669-690, :577-580).  Goals Q & passable.  D(c) = the
//                least sum of entry costs over 4-neighbour paths from c into a goal cell (the goal's own cost counted, c's not; D of
//                a goal is 0).  Action: the lowest-numbered of 0..3 whose neighbour n is inside the grid, passable and has the minimum
//                finite w(n) + D(n); none: 4.  Moving into a destructible tile IS the mining action.
//   SCR_VAULTER  ability bit, type 2 and (hp - vault_hp_cost) > vault_min_hp in f64, as the step tests it (gridworld_ctf.py:649-650).
//                Passable: OPEN.  Moves: the four unit moves and the jumps 5..8, deltas (-2,0), (2,0), (0,2), (0,-2); a jump needs its
//                landing cell inside the grid and OPEN, the cell jumped over may hold anything (:123-133, :643-650).  Every move
//                costs 1; later jumps are taken to be affordable (the agent plans again every step).  Action: the lowest-numbered of
//                0, 1, 2, 3, 5, 6, 7, 8 whose landing cell has the minimum finite D (a walk wins a tie with a jump); none: 4.
//   SCR_WALKER   everyone else: scr_env_roles' result, bit for bit, whatever the ability bit says.
// A FIELD is now (goal kind of SCR_FIELDS, class).
//
// BIT-PARALLEL FORM.  One search serves the three classes.  A passable cell x with D(x) settled EMITS in iteration D(x) + w(x): that
// is the cost, from any neighbour, of the path that enters x first, so
//   settled = (the neighbours of the emitting frontier E) & passable & ~seen          D of these cells is this iteration's number
//   E' = p1 | settled & w1,  p1' = p2 | settled & w2,  p2' = settled & w3             two pending masks per row: emit in 2, in 3
// and an asker takes the first iteration in which a neighbour of its cell emits (scr_pick's rule on E).  The goals are settled at 0:
// E = goal & w1, p1 = goal & w2, p2 = goal & w3.  With w2 = w3 = 0 this is the runner's loop, iteration for iteration.  The vaulter's
// neighbours are the eight cells at distance 1 and 2 along a row or a column (a jump and its reverse need the same thing: the cell
// landed on is OPEN), and its pick keeps a third bit: 1 = a jump.  An iteration can pass with nothing emitting, so the loop ends on
// "every asker decided" or "nothing emits and nothing is pending", at most 3 G G + 2 iterations.
#define SCR_WALKER 0u
#define SCR_DIGGER 1u
#define SCR_VAULTER 2u
#define SCR_CLASSES 3
#define SCR_ITER_BOUND (3 * CTF_MAX_CELLS + 8)  // not reached: every cell emits once, at most 3 iterations after it settled

struct ScriptAbil {
    uint32_t type_pack;            // 2 bits per agent
    int32_t off_hp;                // f64 hp[N] in the record
    double vault_cost, vault_min;  // VAULT_HP_COST, VAULT_MIN_HP
};
static inline ScriptAbil script_abil(const DevCfg& d) { return ScriptAbil{d.type_pack, 0, d.vault_cost, d.vault_min}; }
// does any asked agent move by an ability, judged by TYPE alone (what a launcher can know)
static inline bool script_any_ability(const ScriptArgs& A, const ScriptAbil& B, uint32_t agent_mask, uint32_t ability_mask) {
    for (int i = 0; i < A.N; i++)
        if ((((agent_mask & ability_mask) >> i) & 1u) && ((B.type_pack >> (2 * i)) & 3u) >= 2u) return true;
    return false;
}
// the class of agent i (record rec, 8-byte aligned)
CTF_HD uint32_t scr_class(const ScriptAbil& B, const uint8_t* rec, int i, uint32_t ability_mask) {
    const uint32_t type = (B.type_pack >> (2 * i)) & 3u;
    const double hp = *(const double*)(rec + B.off_hp + 8 * i);
    if (!((ability_mask >> i) & 1u)) return SCR_WALKER;
    if (type == 3u) return SCR_DIGGER;
    return (type == 2u && (hp - B.vault_cost) > B.vault_min) ? SCR_VAULTER : SCR_WALKER;
}
// scr_row_open with the rows of DESTRUCTIBLE_TILE1 (t2) and DESTRUCTIBLE_TILE2 (t3) from the same nine dwords
CTF_HD void scr_row_tiles(const uint8_t* grid, int G, int GS, int r, uint32_t& open, uint32_t& t2, uint32_t& t3) {
    const int rr = r < G ? r : G - 1;
    const int b0 = rr * G, w0 = b0 >> 2, last = (GS >> 2) - 1;
    const uint32_t* words = (const uint32_t*)grid;
    uint32_t v[9];
#pragma unroll
    for (int j = 0; j < 9; j++) v[j] = words[(size_t)(w0 + j < last ? w0 + j : last)];  // all in flight together
    uint64_t a0 = 0, a2 = 0, a3 = 0;
#pragma unroll
    for (int j = 0; j < 9; j++) {
        a0 |= (uint64_t)scr_zero_bytes(v[j]) << (4 * j);
        a2 |= (uint64_t)scr_zero_bytes(v[j] ^ 0x02020202u) << (4 * j);
        a3 |= (uint64_t)scr_zero_bytes(v[j] ^ 0x03030303u) << (4 * j);
    }
    const uint32_t cols = r < G ? (G >= 32 ? 0xFFFFFFFFu : (1u << G) - 1u) : 0u;
    open = (uint32_t)(a0 >> (b0 & 3)) & cols;
    t2 = (uint32_t)(a2 >> (b0 & 3)) & cols;
    t3 = (uint32_t)(a3 >> (b0 & 3)) & cols;
}
// the cells of a row by entry cost, for a class: w[0] | w[1] | w[2] is what the class may enter
CTF_HD void scr_class_cost(uint32_t cls, uint32_t open, uint32_t t2, uint32_t t3, uint32_t* w) {
    w[0] = open;
    w[1] = cls == SCR_DIGGER ? t3 : 0u;
    w[2] = cls == SCR_DIGGER ? t2 : 0u;
}

// a row's search state: the emitting frontier, the two pending masks, what has been settled
struct ScrFront {
    uint32_t e, p1, p2, seen;
};
// the goals Q of a field, cut to what the class may enter, settled at 0
CTF_HD ScrFront scr_front(uint32_t Q, const uint32_t* w) { return ScrFront{Q & w[0], Q & w[1], Q & w[2], Q & (w[0] | w[1] | w[2])}; }
// one iteration of a row: near = E of rows r - 1 | r + 1, far = E of rows r - 2 | r + 2 (0 unless the class jumps)
CTF_HD void scr_advance(ScrFront& s, uint32_t near, uint32_t far, bool jumps, const uint32_t* w) {
    const uint32_t side = (s.e << 1) | (s.e >> 1) | (jumps ? (s.e << 2) | (s.e >> 2) : 0u);
    const uint32_t settled = (side | near | far) & (w[0] | w[1] | w[2]) & ~s.seen;
    s.seen |= settled;
    s.e = s.p1 | (settled & w[0]);
    s.p1 = s.p2 | (settled & w[1]);
    s.p2 = settled & w[2];
}
// scr_pick with the four jumps behind the four walks: b2 = the action is a jump, (b1, b0) = which of the four
struct ScrPick8 {
    uint32_t dec, b0, b1, b2;
};
CTF_HD void scr_pick8(ScrPick8& k, uint32_t P, uint32_t e, uint32_t up, uint32_t down, uint32_t up2, uint32_t down2, bool jumps) {
    const uint32_t a0 = up, a1 = down, a2 = e >> 1, a3 = e << 1;
    const uint32_t j0 = jumps ? up2 : 0u, j1 = jumps ? down2 : 0u, j2 = jumps ? e >> 2 : 0u, j3 = jumps ? e << 2 : 0u;
    const uint32_t walk = a0 | a1 | a2 | a3, undecided = P & ~k.dec;
    const uint32_t now_w = walk & undecided, now_j = (j0 | j1 | j2 | j3) & undecided & ~walk;
    k.b0 |= (now_w & ~a0 & (a1 | ~a2)) | (now_j & ~j0 & (j1 | ~j2));
    k.b1 |= (now_w & ~a0 & ~a1) | (now_j & ~j0 & ~j1);
    k.b2 |= now_j;
    k.dec |= now_w | now_j;
}
CTF_HD int scr_action8(uint32_t dec, uint32_t b0, uint32_t b1, uint32_t b2, int pc) {
    return ((dec >> pc) & 1u) ? (int)(((b2 >> pc) & 1u) * 5u + ((b1 >> pc) & 1u) * 2u + ((b0 >> pc) & 1u)) : 4;
}
// the class agent j (word v of scr_agent, class in bits 18..19) shows row r: its cell's bit in dig / vault
CTF_HD void scr_class_add(uint32_t& dig, uint32_t& vault, uint32_t v, int r) {
    const uint32_t bit = ((v >> 17) & 1u) && (int)(v & 0xFFu) == r ? 1u << ((v >> 8) & 31u) : 0u, cls = (v >> 18) & 3u;
    dig |= cls == SCR_DIGGER ? bit : 0u;
    vault |= cls == SCR_VAULTER ? bit : 0u;
}
// the askers of a class among the askers P of a goal kind
CTF_HD uint32_t scr_class_askers(uint32_t P, uint32_t cls, uint32_t dig, uint32_t vault) {
    return P & (cls == SCR_DIGGER ? dig : cls == SCR_VAULTER ? vault : ~(dig | vault));
}

// the search of one field over an array of rows: askers P, goal cells Q (not yet cut to what the class may enter)
static inline void scr_rows_search8(const uint32_t* open, const uint32_t* t2, const uint32_t* t3, uint32_t cls, const uint32_t* P, const uint32_t* Q,
                                    ScrPick8* k) {
    ScrFront s[32];
    uint32_t w[32][3];
    const bool jumps = cls == SCR_VAULTER;
    for (int r = 0; r < 32; r++) {
        scr_class_cost(cls, open[r], t2[r], t3[r], w[r]);
        s[r] = scr_front(Q[r], w[r]);
        k[r] = ScrPick8{0, 0, 0, 0};
    }
    for (int n = 0; n < SCR_ITER_BOUND; n++) {
        uint32_t e[32], left = 0, alive = 0;
        for (int r = 0; r < 32; r++) e[r] = s[r].e;
        for (int r = 0; r < 32; r++) {
            const uint32_t up = r > 0 ? e[r - 1] : 0u, down = r < 31 ? e[r + 1] : 0u;
            const uint32_t up2 = (jumps && r > 1) ? e[r - 2] : 0u, down2 = (jumps && r < 30) ? e[r + 2] : 0u;
            scr_pick8(k[r], P[r], e[r], up, down, up2, down2, jumps);
            left |= P[r] & ~k[r].dec;
            scr_advance(s[r], up | down, up2 | down2, jumps, w[r]);
            alive |= s[r].e | s[r].p1 | s[r].p2;
        }
        if (!left || !alive) break;
    }
}

// scr_env_roles with abilities
static inline void scr_env_abilities(const ScriptArgs& A, const ScriptAbil& B, const uint8_t* grid, const uint8_t* rec, uint32_t agent_mask,
                                     uint64_t role_pack, uint32_t ability_mask, uint32_t epsilon_q32, uint64_t seed, uint32_t step, uint32_t env,
                                     int8_t* out) {
    uint32_t open[32], t2[32], t3[32], word[CTF_MAX_AGENTS];
    for (int r = 0; r < 32; r++) scr_row_tiles(grid, A.G, A.GS, r, open[r], t2[r], t3[r]);
    for (int i = 0; i < A.N; i++) {
        word[i] = scr_agent(A, rec, i);
        if (word[i]) word[i] |= scr_class(B, rec, i, ability_mask) << 18;
    }
    for (int team = 0; team < 2; team++) {
        if (!((script_teams(A, agent_mask) >> team) & 1u)) continue;
        ScrRoles m[32];
        uint32_t P[SCR_FIELDS][32], Q[SCR_FIELDS][32], dig[32], vault[32];
        for (int r = 0; r < 32; r++) {
            m[r] = ScrRoles{0, 0, 0, 0, 0, 0, 0, 0};
            dig[r] = vault[r] = 0;
            for (int j = 0; j < A.N; j++) {
                scr_roles_add(m[r], A, word[j] & 0x3FFFFu, j, r, team, agent_mask, role_pack);
                scr_class_add(dig[r], vault[r], word[j], r);
            }
        }
        for (int r = 0; r < 32; r++) {
            const uint32_t o_up = r > 0 ? m[r - 1].opp : 0u, o_down = r < 31 ? m[r + 1].opp : 0u;
            const uint32_t s_up = r > 0 ? scr_guard_set(m[r - 1]) : 0u, s_down = r < 31 ? scr_guard_set(m[r + 1]) : 0u;
            uint32_t p[SCR_FIELDS], q[SCR_FIELDS];
            scr_role_fields(m[r], 0xFFFFFFFFu, r, A.flag_pack, team, scr_dil(o_up, m[r].opp, o_down, A.G, r),
                            scr_dil(s_up, scr_guard_set(m[r]), s_down, A.G, r), p, q);  // q: the goal sets before any tile is asked for
            for (int f = 0; f < SCR_FIELDS; f++) P[f][r] = p[f], Q[f][r] = q[f];
        }
        for (int i = 0; i < A.N; i++)
            if (((agent_mask >> i) & 1u) && (int)((A.team_mask >> i) & 1u) == team) out[i] = 4;
        for (int f = 0; f < SCR_FIELDS; f++)
            for (uint32_t cls = 0; cls < SCR_CLASSES; cls++) {
                uint32_t Pc[32], any = 0;
                for (int r = 0; r < 32; r++) any |= Pc[r] = scr_class_askers(P[f][r], cls, dig[r], vault[r]);
                if (!any) continue;
                ScrPick8 k[32];
                scr_rows_search8(open, t2, t3, cls, Pc, Q[f], k);
                for (int i = 0; i < A.N; i++)
                    if (((agent_mask >> i) & 1u) && (int)((A.team_mask >> i) & 1u) == team && (word[i] >> 17) && ((word[i] >> 18) & 3u) == cls &&
                        scr_role_field(word[i], scr_role_of(role_pack, i), m[0].any) == f) {
                        const ScrPick8& q = k[word[i] & 0xFFu];
                        out[i] = (int8_t)scr_action8(q.dec, q.b0, q.b1, q.b2, (int)((word[i] >> 8) & 0xFFu));
                    }
            }
        for (int i = 0; i < A.N; i++)
            if (((agent_mask >> i) & 1u) && (int)((A.team_mask >> i) & 1u) == team)
                out[i] = (int8_t)scr_explore(out[i], epsilon_q32, seed, env, step, (uint32_t)i);
    }
}

// ---- COSTS (ctf_scripted_costs, ctf_scripted_costs.hip): how far every asked agent is from its goal, under the rules it plans with ----
// Roles, classes and goal sets Q are those of the ABILITIES above (scr_class, scr_role_field, scr_role_fields with open = all ones).
// cost(a), an int16, is THE COST OF REACHING Q, not "the planner's next move + 1":
//   0              a is decided before the search (a chaser standing in dil(S), a posted guard next to its flag), or a's own cell lies
//                  in Q.  An agent's cell holds its tile and is never passable, so the test is on the uncut Q; such bits are taken out
//                  of the field's askers as the "decided before the search" bits are.  (The action kernels still MOVE an agent that
//                  stands in Q — a runner next to the flag steps to another open cell of the window — so cost 0 does not mean action 4.)
//   n + 1          otherwise: n the 0-based iteration of the search loop in which scr_pick8 decides the asker.  A goal cell of entry
//                  cost 1 emits in iteration 0, a cell x in iteration D(x) + w(x) - 1, so this is, for the
//                    WALKER   1 + d(n), the minimum over the four neighbours n, d the BFS distance over OPEN cells,
//                    DIGGER   w(n) + D(n), the minimum over the four neighbours, entry costs w = 1 / 2 / 3,
//                    VAULTER  1 + d(n), the minimum over the eight landing cells:
//                  the least total entry cost over move sequences of a's class from a's cell into a cell of Q the class may enter.
//   CTF_COST_NONE  no such sequence exists, or a stands outside the grid (no valid state has one).
// Finite costs are at most 3 G G < 2^15.  No exploration and no seed: the cost is a function of the state.  (CTF_COST_NONE: ctf_env.h)

// the askers of a field for the costs: those of the action rule that do not stand in the (uncut) goal set
CTF_HD uint32_t scr_cost_askers(uint32_t P, uint32_t Q) { return P & ~Q; }
// what an iteration adds to a row's decided mask -> the cost its askers latch: n + 1
CTF_HD int scr_cost_of_iteration(int n) { return n + 1; }

// scr_rows_search8 that keeps WHEN instead of which way: cost[r * 32 + c] = n + 1 for the asker at (r, c) decided in iteration n,
// CTF_COST_NONE for an asker no iteration decides; the entries of cells without an asker are not written
static inline void scr_rows_costs8(const uint32_t* open, const uint32_t* t2, const uint32_t* t3, uint32_t cls, const uint32_t* P, const uint32_t* Q,
                                   int16_t* cost /* [32][32] */) {
    ScrFront s[32];
    ScrPick8 k[32];
    uint32_t w[32][3];
    const bool jumps = cls == SCR_VAULTER;
    for (int r = 0; r < 32; r++) {
        scr_class_cost(cls, open[r], t2[r], t3[r], w[r]);
        s[r] = scr_front(Q[r], w[r]);
        k[r] = ScrPick8{0, 0, 0, 0};
        for (int c = 0; c < 32; c++)
            if ((P[r] >> c) & 1u) cost[r * 32 + c] = CTF_COST_NONE;
    }
    for (int n = 0; n < SCR_ITER_BOUND; n++) {
        uint32_t e[32], left = 0, alive = 0;
        for (int r = 0; r < 32; r++) e[r] = s[r].e;
        for (int r = 0; r < 32; r++) {
            const uint32_t up = r > 0 ? e[r - 1] : 0u, down = r < 31 ? e[r + 1] : 0u;
            const uint32_t up2 = (jumps && r > 1) ? e[r - 2] : 0u, down2 = (jumps && r < 30) ? e[r + 2] : 0u;
            const uint32_t before = k[r].dec;
            scr_pick8(k[r], P[r], e[r], up, down, up2, down2, jumps);
            const uint32_t now = k[r].dec & ~before;
            for (int c = 0; c < 32; c++)
                if ((now >> c) & 1u) cost[r * 32 + c] = (int16_t)scr_cost_of_iteration(n);
            left |= P[r] & ~k[r].dec;
            scr_advance(s[r], up | down, up2 | down2, jumps, w[r]);
            alive |= s[r].e | s[r].p1 | s[r].p2;
        }
        if (!left || !alive) break;
    }
}

// One env, rows as an array: out[i] = cost(i) for the agents of agent_mask, every other entry of out untouched
static inline void scr_env_costs(const ScriptArgs& A, const ScriptAbil& B, const uint8_t* grid, const uint8_t* rec, uint32_t agent_mask, uint64_t role_pack,
                                 uint32_t ability_mask, int16_t* out) {
    uint32_t open[32], t2[32], t3[32], word[CTF_MAX_AGENTS];
    for (int r = 0; r < 32; r++) scr_row_tiles(grid, A.G, A.GS, r, open[r], t2[r], t3[r]);
    for (int i = 0; i < A.N; i++) {
        word[i] = scr_agent(A, rec, i);
        if (word[i]) word[i] |= scr_class(B, rec, i, ability_mask) << 18;
    }
    int16_t cost[32 * 32];
    for (int team = 0; team < 2; team++) {
        if (!((script_teams(A, agent_mask) >> team) & 1u)) continue;
        ScrRoles m[32];
        uint32_t P[SCR_FIELDS][32], Q[SCR_FIELDS][32], dig[32], vault[32];
        for (int r = 0; r < 32; r++) {
            m[r] = ScrRoles{0, 0, 0, 0, 0, 0, 0, 0};
            dig[r] = vault[r] = 0;
            for (int j = 0; j < A.N; j++) {
                scr_roles_add(m[r], A, word[j] & 0x3FFFFu, j, r, team, agent_mask, role_pack);
                scr_class_add(dig[r], vault[r], word[j], r);
            }
        }
        for (int r = 0; r < 32; r++) {
            const uint32_t o_up = r > 0 ? m[r - 1].opp : 0u, o_down = r < 31 ? m[r + 1].opp : 0u;
            const uint32_t s_up = r > 0 ? scr_guard_set(m[r - 1]) : 0u, s_down = r < 31 ? scr_guard_set(m[r + 1]) : 0u;
            uint32_t p[SCR_FIELDS], q[SCR_FIELDS];
            scr_role_fields(m[r], 0xFFFFFFFFu, r, A.flag_pack, team, scr_dil(o_up, m[r].opp, o_down, A.G, r),
                            scr_dil(s_up, scr_guard_set(m[r]), s_down, A.G, r), p, q);  // q: the goal sets before any tile is asked for
            for (int f = 0; f < SCR_FIELDS; f++) P[f][r] = scr_cost_askers(p[f], q[f]), Q[f][r] = q[f];
        }
        // asked and inside the grid: 0 unless a search below says otherwise; outside the grid: no cost
        for (int i = 0; i < A.N; i++)
            if (((agent_mask >> i) & 1u) && (int)((A.team_mask >> i) & 1u) == team) out[i] = (int16_t)((word[i] >> 17) ? 0 : CTF_COST_NONE);
        for (int f = 0; f < SCR_FIELDS; f++)
            for (uint32_t cls = 0; cls < SCR_CLASSES; cls++) {
                uint32_t Pc[32], any = 0;
                for (int r = 0; r < 32; r++) any |= Pc[r] = scr_class_askers(P[f][r], cls, dig[r], vault[r]);
                if (!any) continue;
                scr_rows_costs8(open, t2, t3, cls, Pc, Q[f], cost);
                for (int i = 0; i < A.N; i++)
                    if (((agent_mask >> i) & 1u) && (int)((A.team_mask >> i) & 1u) == team && (word[i] >> 17) && ((word[i] >> 18) & 3u) == cls &&
                        scr_role_field(word[i], scr_role_of(role_pack, i), m[0].any) == f) {
                        const int pr = (int)(word[i] & 0xFFu), pc = (int)((word[i] >> 8) & 0xFFu);
                        if ((Pc[pr] >> pc) & 1u) out[i] = cost[pr * 32 + pc];
                    }
            }
    }
}
