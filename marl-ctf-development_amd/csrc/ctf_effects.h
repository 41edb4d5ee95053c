// ctf_effects.h — WHAT EACH ACTION WOULD DO (ctf_action_effects, ctf_random_effective_actions; kernels in ctf_effects.hip): the `act`
// part of the step (ctf_step_core.h env_step, "---- act"; gridworld_ctf.py:700-732) stated once as a pure function of the state, as
// plain inline functions that compile for the host and the device.  The kernels call them with one lane per (env, agent);
// eff_env_effects / eff_env_sample below walk the same functions over the agents of one env (the host test,
// tests/effects/effects_main.cpp).
//
// effect(i, a), a byte of CTF_EFF_* flags (include/ctf_env.h), says what act(i, a) would do IF AGENT i ACTED NOW, BEFORE ANYONE ELSE
// MOVES, from the state as it stands (grid, position, hp, has_flag, inventory) and the config:
//   target   the agent's cell + the action's delta: 0..3 (-1,0), (1,0), (0,1), (0,-1); 5..8 the same four, twice as far for a vaulter
//            (type 2), as far for a miner (type 3) and nowhere for types 0 and 1 (ACTION_DELTAS, :100-145); 4 nowhere
//   MOVES    target inside the grid and OPEN (0), and the action is 0..3 or a vault (movement_handler, :577-580)
//   JUMPS    a vault: actions 5..8, type 2, target OPEN and (hp - VAULT_HP_COST) > VAULT_MIN_HP in f64, the step's own expression
//            (:643-657); the hp falls by the cost.  The cell jumped over may hold anything
//   PICKS_UP the move ends within Chebyshev distance 1 of the other team's flag cell and that cell holds the flag tile (:583-591)
//   CAPTURES the move ends within Chebyshev distance 1 of the own flag cell, the agent carries a flag (or has just picked it up:
//            a pickup and a capture in one move set both flags) and, under HOME_FLAG_CAPTURE, the own flag cell holds the own flag
//            tile (:594-610)
//   MINES    a miner, actions 0..3, target DESTRUCTIBLE_TILE1 (2, becomes 3) or DESTRUCTIBLE_TILE2 (3, becomes OPEN) (:669-690)
//   BREAKS   that target was 3: the hit opens the cell, and the inventory rises by one unless it is at its cap
//   LAYS     a miner, actions 5..8, inventory > 0, target OPEN and further than Chebyshev distance 1 from BOTH spawn cells (:659-667)
// JUMPS, PICKS_UP and CAPTURES imply MOVES, BREAKS implies MINES; MOVES, MINES and LAYS exclude one another; bit 7 is never set.
// effect == 0: the action leaves grid, positions, hp, flags, inventory and counters untouched — action 4, actions 5..8 of types 0 and
// 1, a target outside the grid, a target that is neither open nor minable, a refused vault or lay.  An agent whose position is
// outside the grid (no valid state has one) has every effect 0.  Tagging, healing and the shuffle are not part of `act` and not
// part of the effect.
//
// THE CAVEAT every multi-agent action mask carries: inside a real step the agents act one after the other in a shuffled order, so
// ANOTHER AGENT MAY MOVE FIRST — into the cell this agent wanted, away from it, onto the flag — or tag this agent out, and what the
// action then does differs from what is promised here.  The promise is exact for the agent the step happens to move first, and for
// every agent when the others stay.
//
// mask(i): bit a = (effect(i, a) != 0); bit 4 and bits 9..15 are never set.
// sample(i): S = mask(i).  S empty: 4, no draw.  Otherwise w = Philox4x32-10(key = seed, counter = (global env, step, i, "EFF1")),
// k = mulhi(w[0], popcount(S)), and the action is the index of the (k + 1)-th lowest set bit of S: uniform over the effective actions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ctf_device.h"

#define CTF_EFFECT_TAG 0x45464631u  // "EFF1": word 3 of the sampler's counter

struct EffectArgs {
    const uint8_t* grid;  // u8 [E][GS]
    const uint8_t* rec;   // u8 [E][RS]: f64 hp[N] at off_hp, i8 pos[N][2] at off_pos, u8 has_flag[N] at off_flag, i16 inv[N] at off_inv
    int32_t n_envs, N, G, GS, RS, off_hp, off_pos, off_flag, off_inv;
    int32_t home_flag_capture;
    uint32_t team_mask;              // bit i = team(i)
    uint32_t type_pack;              // 2 bits per agent
    uint32_t flag_pack, spawn_pack;  // the two teams' cells: row 0 | col 0 << 8 | row 1 << 16 | col 1 << 24
    double vault_cost, vault_min;    // VAULT_HP_COST, VAULT_MIN_HP
    FastDiv div_n;                   // / N over 0 .. 256 (the kernels' lane -> (env of the block, agent))
};

static inline EffectArgs effect_args(const DevCfg& d, const DevPtrs& p) {
    return EffectArgs{p.grid,      p.rec,       d.n_envs,    d.N,         d.G,          d.GS,         d.RS, 0, d.off_pos, d.off_flag, d.off_inv, d.home_flag_capture,
                      d.team_mask, d.type_pack, d.flag_pack, d.spawn_pack, d.vault_cost, d.vault_min, d.div_n};
}

CTF_HD int eff_abs(int x) { return x < 0 ? -x : x; }
CTF_HD int eff_cheb(int r0, int c0, int r1, int c1) {
    const int a = eff_abs(r0 - r1), b = eff_abs(c0 - c1);
    return a > b ? a : b;
}
CTF_HD int eff_pack_row(uint32_t pack, int team) { return (int)((pack >> (16 * team)) & 0xFFu); }
CTF_HD int eff_pack_col(uint32_t pack, int team) { return (int)((pack >> (16 * team + 8)) & 0xFFu); }
// the tile at (r, c), or -1 outside the grid: the load is unconditional, on a clamped index
CTF_HD int eff_tile(const uint8_t* grid, int G, int r, int c) {
    const bool inside = (uint32_t)r < (uint32_t)G && (uint32_t)c < (uint32_t)G;
    const int rr = r < 0 ? 0 : (r < G ? r : G - 1), cc = c < 0 ? 0 : (c < G ? c : G - 1);
    const int v = grid[(size_t)(rr * G + cc)];
    return inside ? v : -1;
}

// what the rule needs of agent i, read once for its nine actions
struct EffAgent {
    int pr, pc, type, team, inv;
    bool inside, carrying, vault_hp;  // vault_hp: (hp - VAULT_HP_COST) > VAULT_MIN_HP
    int opp_flag_tile, home_flag_tile;  // the tiles on the two flag cells
};
CTF_HD EffAgent eff_agent(const EffectArgs& A, const uint8_t* grid, const uint8_t* rec, int i) {
    EffAgent s;
    s.pr = (int8_t)rec[A.off_pos + 2 * i];
    s.pc = (int8_t)rec[A.off_pos + 2 * i + 1];
    s.type = (int)((A.type_pack >> (2 * i)) & 3u);
    s.team = (int)((A.team_mask >> i) & 1u);
    s.inv = *(const int16_t*)(rec + A.off_inv + 2 * i);
    s.inside = (uint32_t)s.pr < (uint32_t)A.G && (uint32_t)s.pc < (uint32_t)A.G;
    s.carrying = (rec[A.off_flag + i] & 1u) != 0;
    const double hp = *(const double*)(rec + A.off_hp + 8 * i);
    s.vault_hp = (hp - A.vault_cost) > A.vault_min;
    s.opp_flag_tile = eff_tile(grid, A.G, eff_pack_row(A.flag_pack, 1 - s.team), eff_pack_col(A.flag_pack, 1 - s.team));
    s.home_flag_tile = eff_tile(grid, A.G, eff_pack_row(A.flag_pack, s.team), eff_pack_col(A.flag_pack, s.team));
    return s;
}

// the cell action a of an agent of `type` at (pr, pc) aims at; scale 0: the action has no target (4; 5..8 of types 0 and 1)
CTF_HD int eff_target(int type, int pr, int pc, int a, int& nr, int& nc) {
    const int base = a <= 4 ? a : a - 5;
    const int scale = a == 4 ? 0 : (a < 4 ? 1 : (type == 2 ? 2 : (type == 3 ? 1 : 0)));
    nr = pr + (base == 0 ? -1 : (base == 1 ? 1 : 0)) * scale;
    nc = pc + (base == 2 ? 1 : (base == 3 ? -1 : 0)) * scale;
    return scale;
}
// effect(i, a) for the agent s describes; a in 0..8, cell = the tile at a's target (eff_tile)
CTF_HD uint32_t eff_action(const EffectArgs& A, const EffAgent& s, int a, int cell) {
    int nr, nc;
    const int scale = eff_target(s.type, s.pr, s.pc, a, nr, nc);
    if (!s.inside || a == 4 || scale == 0 || cell < 0) return 0u;
    const bool vault = a >= 5 && s.type == 2 && cell == 0 && s.vault_hp;
    if (cell == 0 && (a <= 3 || vault)) {
        const int team = s.team;
        uint32_t f = CTF_EFF_MOVES | (vault ? CTF_EFF_JUMPS : 0u);
        const bool pickup = eff_cheb(nr, nc, eff_pack_row(A.flag_pack, 1 - team), eff_pack_col(A.flag_pack, 1 - team)) <= 1 && s.opp_flag_tile == 12 + (1 - team);
        const bool capture = eff_cheb(nr, nc, eff_pack_row(A.flag_pack, team), eff_pack_col(A.flag_pack, team)) <= 1 && (s.carrying || pickup) &&
                             (!A.home_flag_capture || s.home_flag_tile == 12 + team);
        return f | (pickup ? CTF_EFF_PICKS_UP : 0u) | (capture ? CTF_EFF_CAPTURES : 0u);
    }
    if (a >= 5 && s.type == 3 && s.inv > 0 && cell == 0 && eff_cheb(nr, nc, eff_pack_row(A.spawn_pack, s.team), eff_pack_col(A.spawn_pack, s.team)) > 1 &&
        eff_cheb(nr, nc, eff_pack_row(A.spawn_pack, 1 - s.team), eff_pack_col(A.spawn_pack, 1 - s.team)) > 1)
        return CTF_EFF_LAYS;
    if (a < 5 && s.type == 3 && (cell == 2 || cell == 3)) return CTF_EFF_MINES | (cell == 3 ? CTF_EFF_BREAKS : 0u);
    return 0u;
}

// the nine effects of agent i as bytes 0..7 (lo) and 8 (hi), and its mask
CTF_HD uint32_t eff_agent_effects(const EffectArgs& A, const uint8_t* grid, const uint8_t* rec, int i, uint64_t& lo, uint32_t& hi) {
    const EffAgent s = eff_agent(A, grid, rec, i);
    uint32_t mask = 0;
    lo = 0;
    hi = 0;
    int cell[CTF_N_ACTIONS];
#pragma unroll
    for (int a = 0; a < CTF_N_ACTIONS; a++) {  // the eight loads in flight together (action 4 aims at the agent's own cell: unused)
        int nr, nc;
        eff_target(s.type, s.pr, s.pc, a, nr, nc);
        cell[a] = a == 4 ? -1 : eff_tile(grid, A.G, nr, nc);
    }
#pragma unroll
    for (int a = 0; a < CTF_N_ACTIONS; a++) {
        const uint32_t f = eff_action(A, s, a, cell[a]);
        mask |= (f ? 1u : 0u) << a;
        if (a < 8) lo |= (uint64_t)f << (8 * a);
        else hi = f;
    }
    return mask;
}

// the (k + 1)-th lowest set bit of S for k = mulhi(w[0], popcount(S)); 4 for an empty S, without a draw
CTF_HD int eff_sample(uint32_t S, uint64_t seed, uint32_t env, uint32_t step, uint32_t agent) {
    if (!S) return 4;
    uint32_t w[4];
    philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), env, step, agent, CTF_EFFECT_TAG, w);
    const uint32_t k = (uint32_t)(((uint64_t)w[0] * (uint32_t)__builtin_popcount(S)) >> 32);
    for (uint32_t t = 0; t < k; t++) S &= S - 1;  // drop the k lowest
    return __builtin_ctz(S);
}

// One env: mask[i] (or NULL) and effects[i][9] (or NULL) for the agents of agent_mask, every other byte untouched
static inline void eff_env_effects(const EffectArgs& A, const uint8_t* grid, const uint8_t* rec, uint32_t agent_mask, uint16_t* mask, uint8_t* effects) {
    for (int i = 0; i < A.N; i++) {
        if (!((agent_mask >> i) & 1u)) continue;
        uint64_t lo;
        uint32_t hi;
        const uint32_t m = eff_agent_effects(A, grid, rec, i, lo, hi);
        if (mask) mask[i] = (uint16_t)m;
        if (effects) {
            for (int a = 0; a < 8; a++) effects[i * CTF_N_ACTIONS + a] = (uint8_t)(lo >> (8 * a));
            effects[i * CTF_N_ACTIONS + 8] = (uint8_t)hi;
        }
    }
}
// One env: out[i] = sample(i) for the agents of agent_mask, every other byte untouched.  `env` is the env's GLOBAL index
static inline void eff_env_sample(const EffectArgs& A, const uint8_t* grid, const uint8_t* rec, uint32_t agent_mask, uint64_t seed, uint32_t step,
                                  uint32_t env, int8_t* out) {
    for (int i = 0; i < A.N; i++) {
        if (!((agent_mask >> i) & 1u)) continue;
        uint64_t lo;
        uint32_t hi;
        out[i] = (int8_t)eff_sample(eff_agent_effects(A, grid, rec, i, lo, hi), seed, env, step, (uint32_t)i);
    }
}
