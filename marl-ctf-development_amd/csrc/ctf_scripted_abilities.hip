// ctf_scripted_abilities.hip — k_scripted_abilities: the roles of ctf_scripted.h moved by the agents' ABILITIES (a miner digs, a vaulter
// jumps; bit i of ability_mask, class by type and hp) on the device (ctf_scripted_abilities).
//
// The shape is k_scripted_roles' (ctf_scripted_roles.hip): one lane per grid ROW, one GROUP of W lanes per (env, team), W = 16 when
// G <= 16, else 32; lane i < N of a group holds agent i's bytes; no LDS, no distance array, no atomics; the loop's exits are
// wave-uniform ballots.  What differs:
//   - lane i also reads agent i's hp and keeps the agent's CLASS (scr_class) in bits 18..19 of its word, so the one readlane pass
//     that builds the row's role masks builds the row masks of the diggers and the vaulters as well;
//   - a row keeps three tile masks (OPEN, tile 2, tile 3: scr_row_tiles, the same nine dwords) and the goal sets uncut;
//   - a FIELD is (goal kind, class): up to twelve, searched one after the other by ONE loop (scr_front / scr_pick8 / scr_advance),
//     and only those some asked agent of the wave is in.  The digger's loop carries two pending masks; the vaulter's takes the
//     frontier of rows r - 2 and r + 2 as well, by making each of the two DPP moves twice, cut at the group's edges both times,
//     and keeps a third action bit;
//   - n < G * G is no bound for a digger (a path costs up to 3 G G): the loop ends on "every asker decided" or "nothing emits and
//     nothing is pending", behind SCR_ITER_BOUND.
// Loads are unconditional on clamped indices (a group past the last item works on the last one and stores nothing), index
// arithmetic is size_t, and one byte is stored per asked agent, from lane i (vector stores).  The env state is only read.
#include <hip/hip_runtime.h>

#include "ctf_launch.h"
#include "ctf_scripted.h"
#include "ctf_scripted_dev.h"

template <int W>
__global__ void __launch_bounds__(SCR_WAVE* SCR_WPB) k_scripted_abilities(ScriptArgs A, ScriptAbil B, int8_t* actions, uint32_t agent_mask, uint64_t role_pack,
                                                                           uint32_t ability_mask, uint32_t teams, uint32_t epsilon_q32, uint64_t seed,
                                                                           uint32_t step, uint32_t env_offset) {
    constexpr int GPW = SCR_WAVE / W;  // groups per wave
    const int lane = threadIdx.x & (SCR_WAVE - 1), group = lane / W, r = lane & (W - 1);
    const bool both = teams == 3u;
    const size_t items = (size_t)A.n_envs * (both ? 2u : 1u);
    const size_t gi = ((size_t)blockIdx.x * SCR_WPB + (threadIdx.x / SCR_WAVE)) * GPW + (size_t)group;
    const bool live = gi < items;
    const size_t item = live ? gi : items - 1;
    const size_t e = both ? item >> 1 : item;
    const int team = both ? (int)(item & 1u) : (int)(teams >> 1);
    const int G = A.G, N = A.N;

    uint32_t open, t2, t3;
    scr_row_tiles(A.grid + e * (size_t)A.GS, G, A.GS, r, open, t2, t3);
    const uint8_t* rec = A.rec + e * (size_t)A.RS;
    const int i = r < N ? r : N - 1;  // lane i < N of a group looks after agent i
    const bool asked = live && r < N && ((agent_mask >> i) & 1u) && (int)((A.team_mask >> i) & 1u) == team;
    const uint32_t word_i = scr_agent(A, rec, i);
    const uint32_t cls_i = scr_class(B, rec, i, ability_mask);
    const uint32_t word = (live && r < N && word_i) ? word_i | cls_i << 18 : 0u;

    // the agents as this lane's row sees them
    ScrRoles m = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t dig = 0u, vault = 0u;
    for (int j = 0; j < N; j++) {
        uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)word, j);
#pragma unroll
        for (int g = 1; g < GPW; g++) {
            const uint32_t vg = (uint32_t)__builtin_amdgcn_readlane((int)word, g * W + j);
            v = group == g ? vg : v;
        }
        scr_roles_add(m, A, v & 0x3FFFFu, j, r, team, agent_mask, role_pack);
        scr_class_add(dig, vault, v, r);
    }

    const uint32_t not_first = r > 0 ? 0xFFFFFFFFu : 0u, not_last = r < W - 1 ? 0xFFFFFFFFu : 0u;  // a group's rows end at its own lanes
    const uint32_t set = scr_guard_set(m);
    const uint32_t dil_opp = scr_dil(scr_from_lower_lane(m.opp) & not_first, m.opp, scr_from_upper_lane(m.opp) & not_last, G, r);
    const uint32_t dil_set = scr_dil(scr_from_lower_lane(set) & not_first, set, scr_from_upper_lane(set) & not_last, G, r);
    uint32_t P[SCR_FIELDS], Q[SCR_FIELDS];
    scr_role_fields(m, 0xFFFFFFFFu, r, A.flag_pack, team, dil_opp, dil_set, P, Q);  // Q: the goal sets before any tile is asked for

    int act = 4;
    const int src = group * W + (int)(word & (uint32_t)(W - 1));  // the lane of the row this lane's agent stands in
    const int mine = (asked && (word >> 17)) ? scr_role_field(word, scr_role_of(role_pack, i), m.any) : -1;
#pragma unroll
    for (int fld = 0; fld < SCR_FIELDS; fld++) {
        if (__ballot(P[fld] != 0u) == 0ull) continue;  // uniform: nobody of this wave is in the goal kind
        for (uint32_t cls = 0; cls < SCR_CLASSES; cls++) {
            const uint32_t Pf = scr_class_askers(P[fld], cls, dig, vault);
            if (__ballot(Pf != 0u) == 0ull) continue;  // uniform: nobody of this wave is in the field
            const bool jumps = cls == SCR_VAULTER;
            uint32_t w[3];
            scr_class_cost(cls, open, t2, t3, w);
            ScrFront s = scr_front(Q[fld], w);
            ScrPick8 k = {0u, 0u, 0u, 0u};
            for (int n = 0; n < SCR_ITER_BOUND; n++) {
                const uint32_t up = scr_from_lower_lane(s.e) & not_first, down = scr_from_upper_lane(s.e) & not_last;  // every lane makes the moves
                uint32_t up2 = 0u, down2 = 0u;
                if (jumps) {  // uniform
                    up2 = scr_from_lower_lane(up) & not_first;
                    down2 = scr_from_upper_lane(down) & not_last;
                }
                scr_pick8(k, Pf, s.e, up, down, up2, down2, jumps);
                if (__ballot((Pf & ~k.dec) != 0u) == 0ull) break;
                scr_advance(s, up | down, up2 | down2, jumps, w);
                if (__ballot((s.e | s.p1 | s.p2) != 0u) == 0ull) break;
            }
            const uint32_t dec = (uint32_t)__shfl((int)k.dec, src, SCR_WAVE), b0 = (uint32_t)__shfl((int)k.b0, src, SCR_WAVE),
                           b1 = (uint32_t)__shfl((int)k.b1, src, SCR_WAVE), b2 = (uint32_t)__shfl((int)k.b2, src, SCR_WAVE);
            if (mine == fld && ((word >> 18) & 3u) == cls) act = scr_action8(dec, b0, b1, b2, (int)((word >> 8) & 31u));
        }
    }
    if (epsilon_q32) act = scr_explore(act, epsilon_q32, seed, env_offset + (uint32_t)e, step, (uint32_t)i);  // uniform: epsilon 0 computes no block
    if (asked) actions[e * (size_t)N + (size_t)i] = (int8_t)act;
}

extern "C" hipError_t ctf_launch_scripted_abilities(const ScriptArgs& A, const ScriptAbil& B, int8_t* actions, uint32_t agent_mask, uint64_t role_pack,
                                                    uint32_t ability_mask, uint32_t epsilon_q32, uint64_t seed, uint32_t step, uint32_t env_offset,
                                                    hipStream_t st) {
    // every asked agent a walker by type: the roles' launcher as it is (and, from there, the runner's kernel for an all-runner pack)
    if (!script_any_ability(A, B, agent_mask, ability_mask))
        return ctf_launch_scripted_roles(A, actions, agent_mask, role_pack, epsilon_q32, seed, step, env_offset, st);
    const uint32_t teams = script_teams(A, agent_mask);
    if (!teams || A.n_envs < 1) return hipSuccess;
    const size_t items = (size_t)A.n_envs * (teams == 3u ? 2u : 1u);
    const size_t gpw = A.G <= 16 ? 4 : 2;
    const size_t waves = (items + gpw - 1) / gpw, blocks = (waves + SCR_WPB - 1) / SCR_WPB;
    if (A.G <= 16)
        hipLaunchKernelGGL(k_scripted_abilities<16>, dim3((unsigned)blocks), dim3(SCR_WAVE * SCR_WPB), 0, st, A, B, actions, agent_mask, role_pack,
                           ability_mask, teams, epsilon_q32, seed, step, env_offset);
    else
        hipLaunchKernelGGL(k_scripted_abilities<32>, dim3((unsigned)blocks), dim3(SCR_WAVE * SCR_WPB), 0, st, A, B, actions, agent_mask, role_pack,
                           ability_mask, teams, epsilon_q32, seed, step, env_offset);
    return hipGetLastError();
}
static_assert(CTF_MAX_AGENTS <= 16 && CTF_MAX_GRID <= 32, "a group's first N lanes hold the agents, its W lanes the rows");
