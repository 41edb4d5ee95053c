// ctf_scripted_roles.hip — k_scripted_roles: the roles of ctf_scripted.h (runner, chaser, guard; one nibble of role_pack per agent) on
// the device (ctf_scripted_roles).
//
// The shape is k_scripted_actions' (ctf_scripted.hip): one lane per grid ROW, one GROUP of W lanes per (env, team), W = 16 when
// G <= 16, else 32; no LDS, no distance array, no atomics; the loop's exits are wave-uniform ballots.  What differs:
//   - lane i < N of a group holds the bytes of agent i WHOEVER it plays for, so the one readlane pass that builds the row's asker masks
//     builds the opponents' row masks as well (ScrRoles);
//   - dil(S) of a row is h(S[r - 1] | S[r] | S[r + 1]) (scr_dil): the rows above and below come with the frontier's two DPP moves,
//     cut at the group's edges, once for the opponents and once for the guards' set; every lane makes all four moves;
//   - a group has up to four FIELDS (scr_role_fields), searched one after the other, and only those some asked agent of the wave is
//     in; who is decided before the search (a chaser that tags already, a posted guard next to its flag) is not in its field's mask.
// Loads are unconditional on clamped indices (a group past the last item works on the last one and stores nothing), index
// arithmetic is size_t, and one byte is stored per asked agent, from lane i (vector stores).  The env state is only read.
#include <hip/hip_runtime.h>

#include "ctf_launch.h"
#include "ctf_scripted.h"
#include "ctf_scripted_dev.h"

template <int W>
__global__ void __launch_bounds__(SCR_WAVE* SCR_WPB) k_scripted_roles(ScriptArgs A, int8_t* actions, uint32_t agent_mask, uint64_t role_pack, uint32_t teams,
                                                                       uint32_t epsilon_q32, uint64_t seed, uint32_t step, uint32_t env_offset) {
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

    const uint32_t open = scr_row_open(A.grid + e * (size_t)A.GS, G, A.GS, r);
    const uint8_t* rec = A.rec + e * (size_t)A.RS;
    const int i = r < N ? r : N - 1;  // lane i < N of a group looks after agent i
    const bool asked = live && r < N && ((agent_mask >> i) & 1u) && (int)((A.team_mask >> i) & 1u) == team;
    const uint32_t word_i = scr_agent(A, rec, i);
    const uint32_t word = (live && r < N) ? word_i : 0u;

    // the agents as this lane's row sees them
    ScrRoles m = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (int j = 0; j < N; j++) {
        uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)word, j);
#pragma unroll
        for (int g = 1; g < GPW; g++) {
            const uint32_t vg = (uint32_t)__builtin_amdgcn_readlane((int)word, g * W + j);
            v = group == g ? vg : v;
        }
        scr_roles_add(m, A, v, j, r, team, agent_mask, role_pack);
    }

    const uint32_t not_first = r > 0 ? 0xFFFFFFFFu : 0u, not_last = r < W - 1 ? 0xFFFFFFFFu : 0u;  // a group's rows end at its own lanes
    const uint32_t set = scr_guard_set(m);
    const uint32_t dil_opp = scr_dil(scr_from_lower_lane(m.opp) & not_first, m.opp, scr_from_upper_lane(m.opp) & not_last, G, r);
    const uint32_t dil_set = scr_dil(scr_from_lower_lane(set) & not_first, set, scr_from_upper_lane(set) & not_last, G, r);
    uint32_t P[SCR_FIELDS], goal[SCR_FIELDS];
    scr_role_fields(m, open, r, A.flag_pack, team, dil_opp, dil_set, P, goal);

    int act = 4;
    const int src = group * W + (int)(word & (uint32_t)(W - 1));  // the lane of the row this lane's agent stands in
    const int mine = (asked && (word >> 17)) ? scr_role_field(word, scr_role_of(role_pack, i), m.any) : -1;
#pragma unroll
    for (int fld = 0; fld < SCR_FIELDS; fld++) {
        const uint32_t Pf = P[fld];
        if (__ballot(Pf != 0u) == 0ull) continue;  // uniform: nobody of this wave is in the field
        uint32_t f = goal[fld], seen = f;
        ScrPick k = {0u, 0u, 0u};
        for (int n = 0; n < G * G; n++) {
            const uint32_t up = scr_from_lower_lane(f) & not_first, down = scr_from_upper_lane(f) & not_last;  // every lane makes both moves
            scr_pick(k, Pf, f, up, down);
            if (__ballot((Pf & ~k.dec) != 0u) == 0ull) break;
            f = scr_step(f, up, down, open, seen);
            seen |= f;
            if (__ballot(f != 0u) == 0ull) break;
        }
        const uint32_t dec = (uint32_t)__shfl((int)k.dec, src, SCR_WAVE), b0 = (uint32_t)__shfl((int)k.b0, src, SCR_WAVE),
                       b1 = (uint32_t)__shfl((int)k.b1, src, SCR_WAVE);
        if (mine == fld) act = scr_action(dec, b0, b1, (int)((word >> 8) & 31u));
    }
    if (epsilon_q32) act = scr_explore(act, epsilon_q32, seed, env_offset + (uint32_t)e, step, (uint32_t)i);  // uniform: epsilon 0 computes no block
    if (asked) actions[e * (size_t)N + (size_t)i] = (int8_t)act;
}

extern "C" hipError_t ctf_launch_scripted_roles(const ScriptArgs& A, int8_t* actions, uint32_t agent_mask, uint64_t role_pack, uint32_t epsilon_q32,
                                                uint64_t seed, uint32_t step, uint32_t env_offset, hipStream_t st) {
    bool runners = true;
    for (int i = 0; i < A.N; i++) runners = runners && !(((agent_mask >> i) & 1u) && scr_role_of(role_pack, i) != CTF_ROLE_RUNNER);
    if (runners) return ctf_launch_scripted_actions(A, actions, agent_mask, epsilon_q32, seed, step, env_offset, st);  // the runner's kernel as it is
    const uint32_t teams = script_teams(A, agent_mask);
    if (!teams || A.n_envs < 1) return hipSuccess;
    const size_t items = (size_t)A.n_envs * (teams == 3u ? 2u : 1u);
    const size_t gpw = A.G <= 16 ? 4 : 2;
    const size_t waves = (items + gpw - 1) / gpw, blocks = (waves + SCR_WPB - 1) / SCR_WPB;
    if (A.G <= 16)
        hipLaunchKernelGGL(k_scripted_roles<16>, dim3((unsigned)blocks), dim3(SCR_WAVE * SCR_WPB), 0, st, A, actions, agent_mask, role_pack, teams, epsilon_q32,
                           seed, step, env_offset);
    else
        hipLaunchKernelGGL(k_scripted_roles<32>, dim3((unsigned)blocks), dim3(SCR_WAVE * SCR_WPB), 0, st, A, actions, agent_mask, role_pack, teams, epsilon_q32,
                           seed, step, env_offset);
    return hipGetLastError();
}
static_assert(CTF_MAX_AGENTS <= 16 && CTF_MAX_GRID <= 32, "a group's first N lanes hold the agents, its W lanes the rows");
