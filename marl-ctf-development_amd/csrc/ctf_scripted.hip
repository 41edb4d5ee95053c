// ctf_scripted.hip — k_scripted_actions: the scripted opponents of ctf_scripted.h on the device (ctf_scripted_actions).
//
// One lane per grid ROW, one GROUP of W lanes per (env, team): W = 16 when G <= 16 (four groups per wave), else 32 (two).  With
// agents of both teams asked for, consecutive groups are the two teams of one env; with one team, consecutive envs.  A group runs up
// to two breadth-first searches, one per FIELD (the team's agents that do not carry a flag head for the other flag, those that do
// for their own), and only the fields some asked agent is in.  A search keeps four masks per lane (frontier, seen, open, askers)
// and the three of ScrPick; the rows above and below come from the neighbouring lanes with one DPP move each (wave_shr:1 /
// wave_shl:1, cut at the groups' edges), and the loop's two exits — every asker decided, frontier empty — are wave-uniform
// ballots.  No LDS, no distance array, no atomics.
// Loads: the row's dwords of the grid and, in lane i < N of a group, agent i's position and flag bytes (N <= 16 <= W), all
// unconditional on clamped indices (a group past the last item works on the last one and stores nothing).  Stores: one byte per
// asked agent, from lane i (vector stores).  Index arithmetic is size_t.  The env state is only read; the env's generators are
// not touched.
#include <hip/hip_runtime.h>

#include "ctf_launch.h"
#include "ctf_scripted.h"
#include "ctf_scripted_dev.h"

template <int W>
__global__ void __launch_bounds__(SCR_WAVE* SCR_WPB) k_scripted_actions(ScriptArgs A, int8_t* actions, uint32_t agent_mask, uint32_t teams,
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
    const uint32_t ask_i = scr_asker(A, rec, i, agent_mask, team);
    const uint32_t ask = (live && r < N) ? ask_i : 0u;

    // the askers of this lane's row, per field
    uint32_t P[2] = {0u, 0u};
    for (int j = 0; j < N; j++) {
        uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)ask, j);
#pragma unroll
        for (int g = 1; g < GPW; g++) {
            const uint32_t vg = (uint32_t)__builtin_amdgcn_readlane((int)ask, g * W + j);
            v = group == g ? vg : v;
        }
        const uint32_t bit = ((v >> 17) && (int)(v & 0xFFu) == r) ? 1u << ((v >> 8) & 31u) : 0u;
        P[0] |= (v & 0x10000u) ? 0u : bit;
        P[1] |= (v & 0x10000u) ? bit : 0u;
    }

    int act = 4;
    const uint32_t not_first = r > 0 ? 0xFFFFFFFFu : 0u, not_last = r < W - 1 ? 0xFFFFFFFFu : 0u;  // a group's rows end at its own lanes
    const int src = group * W + (int)(ask & (uint32_t)(W - 1));  // the lane of the row this lane's agent stands in
#pragma unroll
    for (int carrying = 0; carrying < 2; carrying++) {
        const uint32_t Pc = P[carrying];
        if (__ballot(Pc != 0u) == 0ull) continue;  // uniform: nobody of this wave is in the field
        int tr, tc;
        scr_target(A.flag_pack, team, carrying, tr, tc);
        uint32_t f = scr_goal_row(open, r, tr, tc), seen = f;
        ScrPick k = {0u, 0u, 0u};
        for (int n = 0; n < G * G; n++) {
            const uint32_t up = scr_from_lower_lane(f) & not_first, down = scr_from_upper_lane(f) & not_last;  // every lane makes both moves
            scr_pick(k, Pc, f, up, down);
            if (__ballot((Pc & ~k.dec) != 0u) == 0ull) break;
            f = scr_step(f, up, down, open, seen);
            seen |= f;
            if (__ballot(f != 0u) == 0ull) break;
        }
        const uint32_t dec = (uint32_t)__shfl((int)k.dec, src, SCR_WAVE), b0 = (uint32_t)__shfl((int)k.b0, src, SCR_WAVE),
                       b1 = (uint32_t)__shfl((int)k.b1, src, SCR_WAVE);
        if ((ask >> 17) && (int)((ask >> 16) & 1u) == carrying) act = scr_action(dec, b0, b1, (int)((ask >> 8) & 31u));
    }
    if (epsilon_q32) act = scr_explore(act, epsilon_q32, seed, env_offset + (uint32_t)e, step, (uint32_t)i);  // uniform: epsilon 0 computes no block
    if (asked) actions[e * (size_t)N + (size_t)i] = (int8_t)act;
}

extern "C" hipError_t ctf_launch_scripted_actions(const ScriptArgs& A, int8_t* actions, uint32_t agent_mask, uint32_t epsilon_q32, uint64_t seed,
                                                  uint32_t step, uint32_t env_offset, hipStream_t st) {
    const uint32_t teams = script_teams(A, agent_mask);
    if (!teams || A.n_envs < 1) return hipSuccess;  // nobody asked: nothing to write
    const size_t items = (size_t)A.n_envs * (teams == 3u ? 2u : 1u);
    const size_t gpw = A.G <= 16 ? 4 : 2;
    const size_t waves = (items + gpw - 1) / gpw, blocks = (waves + SCR_WPB - 1) / SCR_WPB;
    if (A.G <= 16)
        hipLaunchKernelGGL(k_scripted_actions<16>, dim3((unsigned)blocks), dim3(SCR_WAVE * SCR_WPB), 0, st, A, actions, agent_mask, teams, epsilon_q32, seed,
                           step, env_offset);
    else
        hipLaunchKernelGGL(k_scripted_actions<32>, dim3((unsigned)blocks), dim3(SCR_WAVE * SCR_WPB), 0, st, A, actions, agent_mask, teams, epsilon_q32, seed,
                           step, env_offset);
    return hipGetLastError();
}
static_assert(CTF_MAX_AGENTS <= 16 && CTF_MAX_GRID <= 32, "a group's first N lanes hold the agents, its W lanes the rows");
