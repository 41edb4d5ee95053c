// ctf_scripted_costs.hip — k_scripted_costs: the COSTS of ctf_scripted.h on the device (ctf_scripted_costs): for every asked agent the
// cost of reaching its goal set under the rules its scripted planner moves by, one int16 per agent.
//
// The shape and the discipline are k_scripted_abilities' (ctf_scripted_abilities.hip): one lane per grid ROW, one GROUP of W lanes per
// (env, team), W = 16 when G <= 16, else 32; lane i < N of a group holds agent i's bytes and class; a FIELD is (goal kind, class),
// searched one after the other by one loop (scr_front / scr_pick8 / scr_advance), only those some asked agent of the wave is in; no
// LDS, no distance array, no atomics; the loop's exits are wave-uniform ballots behind SCR_ITER_BOUND.  Loads are unconditional on
// clamped indices (a group past the last item works on the last one and stores nothing), index arithmetic is size_t, and one 2-byte
// vector store is made per asked agent, from lane i.  The env state is only read.  What differs:
//   - the askers of a field lose the agents that stand in the field's uncut goal set (scr_cost_askers): their cost is 0, as is the
//     cost of an agent decided before the search;
//   - the picks keep no action bits (nothing reads them: the compiler drops them); what is kept is WHEN.  The row lane knows in which
//     iteration a bit of its decided mask appears, the agent lane has to learn it: in an iteration in which some row of the wave
//     decided an asker (a uniform ballot; most iterations decide nobody) every lane reads the decided mask of the row its agent stands
//     in (one ds_bpermute, no LDS memory) and an agent lane that still waits and finds its bit latches n + 1;
//   - whether the agent was an asker of its field at all is one more such read per searched field, before the loop.
// One kernel serves every role and class: there is no delegation to the action launchers.
#include <hip/hip_runtime.h>

#include "ctf_launch.h"
#include "ctf_scripted.h"
#include "ctf_scripted_dev.h"

// v of lane `byte_addr / 4` of the wave
__device__ __forceinline__ uint32_t scr_from_lane(int byte_addr, uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_bpermute(byte_addr, (int)v); }

template <int W>
__global__ void __launch_bounds__(SCR_WAVE* SCR_WPB) k_scripted_costs(ScriptArgs A, ScriptAbil B, int16_t* costs, uint32_t agent_mask, uint64_t role_pack,
                                                                       uint32_t ability_mask, uint32_t teams) {
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

    // asked and inside the grid: 0 unless a search below says otherwise; outside the grid: no cost
    int cost = (word >> 17) ? 0 : CTF_COST_NONE;
    const int src4 = (group * W + (int)(word & (uint32_t)(W - 1))) * 4;  // the lane of the row this lane's agent stands in, as a byte address
    const int pc = (int)((word >> 8) & 31u);
    const int mine = (asked && (word >> 17)) ? scr_role_field(word, scr_role_of(role_pack, i), m.any) : -1;
#pragma unroll
    for (int fld = 0; fld < SCR_FIELDS; fld++) {
        const uint32_t Pa = scr_cost_askers(P[fld], Q[fld]);
        if (__ballot(Pa != 0u) == 0ull) continue;  // uniform: nobody of this wave is in the goal kind
        for (uint32_t cls = 0; cls < SCR_CLASSES; cls++) {
            const uint32_t Pf = scr_class_askers(Pa, cls, dig, vault);
            if (__ballot(Pf != 0u) == 0ull) continue;  // uniform: nobody of this wave is in the field
            const bool jumps = cls == SCR_VAULTER;
            uint32_t w[3];
            scr_class_cost(cls, open, t2, t3, w);
            ScrFront s = scr_front(Q[fld], w);
            ScrPick8 k = {0u, 0u, 0u, 0u};
            // is this lane's agent an asker of the field (every lane makes the read)
            bool wait = ((scr_from_lane(src4, Pf) >> pc) & 1u) && mine == fld && ((word >> 18) & 3u) == cls;
            cost = wait ? CTF_COST_NONE : cost;
            for (int n = 0; n < SCR_ITER_BOUND; n++) {
                const uint32_t up = scr_from_lower_lane(s.e) & not_first, down = scr_from_upper_lane(s.e) & not_last;  // every lane makes the moves
                uint32_t up2 = 0u, down2 = 0u;
                if (jumps) {  // uniform
                    up2 = scr_from_lower_lane(up) & not_first;
                    down2 = scr_from_upper_lane(down) & not_last;
                }
                const uint32_t before = k.dec;
                scr_pick8(k, Pf, s.e, up, down, up2, down2, jumps);
                if (__ballot(k.dec != before) != 0ull) {  // uniform: some row of the wave decided an asker in this iteration
                    const uint32_t dec = scr_from_lane(src4, k.dec);  // every lane makes the read: a lane that is switched off shows 0
                    const bool hit = wait && ((dec >> pc) & 1u);
                    cost = hit ? scr_cost_of_iteration(n) : cost;
                    wait = wait && !hit;
                }
                if (__ballot((Pf & ~k.dec) != 0u) == 0ull) break;
                scr_advance(s, up | down, up2 | down2, jumps, w);
                if (__ballot((s.e | s.p1 | s.p2) != 0u) == 0ull) break;
            }
        }
    }
    if (asked) costs[e * (size_t)N + (size_t)i] = (int16_t)cost;
}

extern "C" hipError_t ctf_launch_scripted_costs(const ScriptArgs& A, const ScriptAbil& B, int16_t* costs, uint32_t agent_mask, uint64_t role_pack,
                                                uint32_t ability_mask, hipStream_t st) {
    const uint32_t teams = script_teams(A, agent_mask);
    if (!teams || A.n_envs < 1) return hipSuccess;
    const size_t items = (size_t)A.n_envs * (teams == 3u ? 2u : 1u);
    const size_t gpw = A.G <= 16 ? 4 : 2;
    const size_t waves = (items + gpw - 1) / gpw, blocks = (waves + SCR_WPB - 1) / SCR_WPB;
    if (A.G <= 16)
        hipLaunchKernelGGL(k_scripted_costs<16>, dim3((unsigned)blocks), dim3(SCR_WAVE * SCR_WPB), 0, st, A, B, costs, agent_mask, role_pack, ability_mask,
                           teams);
    else
        hipLaunchKernelGGL(k_scripted_costs<32>, dim3((unsigned)blocks), dim3(SCR_WAVE * SCR_WPB), 0, st, A, B, costs, agent_mask, role_pack, ability_mask,
                           teams);
    return hipGetLastError();
}
static_assert(CTF_MAX_AGENTS <= 16 && CTF_MAX_GRID <= 32, "a group's first N lanes hold the agents, its W lanes the rows");
static_assert(3 * CTF_MAX_CELLS < 32768, "a finite cost fits an int16");
