// ctf_effects.hip — k_action_effects and k_random_effective: the rule of ctf_effects.h on the device (ctf_action_effects,
// ctf_random_effective_actions): for every asked agent of every env what each of its nine actions would do if it acted now, as a
// 9-bit mask and nine flag bytes, and a uniform draw among the actions that do something.
//
// One lane per (env, agent).  A block of EFF_BLOCK lanes takes EPB = EFF_BLOCK / N whole envs (the lanes past EPB * N idle: none for
// N = 2, 4, 8, 16), lane t of it agent t % N of the block's env t / N — one multiply and shift (cfg.div_n, exact far beyond 256) —
// so consecutive lanes are the consecutive agents of consecutive envs and a wave's 2-byte masks, 9-byte flag rows and 1-byte actions
// are each one contiguous run of memory.  A lane reads its agent's bytes of the record, the two flag cells and the eight cells its
// actions aim at: unconditional byte loads on clamped indices (a lane past the last env works on the last one, a target outside the
// grid on the nearest cell inside; neither stores anything), index arithmetic in size_t.  No LDS, no atomics, no cross-lane moves;
// the env state is only read.  Stores are plain C++: one 2-byte store for the mask, and the nine flag bytes packed in registers and
// written as eight bytes and one (the row starts at any byte: 9 is odd).
#include <hip/hip_runtime.h>

#include "ctf_effects.h"
#include "ctf_launch.h"

#define EFF_BLOCK 256

struct EffLane {
    size_t e;   // the env (clamped)
    int i;      // the agent
    bool live;  // the lane has an (env, agent) of its own
};
__device__ __forceinline__ EffLane eff_lane(const EffectArgs& A, int epb) {
    const uint32_t t = threadIdx.x;
    const uint32_t el = (uint32_t)(((uint64_t)t * A.div_n.m) >> A.div_n.s);
    const size_t e = (size_t)blockIdx.x * (size_t)epb + (size_t)el;
    const bool live = (int)el < epb && e < (size_t)A.n_envs;
    return EffLane{live ? e : (size_t)A.n_envs - 1, (int)(t - el * (uint32_t)A.N), live};
}

template <bool MASK, bool FLAGS>
__global__ void __launch_bounds__(EFF_BLOCK) k_action_effects(EffectArgs A, int epb, uint16_t* __restrict__ mask, uint8_t* __restrict__ effects,
                                                               uint32_t agent_mask) {
    const EffLane l = eff_lane(A, epb);
    uint64_t lo;
    uint32_t hi;
    const uint32_t m = eff_agent_effects(A, A.grid + l.e * (size_t)A.GS, A.rec + l.e * (size_t)A.RS, l.i, lo, hi);
    if (!(l.live && ((agent_mask >> l.i) & 1u))) return;
    const size_t item = l.e * (size_t)A.N + (size_t)l.i;
    if (MASK) mask[item] = (uint16_t)m;
    if (FLAGS) {
        uint8_t* row = effects + item * (size_t)CTF_N_ACTIONS;
        __builtin_memcpy(row, &lo, 8);
        row[8] = (uint8_t)hi;
    }
}

__global__ void __launch_bounds__(EFF_BLOCK) k_random_effective(EffectArgs A, int epb, int8_t* __restrict__ actions, uint32_t agent_mask, uint64_t seed,
                                                                 uint32_t step, uint32_t env_offset) {
    const EffLane l = eff_lane(A, epb);
    uint64_t lo;
    uint32_t hi;
    const uint32_t S = eff_agent_effects(A, A.grid + l.e * (size_t)A.GS, A.rec + l.e * (size_t)A.RS, l.i, lo, hi);
    if (!(l.live && ((agent_mask >> l.i) & 1u))) return;
    actions[l.e * (size_t)A.N + (size_t)l.i] = (int8_t)eff_sample(S, seed, env_offset + (uint32_t)l.e, step, (uint32_t)l.i);
}

static inline unsigned eff_blocks(const EffectArgs& A, int epb) { return (unsigned)(((size_t)A.n_envs + (size_t)epb - 1) / (size_t)epb); }

extern "C" hipError_t ctf_launch_action_effects(const EffectArgs& A, uint16_t* mask, uint8_t* effects, uint32_t agent_mask, hipStream_t st) {
    if (!agent_mask || A.n_envs < 1 || (!mask && !effects)) return hipSuccess;
    const int epb = EFF_BLOCK / A.N;
    const dim3 grid(eff_blocks(A, epb)), block(EFF_BLOCK);
    if (mask && effects) hipLaunchKernelGGL((k_action_effects<true, true>), grid, block, 0, st, A, epb, mask, effects, agent_mask);
    else if (mask) hipLaunchKernelGGL((k_action_effects<true, false>), grid, block, 0, st, A, epb, mask, effects, agent_mask);
    else hipLaunchKernelGGL((k_action_effects<false, true>), grid, block, 0, st, A, epb, mask, effects, agent_mask);
    return hipGetLastError();
}

extern "C" hipError_t ctf_launch_random_effective(const EffectArgs& A, int8_t* actions, uint32_t agent_mask, uint64_t seed, uint32_t step,
                                                  uint32_t env_offset, hipStream_t st) {
    if (!agent_mask || A.n_envs < 1) return hipSuccess;
    const int epb = EFF_BLOCK / A.N;
    hipLaunchKernelGGL(k_random_effective, dim3(eff_blocks(A, epb)), dim3(EFF_BLOCK), 0, st, A, epb, actions, agent_mask, seed, step, env_offset);
    return hipGetLastError();
}
static_assert(CTF_MAX_AGENTS <= EFF_BLOCK && CTF_N_ACTIONS == 9, "a block takes whole envs; eight flag bytes and one");
