// ctf_launch.h — the launch interface between the translation units of the env side: everything ctf_abi.hip calls in
// ctf_kernels.hip, ctf_observe_delta.hip, ctf_step_direct.hip, ctf_rng.hip, ctf_snapshot.hip, ctf_harvest.hip, ctf_visitation.hip, ctf_states.hip, ctf_scripted.hip, ctf_scripted_roles.hip, ctf_scripted_abilities.hip, ctf_scripted_costs.hip, ctf_effects.hip and ctf_scatter.hip.  Every file that defines or calls one of these includes
// this header, so a parameter list cannot drift between them unnoticed (the names have C linkage: a mismatch would link).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ctf_device.h"
#include "ctf_effects.h"
#include "ctf_harvest.h"
#include "ctf_scatter.h"
#include "ctf_scripted.h"
#include "ctf_snapshot.h"
#include "ctf_states.h"
#include "ctf_visitation.h"

// what one step reads and writes (ctf_step's arguments)
struct StepArgs {
    const int8_t* actions;
    float* rw32;
    double* rw64;
    uint8_t* done;
    uint32_t flags;
    uint16_t* meta = nullptr;  // not NULL: the step also writes the envs' metadata rows f16 [E][N][M] (ctf_step_observe; ctf_meta.h)
};
// what one render writes (ctf_observe's arguments) ...
struct RenderArgs {
    uint8_t* obs;
    uint16_t* meta;
    uint32_t reverse_mask;
    // ... and, for the one-launch form only: the handle's sync words (ctf_sync_words) and a tile's bound on its wait, in wall-clock ticks
    uint32_t* sync;
    uint64_t spin_ticks;
};

extern "C" {
// ---- ctf_kernels.hip
hipError_t ctf_launch_reset(const DevCfg&, const DevPtrs&, const uint8_t* mask, int init_perm, hipStream_t);
hipError_t ctf_launch_step(const DevCfg&, const DevPtrs&, const StepArgs&, int with_tail, hipStream_t);
hipError_t ctf_launch_step_observe(const DevCfg&, const DevPtrs&, const StepArgs&, const RenderArgs&, hipStream_t);
// ---- ctf_step_direct.hip: the step of CTF_RNG_COUNTER_DIRECT, in the shape ctf_launch_step worked out (w lanes per env)
hipError_t ctf_launch_step_direct(const DevCfg&, const DevPtrs&, const StepArgs&, int w, int n_step_blocks, size_t lds, hipStream_t);
hipError_t ctf_launch_observe(const DevCfg&, const DevPtrs&, const RenderArgs&, int n_cus, hipStream_t);
hipError_t ctf_launch_observe_codes(const DevCfg&, const DevPtrs&, uint8_t* codes, uint16_t* meta, uint16_t* selfcells, uint32_t reverse_mask,
                                    int n_cus, hipStream_t);
hipError_t ctf_launch_export_counters(const DevCfg&, const DevPtrs&, int32_t* metrics, int32_t* captures, int32_t* steps, hipStream_t);
hipError_t ctf_launch_random_actions(const DevCfg&, int8_t* actions, uint64_t seed, uint32_t step, uint32_t env_offset, hipStream_t);
int ctf_step_blocks(const DevCfg&);                                // step blocks of a step launch
int ctf_observe_uses_tiles(const DevCfg&, const uint8_t* obs);       // 1: a render into `obs` is k_observe_tiles, 0: k_observe
int ctf_step_observe_one_launch(const DevCfg&, const uint8_t* obs);  // 1: ctf_step_observe is k_step_observe, 0: two launches
// ---- ctf_observe_delta.hip: the retained render
hipError_t ctf_launch_observe_delta(const DevCfg&, const DevPtrs&, const ObsShadow&, const RenderArgs&, int store_nt, int bitmap, uint32_t flags, hipStream_t);
hipError_t ctf_launch_obs_key_clear(const ObsShadow&, int n_envs, hipStream_t);
int ctf_observe_delta_applies(const DevCfg&, const uint8_t* obs);    // 1: a retained `obs` can take k_observe_delta
// ---- ctf_rng.hip (envs [e0, e0 + count): record b of the arrays belongs to env e0 + b)
hipError_t ctf_launch_seed(const DevCfg&, const DevPtrs&, const uint64_t* py_seeds, const uint64_t* np_seeds, hipStream_t);
hipError_t ctf_launch_import_rng(const DevCfg&, const DevPtrs&, const uint32_t* py, const uint32_t* np_, int e0, int count, hipStream_t);
hipError_t ctf_launch_export_rng(const DevCfg&, const DevPtrs&, uint32_t* py, uint32_t* np_, int e0, int count, hipStream_t);
hipError_t ctf_launch_rng_refill(const DevCfg&, const DevPtrs&, int e0, int count, int init, hipStream_t);
hipError_t ctf_launch_get_counters(const DevCfg&, const DevPtrs&, unsigned long long* out, hipStream_t);
hipError_t ctf_launch_set_counters(const DevCfg&, const DevPtrs&, const unsigned long long* in, hipStream_t);
// ---- ctf_snapshot.hip
hipError_t ctf_launch_save_states(const SnapLayout&, const int32_t* idx, int n, uint8_t* dst, hipStream_t);
hipError_t ctf_launch_load_states(const SnapLayout&, const uint8_t* src, const int32_t* idx, int n, hipStream_t);
// ---- ctf_harvest.hip
hipError_t ctf_launch_harvest(const HarvestArgs&, const int32_t* group, int n_groups, const uint8_t* mask, uint32_t flags, int64_t* out, hipStream_t);
// ---- ctf_visitation.hip
hipError_t ctf_launch_visit_harvest(const VisitArgs&, const int32_t* group, int n_groups, const uint8_t* mask, uint32_t flags, int64_t* acc, hipStream_t);
hipError_t ctf_launch_visit_export(const VisitArgs&, const int32_t* idx, int n, uint32_t* out, hipStream_t);
// ---- ctf_states.hip
hipError_t ctf_launch_export_states(const StateShape&, const StateDev&, const int32_t* idx, int n, const StateArrays& out, hipStream_t);
hipError_t ctf_launch_import_states(const StateShape&, const StateDev&, const StateArrays& in, const int32_t* idx, int n, hipStream_t);
// ---- ctf_scripted.hip
hipError_t ctf_launch_scripted_actions(const ScriptArgs&, int8_t* actions, uint32_t agent_mask, uint32_t epsilon_q32, uint64_t seed, uint32_t step,
                                       uint32_t env_offset, hipStream_t);
// ---- ctf_scripted_roles.hip (all asked agents runners: ctf_launch_scripted_actions)
hipError_t ctf_launch_scripted_roles(const ScriptArgs&, int8_t* actions, uint32_t agent_mask, uint64_t role_pack, uint32_t epsilon_q32, uint64_t seed,
                                     uint32_t step, uint32_t env_offset, hipStream_t);
// ---- ctf_scripted_abilities.hip (every asked agent a walker by type: ctf_launch_scripted_roles)
hipError_t ctf_launch_scripted_abilities(const ScriptArgs&, const ScriptAbil&, int8_t* actions, uint32_t agent_mask, uint64_t role_pack,
                                         uint32_t ability_mask, uint32_t epsilon_q32, uint64_t seed, uint32_t step, uint32_t env_offset, hipStream_t);
// ---- ctf_scripted_costs.hip (one kernel for every role and class; nothing is launched for an empty mask)
hipError_t ctf_launch_scripted_costs(const ScriptArgs&, const ScriptAbil&, int16_t* costs, uint32_t agent_mask, uint64_t role_pack, uint32_t ability_mask,
                                     hipStream_t);
// ---- ctf_effects.hip (one kernel each; nothing is launched for an empty mask)
hipError_t ctf_launch_action_effects(const EffectArgs&, uint16_t* mask, uint8_t* effects, uint32_t agent_mask, hipStream_t);
hipError_t ctf_launch_random_effective(const EffectArgs&, int8_t* actions, uint32_t agent_mask, uint64_t seed, uint32_t step, uint32_t env_offset,
                                       hipStream_t);
// ---- ctf_scatter.hip (one kernel; the caller sends radius 0 / an empty agent mask without an episode counter to ctf_launch_reset)
hipError_t ctf_launch_reset_scattered(const ScatterArgs&, const uint8_t* mask, uint32_t agent_mask, int32_t radius, uint32_t flags, uint64_t seed,
                                      uint32_t round, uint32_t* episode, uint32_t env_offset, hipStream_t);
}
