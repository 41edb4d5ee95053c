// ctf_scripted_dev.h — what the scripted kernels (ctf_scripted.hip, ctf_scripted_roles.hip, ctf_scripted_abilities.hip, ctf_scripted_costs.hip) share on the device: the launch shape and
// the two cross-lane moves that bring a row the masks of the rows above and below it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SCR_WAVE 64
#define SCR_WPB 4  // waves per block

// f of the lane below / above in the wave (0 at the wave's ends)
__device__ __forceinline__ uint32_t scr_from_lower_lane(uint32_t f) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)f, 0x138 /* wave_shr:1 */, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t scr_from_upper_lane(uint32_t f) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)f, 0x130 /* wave_shl:1 */, 0xF, 0xF, true);
}
