// ctf_step_direct.hip — the step kernel of CTF_RNG_COUNTER_DIRECT: GridworldCtf.step(actions) with the Philox blocks of the
// env's two tapes computed inside the step (ctf_step_core.h: GroupRngDirect) — no rings, no digests, no tail blocks, so every
// launch is the same kind of launch.  The step block (staging, group_step, write-back) is the one k_step runs: ctf_step_block.h.
// A translation unit of its own so that the code objects of the ring modes' kernels (ctf_kernels.hip) are what they were.
#include <hip/hip_runtime.h>

#include "ctf_launch.h"
#include "ctf_step_block.h"

// one wave per block, 64 / W envs per wave; the register budget is k_step's (4 waves per SIMD)
template <bool METRICS, int W, bool META>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_step_direct(DevCfg cfg, DevPtrs p, const int8_t* __restrict__ actions, float* __restrict__ rw32, double* __restrict__ rw64,
              uint8_t* __restrict__ done_out, uint32_t flags, StepMeta sm) {
    extern __shared__ uint32_t lds[];
    step_block<METRICS, W, false, true, META>(cfg, p, actions, rw32, rw64, done_out, flags, (int)blockIdx.x, (int)threadIdx.x, lds, StepPub{}, sm);
}

extern "C" hipError_t ctf_launch_step_direct(const DevCfg& cfg, const DevPtrs& p, const StepArgs& a, int w, int n_step_blocks, size_t lds,
                                             hipStream_t st) {
    with_step_variant(cfg.log_metrics != 0, w, [&](auto M, auto W) {
        with_bool(a.meta != nullptr, [&](auto META) {  // the metadata rows from the step (StepArgs.meta)
            hipLaunchKernelGGL((k_step_direct<M.value, W.value, META.value>), dim3(n_step_blocks), dim3(WAVE), lds, st, cfg, p, a.actions, a.rw32,
                               a.rw64, a.done, a.flags, step_meta(cfg, a));
        });
    });
    return hipGetLastError();
}
