// ctf_policy_host.h — the host side every entry point of include/ctf_policy.h shares (ctf_policy.hip, ctf_policy_fact.hip,
// ctf_policy_tail.hip): an entry point validates its arguments, declares a DeviceScope, sizes its launch, goes through pol_launch
// and leaves through pol_finish.  Host only; no state of its own.
#pragma once
#include "ctf_device_scope.h"
#include "ctf_policy_dev.h"

// defined in ctf_policy.hip
__attribute__((visibility("hidden"))) int ctf_policy_fail(const char* msg);  // sets ctf_policy_last_error(), returns -1
__attribute__((visibility("hidden"))) int ctf_policy_cus(int device_id);      // compute units of a device (cached), 0 on error

// Deterministic mode (ctf_policy_set_deterministic, include/ctf_policy.h): with a workspace registered for the device, the weight /
// bias gradient kernels do not end in float atomics on the gradient (whose order of arrival differs from run to run) — every block
// stores its partial sums in its own slice of the workspace and a second launch adds the slices IN BLOCK ORDER.
struct DetWorkspace {
    float* ptr;      // NULL: off (atomics)
    int64_t floats;
};
__attribute__((visibility("hidden"))) DetWorkspace ctf_policy_det(int device_id);
// dst[i] += sum over b = 0 .. n_blocks - 1 (in that order, four interleaved chains) of part[b * stride + i], i < elems
__attribute__((visibility("hidden"))) hipError_t ctf_policy_det_reduce(const float* part, int n_blocks, int64_t stride, int elems, float* dst,
                                                                      hipStream_t st);
// what a launch whose partial sums do not fit the registered workspace reports instead of launching (pol_finish words it)
#define POL_WORKSPACE_TOO_SMALL hipErrorOutOfMemory

// One launch: dynamic LDS beyond the 48 KiB every kernel may have needs the attribute first (set on every call: it is per device).
template <typename Args>
static inline hipError_t pol_launch(void (*kernel)(Args), int64_t blocks, int threads, size_t lds_bytes, hipStream_t st, const Args& args) {
    if (lds_bytes > 48 * 1024) {
        const hipError_t err = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (err != hipSuccess) return err;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), lds_bytes, st, args);
    return hipGetLastError();
}

// the end of every entry point: 0, or -1 with ctf_policy_last_error() set
static inline int pol_finish(hipError_t err) {
    if (err == hipSuccess) return 0;
    if (err == POL_WORKSPACE_TOO_SMALL)
        return ctf_policy_fail("deterministic mode: the registered workspace is too small for this launch (ctf_policy_set_deterministic)");
    return ctf_policy_fail(hipGetErrorString(err));
}

// a profiling-only knob: the variable's value when it is set and lies in lo..hi, else `fallback` (read on every call)
static inline int pol_env_int(const char* name, int lo, int hi, int fallback) {
    const char* ov = getenv(name);
    if (!ov) return fallback;
    const int v = atoi(ov);
    return v >= lo && v <= hi ? v : fallback;
}

// The kernels divide a position by G-2 and G-4 as (p * inv) >> 16 with inv = ceil(65536 / divisor): proven exact here for every
// position they will see.  0, or -1 with the error set.
static inline int pol_recips(int grid_size, uint32_t* inv_g1, uint32_t* inv_g2) {
    const int G1 = grid_size - 2, G2 = grid_size - 4;
    *inv_g1 = (65536 + G1 - 1) / G1;
    *inv_g2 = (65536 + G2 - 1) / G2;
    for (int p = 0; p < G1 * G1; p++)
        if ((int)(((uint32_t)p * *inv_g1) >> 16) != p / G1) return ctf_policy_fail("internal: reciprocal of G-2 not exact");
    for (int p = 0; p < G2 * G2; p++)
        if ((int)(((uint32_t)p * *inv_g2) >> 16) != p / G2) return ctf_policy_fail("internal: reciprocal of G-4 not exact");
    return 0;
}

// agent_sel[0 .. n_sel-1] -> nibble k = agent index of selection slot k.  0, or -1 with the error set.  (max_sel 16: ctf_policy_features,
// which has checked the list and its length before; 4: the factored path, which has not.)
static inline int pol_pack_sel(const int32_t* agent_sel, int n_sel, int n_agents, int max_sel, uint64_t* out) {
    if (!agent_sel || n_sel < 1 || n_sel > max_sel) return ctf_policy_fail("the factored path takes 1..4 selected agents");
    uint64_t p = 0;
    for (int k = 0; k < n_sel; k++) {
        if (agent_sel[k] < 0 || agent_sel[k] >= n_agents) return ctf_policy_fail("agent_sel entry out of range");
        p |= (uint64_t)agent_sel[k] << (4 * k);
    }
    *out = p;
    return 0;
}
