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
// which has checked the list and its length before; 4: the factored path, which has not — the one error text names the factored path
// whatever max_sel is.)
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

// The arguments of a forward kernel of the front (h0_out / h1_out: the training instantiation's, else NULL).
static inline PolicyArgs pol_front_args(const uint8_t* codes, const uint16_t* meta, uint16_t* act, const void* conv1_frag, const float* conv1_bias,
                                        const void* conv2_frag, const float* conv2_bias, int n_envs, int n_agents, int grid_size, int meta_len,
                                        int n_sel, uint64_t sel_pack, int Kp, uint32_t inv_g1, uint32_t inv_g2, uint16_t* h0_out, uint16_t* h1_out) {
    PolicyArgs a;
    a.codes = codes; a.meta = meta; a.act = act;
    a.w1frag = (const u32x4_t*)conv1_frag; a.b1 = conv1_bias;
    a.w2frag = (const u32x4_t*)conv2_frag; a.b2 = conv2_bias;
    a.n_envs = n_envs; a.N = n_agents; a.G = grid_size; a.M = meta_len; a.Kp = Kp; a.n_sel = n_sel;
    a.sel_pack = sel_pack;
    a.inv_g1 = inv_g1; a.inv_g2 = inv_g2;
    a.h0_out = h0_out; a.h1_out = h1_out;
    return a;
}

// Blocks of a launch whose waves each take one item at a time (a sample, an env): enough for all items at `wpb` waves a block, at most
// what the device holds at once — per CU as many blocks as 160 KiB of LDS take at `lds_bytes` each (at least one), capped at `per_cu_cap`.
static inline int64_t pol_blocks(int64_t items, int wpb, size_t lds_bytes, int n_cus, int per_cu_cap) {
    int64_t per_cu = (int64_t)((160 * 1024) / lds_bytes);
    if (per_cu < 1) per_cu = 1;
    if (per_cu > per_cu_cap) per_cu = per_cu_cap;
    const int64_t blocks = (items + wpb - 1) / wpb;
    return blocks < n_cus * per_cu ? blocks : n_cus * per_cu;
}

// The preamble of the training front's entry points, in two halves because every entry point's own alignment checks (and its early
// return for zero samples) sit between them: the argument checks, ..
static inline int pol_train_check(int grid_size, int64_t n_samples, int64_t n_min, int64_t n_max) {
    if (grid_size != 15 && grid_size != 11) return ctf_policy_fail("the training front is built for grid_size 11 and 15 (the reference's maps)");
    if (n_samples < n_min || n_samples > n_max) return ctf_policy_fail("n_samples out of range");
    return 0;
}
// .. and what the launch sizing needs: the kernels' reciprocals and the device's compute units.  (The DeviceScope that follows is the
// entry point's own: it lives until its return.)
struct PolTrainSetup {
    uint32_t inv_g1, inv_g2;
    int n_cus;
};
static inline int pol_train_setup(int grid_size, int device_id, PolTrainSetup* t) {
    if (pol_recips(grid_size, &t->inv_g1, &t->inv_g2)) return -1;
    t->n_cus = ctf_policy_cus(device_id);
    if (!t->n_cus) return ctf_policy_fail("hipGetDeviceProperties failed");
    return 0;
}
