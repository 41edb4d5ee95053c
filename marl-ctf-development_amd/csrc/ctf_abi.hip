// ctf_abi.hip — host side of the C ABI declared in include/ctf_env.h.
//
// Owns the device-side SoA state of one handle (one per GPU / shard), validates the config, derives
// the device constant block and enqueues the kernels of the other translation units (ctf_launch.h) on
// the caller's HIP stream.
// No torch, no C++ types across the boundary, no CPU implementation of the path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "ctf_device.h"
#include "ctf_device_scope.h"
#include "ctf_harvest.h"
#include "ctf_launch.h"
#include "ctf_obs_chunk.h"
#include "ctf_snapshot.h"
#include "ctf_state_view.h"
#include "ctf_states.h"
#include "ctf_visitation.h"

struct ctf_env {
    ctf_config cfg;
    DevCfg d;
    DevPtrs p;
    int device;
    int n_cus;
    uint64_t* seed_scratch;  // device, 2*E u64
    uint32_t* rng_scratch;   // device, 2 x 625 u32: one env's two generators in the standard form (ctf_set/get_rng_state)
    // ctf_host_step (n_envs == 1): one pinned, device-mapped host block (allocated on first use) that the kernels read and write directly
    uint8_t* hio_dev;   // the DEVICE address of that block (hipHostGetDevicePointer)
    uint8_t* hio_host;  // its host address
    int nt_override;    // CTF_OBS_NT at create: 0 / 1 force the render's store hint off / on, -1 = the rule (store_hint)
    uint32_t* sync;     // device, ctf_sync_words(E) u32, zeroed at create: k_step_observe's generation, reader counters and flags
    uint64_t spin_ticks;  // 10 ms of the device's wall clock: a render tile's bound on its wait in k_step_observe
    uint64_t fingerprint;  // of the config (ctf_snapshot.h): which handles' snapshot records this one reads
    // the retained observation buffer (ctf_obs_retain): its address (NULL = none) and the device-side shadow of what was last
    // rendered into it, allocated at the first retain.  Whether that shadow is VALID is device state (its keys), never a host flag.
    uint8_t* retained;
    ObsShadow shadow;
    int delta_nt;       // CTF_OBS_DELTA_NT at retain: 0 / 1 force the delta render's store hint off / on, -1 = the full render's rule (store_hint)
    int delta_bitmap;   // CTF_OBS_DELTA_BITMAP=1 at retain: the delta render is the round-11 kernel (the bitmap of the whole block)
    uint32_t delta_flags;  // CTF_OBS_DELTA_REBUILD / CTF_OBS_DELTA_ALL_DIRTY at retain: CTF_OBS_DELTA_F_* (ctf_device.h)
};

// Layout of the ctf_host_step block (byte offsets; every segment 16-byte aligned, the observation 256-byte aligned).
struct HostIo {
    size_t actions, py_in, np_in, in_end;                               // host -> device
    size_t out, rw64, done_status, py_out, np_out, obs, meta, grid, rec, metrics, vis, vislog, end;  // device -> host
};
static size_t up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static HostIo host_io_layout(const DevCfg& d) {
    HostIo L;
    const size_t mt = up((CTF_MT_N + 1) * 4, 16);
    L.actions = 0;
    L.py_in = 16;
    L.np_in = L.py_in + mt;
    L.in_end = L.np_in + mt;
    L.out = up(L.in_end, 256);
    L.rw64 = L.out;
    L.done_status = L.rw64 + CTF_MAX_AGENTS * 8;
    L.py_out = L.done_status + 16;
    L.np_out = L.py_out + mt;
    L.obs = up(L.np_out + mt, 256);
    L.meta = L.obs + up((size_t)d.obs_bytes, 16);
    L.grid = L.meta + up((size_t)d.N * d.M * 2, 16);
    L.rec = L.grid + (size_t)d.GS;
    L.metrics = L.rec + (size_t)d.RS;
    L.vis = L.metrics + up((size_t)CTF_N_METRICS * d.N * 4, 16);
    L.vislog = L.vis + (d.log_metrics ? (size_t)d.N * d.GS * 4 : 0);
    L.end = L.vislog + (d.log_metrics ? (size_t)CTF_VIS_LOG * d.N * 2 : 0);
    return L;
}

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) return fail(CTF_E_HIP, "%s -> %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// The render's nontemporal store hint (ctf_derive.h has the why and the measured crossover) follows what ALL live handles of this
// process on the device write per step, not one handle's share: four shards of 8 192 arena envs (206 MB each) stored plain read
// 183 M env-steps/s, hinted 218 M — each fits the caches, the four together do not (profiles/r05_two_shards_overlap.md).  Other
// PROCESSES on the device are not seen: CTF_OBS_NT=1 is for them.
#define CTF_MAX_DEVICES 64
static std::atomic<long long> g_obs_bytes[CTF_MAX_DEVICES];
static long long obs_total(const ctf_env* h) { return (long long)h->d.n_envs * h->d.obs_bytes; }
static int store_hint(const ctf_env* h) {
    if (h->nt_override >= 0) return h->nt_override;
    const long long all = h->device >= 0 && h->device < CTF_MAX_DEVICES ? g_obs_bytes[h->device].load(std::memory_order_relaxed) : obs_total(h);
    return all > ((long long)320 << 20);
}

#include "ctf_derive.h"

static void free_all(ctf_env* h) {
    if (!h) return;
    (void)hipFree(h->p.grid); (void)hipFree(h->p.rec); (void)hipFree(h->p.mt_py); (void)hipFree(h->p.mt_np);
    (void)hipFree(h->p.rngpos); (void)hipFree(h->p.metrics); (void)hipFree(h->p.vis); (void)hipFree(h->p.vislog);
    (void)hipFree((void*)h->p.init_grid); (void)hipFree((void*)h->p.meta_lut); (void)hipFree(h->p.status); (void)hipFree(h->seed_scratch);
    (void)hipFree(h->p.rngctr); (void)hipFree(h->rng_scratch); (void)hipFree(h->p.rngready); (void)hipFree(h->p.rngage);
    (void)hipFree(h->p.py_top); (void)hipFree(h->p.np_hit); (void)hipFree(h->p.np_nib);
    (void)hipFree(h->sync);
    (void)hipFree(h->shadow.grid); (void)hipFree(h->shadow.pos); (void)hipFree(h->shadow.key); (void)hipFree(h->shadow.images);
    if (h->hio_host) (void)hipHostFree(h->hio_host);
    delete h;
}

extern "C" int ctf_create(const ctf_config* cfg, int32_t n_envs, int32_t device_id, ctf_env** out) {
    if (!cfg || !out) return fail(CTF_E_INVALID, "null argument");
    *out = nullptr;
    DevCfg d;
    int rc = derive(cfg, n_envs, &d);
    if (rc) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(CTF_E_INVALID, "device %d of %d", device_id, ndev);
    DeviceScope guard(device_id);
    if (guard.error) return fail(CTF_E_HIP, "hipSetDevice(%d) failed", device_id);
    ctf_env* h = new (std::nothrow) ctf_env();
    if (!h) return fail(CTF_E_NOMEM, "host allocation failed");
    memset(&h->p, 0, sizeof(h->p));
    h->seed_scratch = nullptr;
    h->rng_scratch = nullptr;
    h->hio_dev = nullptr;
    h->hio_host = nullptr;
    h->sync = nullptr;
    h->retained = nullptr;
    h->shadow = ObsShadow{nullptr, nullptr, nullptr, nullptr};
    h->delta_nt = -1;
    h->delta_bitmap = 0;
    h->delta_flags = 0u;
    {
        const char* ov = getenv("CTF_OBS_NT");
        h->nt_override = ov ? (atoi(ov) != 0) : -1;
    }
    h->cfg = *cfg; h->d = d; h->device = device_id;
    h->fingerprint = snap_fingerprint(cfg, d);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) { free_all(h); return fail(CTF_E_HIP, "hipGetDeviceProperties failed"); }
    h->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->d.n_cus = d.n_cus = h->n_cus;
    {
        int khz = 0;  // the wall clock's rate (100 MHz on CDNA3 / CDNA4)
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_id) != hipSuccess || khz <= 0) khz = 100000;
        h->spin_ticks = (uint64_t)khz * 10;
    }
    const size_t E = (size_t)n_envs;
    const size_t vis_elems = d.log_metrics ? E * d.N * d.GS : 1, met_elems = d.log_metrics ? E * CTF_N_METRICS * d.N : 1;
#define ALLOC(ptr, bytes)                                                                                      \
    if (hipMalloc((void**)&(ptr), (bytes)) != hipSuccess) { free_all(h); return fail(CTF_E_NOMEM, "hipMalloc(%zu) failed", (size_t)(bytes)); }
    ALLOC(h->p.grid, E * d.GS);
    ALLOC(h->p.rec, E * d.RS);
    const bool direct = d.rng_mode == CTF_RNG_COUNTER_DIRECT;  // no rings, digests, positions or flags: placeholders that nothing touches
    const size_t RE = direct ? 0 : E;                          // envs that own rings
    ALLOC(h->p.mt_py, RE ? RE * 2 * CTF_MT_N * 4 : 4);
    ALLOC(h->p.mt_np, RE ? RE * 2 * CTF_MT_N * 4 : 4);
    ALLOC(h->p.py_top, RE ? RE * 2 * CTF_P8_DW * 4 : 4);
    ALLOC(h->p.np_hit, RE ? RE * 2 * CTF_HB_DW * 4 : 4);
    ALLOC(h->p.np_nib, RE ? RE * 2 * CTF_NB_DW * 4 : 4);
    ALLOC(h->p.rngpos, RE ? RE * 2 * 4 : 4);
    ALLOC(h->p.rngready, RE ? RE * 2 : 1);
    ALLOC(h->p.rngage, RE ? RE * 2 : 1);
    ALLOC(h->p.rngctr, (d.rng_mode == CTF_RNG_COUNTER ? E * 6 : (direct ? E * 4 : 1)) * 8);
    ALLOC(h->rng_scratch, 2 * (CTF_MT_N + 1) * 4);
    ALLOC(h->p.metrics, met_elems * 4);
    ALLOC(h->p.vis, vis_elems * 4);
    ALLOC(h->p.vislog, (d.log_metrics ? (size_t)CTF_VIS_LOG * E * d.N : 1) * 2);
    ALLOC(h->p.init_grid, (size_t)d.GS);
    ALLOC(h->p.meta_lut, (size_t)round_up(d.N * d.M, 16));
    ALLOC(h->p.status, 4);
    ALLOC(h->seed_scratch, E * 2 * 8);
    ALLOC(h->sync, ctf_sync_words(n_envs) * 4);
#undef ALLOC
    std::vector<uint8_t> g0((size_t)d.GS, 0);
    memcpy(g0.data(), cfg->init_grid, (size_t)d.GG);
    hipError_t e1 = hipMemcpy((void*)h->p.init_grid, g0.data(), (size_t)d.GS, hipMemcpyHostToDevice);
    std::vector<uint8_t> lut((size_t)round_up(d.N * d.M, 16), 41);
    host_meta_lut(d, lut.data());
    if (hipMemcpy((void*)h->p.meta_lut, lut.data(), lut.size(), hipMemcpyHostToDevice) != hipSuccess) { free_all(h); return fail(CTF_E_HIP, "device initialisation failed"); }
    hipError_t e2 = hipMemset(h->p.status, 0, 4);
    hipError_t e3 = hipMemset(h->p.rec, 0, E * d.RS);
    if (e3 == hipSuccess) e3 = hipMemset(h->sync, 0, ctf_sync_words(n_envs) * 4);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) { free_all(h); return fail(CTF_E_HIP, "device initialisation failed"); }
    // first reset (+ _arr = [0..N-1], gridworld_ctf.py:244) and seeds 0/0
    hipError_t e4 = ctf_launch_reset(h->d, h->p, nullptr, 1, nullptr);
    hipError_t e5 = hipMemset(h->seed_scratch, 0, E * 2 * 8);
    hipError_t e6 = ctf_launch_seed(h->d, h->p, h->seed_scratch, h->seed_scratch + E, nullptr);
    if (e6 == hipSuccess && !direct) e6 = ctf_launch_rng_refill(h->d, h->p, 0, n_envs, 1, nullptr);
    if (e6 == hipSuccess && !direct) e6 = hipMemset(h->p.rngage, 0, E * 2);  // (a seed / state import leaves every ring in place: the ages go back to 0 by themselves, tail_block)
    hipError_t e7 = hipDeviceSynchronize();
    if (e4 != hipSuccess || e5 != hipSuccess || e6 != hipSuccess || e7 != hipSuccess) {
        const hipError_t bad = e4 != hipSuccess ? e4 : e5 != hipSuccess ? e5 : e6 != hipSuccess ? e6 : e7;
        free_all(h);
        return fail(CTF_E_HIP, "first reset/seed failed: %s", hipGetErrorString(bad));
    }
    if (device_id >= 0 && device_id < CTF_MAX_DEVICES) g_obs_bytes[device_id].fetch_add(obs_total(h), std::memory_order_relaxed);
    *out = h;
    return CTF_OK;
}

extern "C" void ctf_destroy(ctf_env* h) {
    if (!h) return;
    if (h->device >= 0 && h->device < CTF_MAX_DEVICES) g_obs_bytes[h->device].fetch_sub(obs_total(h), std::memory_order_relaxed);
    DeviceScope guard(h->device);
    (void)hipDeviceSynchronize();
    free_all(h);
}

extern "C" int32_t ctf_n_envs(const ctf_env* h) { return h ? h->d.n_envs : 0; }
extern "C" int64_t ctf_obs_bytes_per_env(const ctf_env* h) { return h ? h->d.obs_bytes : 0; }
extern "C" int64_t ctf_meta_elems_per_env(const ctf_env* h) { return h ? (int64_t)h->d.N * h->d.M : 0; }
extern "C" const char* ctf_last_error(void) { return g_err; }
extern "C" int32_t ctf_abi_version(void) { return CTF_ABI_VERSION; }
extern "C" int32_t ctf_sizeof_config(void) { return (int32_t)sizeof(ctf_config); }
extern "C" int32_t ctf_sizeof_state_view(void) { return (int32_t)sizeof(ctf_state_view); }

extern "C" int ctf_seed(ctf_env* h, const uint64_t* py_seeds, const uint64_t* np_seeds, void* stream) {
    if (!h || !py_seeds || !np_seeds) return fail(CTF_E_INVALID, "null argument");
    DeviceScope guard(h->device);
    const size_t E = (size_t)h->d.n_envs;
    if (h->d.rng_mode == CTF_RNG_MT19937)
        for (size_t e = 0; e < E; e++)
            if (np_seeds[e] >> 32) return fail(CTF_E_INVALID, "np seed %zu must be < 2**32 (np.random.seed's own limit)", e);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(h->seed_scratch, py_seeds, E * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->seed_scratch + E, np_seeds, E * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(ctf_launch_seed(h->d, h->p, h->seed_scratch, h->seed_scratch + E, st));
    if (h->d.rng_mode != CTF_RNG_COUNTER_DIRECT)
        HIP_TRY(ctf_launch_rng_refill(h->d, h->p, 0, h->d.n_envs, 1, st));  // the blocks after the seeded ones, and all digests
    HIP_TRY(hipStreamSynchronize(st));  // the host arrays are the caller's; do not outlive the call
    return CTF_OK;
}

// `modes`: bit m set = the entry point serves rng_mode m
static int need_mode(const ctf_env* h, unsigned modes, const char* what) {
    static const char* const names[3] = {"MT19937", "counter-RNG", "counter-direct-RNG"};
    if (!((modes >> h->d.rng_mode) & 1u)) return fail(CTF_E_INVALID, "%s: the handle runs in %s mode", what, names[h->d.rng_mode]);
    return CTF_OK;
}
#define MODE_MT (1u << CTF_RNG_MT19937)
#define MODE_COUNTERS ((1u << CTF_RNG_COUNTER) | (1u << CTF_RNG_COUNTER_DIRECT))

extern "C" int ctf_set_rng_state(ctf_env* h, int32_t e, const uint32_t* py, const uint32_t* np_) {
    if (!h) return fail(CTF_E_INVALID, "null handle");
    if (e < 0 || e >= h->d.n_envs) return fail(CTF_E_RANGE, "env index %d", e);
    if (int rc = need_mode(h, MODE_MT, "ctf_set_rng_state")) return rc;
    DeviceScope guard(h->device);
    HIP_TRY(hipDeviceSynchronize());
    const uint32_t* src[2] = {py, np_};
    uint32_t* dev[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; k++) {
        if (!src[k]) continue;
        if (src[k][CTF_MT_N] > CTF_MT_N) return fail(CTF_E_INVALID, "MT position %u > 624", src[k][CTF_MT_N]);
        dev[k] = h->rng_scratch + k * (CTF_MT_N + 1);
        HIP_TRY(hipMemcpy(dev[k], src[k], (CTF_MT_N + 1) * 4, hipMemcpyHostToDevice));
    }
    if (dev[0] || dev[1]) {
        // the two records are not adjacent when only one is given: one launch per generator
        if (dev[0]) HIP_TRY(ctf_launch_import_rng(h->d, h->p, dev[0], nullptr, e, 1, nullptr));
        if (dev[1]) HIP_TRY(ctf_launch_import_rng(h->d, h->p, nullptr, dev[1], e, 1, nullptr));
        // every ring of every env is brought up to date (envs other than e: whatever the last step left for the next launch's tail)
        HIP_TRY(ctf_launch_rng_refill(h->d, h->p, 0, h->d.n_envs, 0, nullptr));
        HIP_TRY(ctf_launch_rng_refill(h->d, h->p, e, 1, 1, nullptr));  // (a stream of env e that was not handed over is simply redone)
        HIP_TRY(hipDeviceSynchronize());
    }
    return CTF_OK;
}

extern "C" int ctf_get_rng_state(ctf_env* h, int32_t e, uint32_t* py, uint32_t* np_) {
    if (!h) return fail(CTF_E_INVALID, "null handle");
    if (e < 0 || e >= h->d.n_envs) return fail(CTF_E_RANGE, "env index %d", e);
    if (int rc = need_mode(h, MODE_MT, "ctf_get_rng_state")) return rc;
    DeviceScope guard(h->device);
    HIP_TRY(hipDeviceSynchronize());
    uint32_t* dst[2] = {py, np_};
    for (int k = 0; k < 2; k++) {
        if (!dst[k]) continue;
        uint32_t* dev = h->rng_scratch + k * (CTF_MT_N + 1);
        HIP_TRY(ctf_launch_export_rng(h->d, h->p, k == 0 ? dev : nullptr, k == 1 ? dev : nullptr, e, 1, nullptr));
        HIP_TRY(hipMemcpy(dst[k], dev, (CTF_MT_N + 1) * 4, hipMemcpyDeviceToHost));
    }
    return CTF_OK;
}

extern "C" int ctf_set_rng_states(ctf_env* h, const uint32_t* py_dev, const uint32_t* np_dev, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "null handle");
    if (!py_dev && !np_dev) return CTF_OK;
    if (int rc = need_mode(h, MODE_MT, "ctf_set_rng_states")) return rc;
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_import_rng(h->d, h->p, py_dev, np_dev, 0, h->d.n_envs, (hipStream_t)stream));
    HIP_TRY(ctf_launch_rng_refill(h->d, h->p, 0, h->d.n_envs, 1, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_get_rng_states(ctf_env* h, uint32_t* py_dev, uint32_t* np_dev, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "null handle");
    if (!py_dev && !np_dev) return CTF_OK;
    if (int rc = need_mode(h, MODE_MT, "ctf_get_rng_states")) return rc;
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_export_rng(h->d, h->p, py_dev, np_dev, 0, h->d.n_envs, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_get_rng_counters(ctf_env* h, uint64_t* counters_dev, void* stream) {
    if (!h || !counters_dev) return fail(CTF_E_INVALID, "null argument");
    if (int rc = need_mode(h, MODE_COUNTERS, "ctf_get_rng_counters")) return rc;
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_get_counters(h->d, h->p, (unsigned long long*)counters_dev, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_set_rng_counters(ctf_env* h, const uint64_t* counters_dev, void* stream) {
    if (!h || !counters_dev) return fail(CTF_E_INVALID, "null argument");
    if (int rc = need_mode(h, MODE_COUNTERS, "ctf_set_rng_counters")) return rc;
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_set_counters(h->d, h->p, (const unsigned long long*)counters_dev, (hipStream_t)stream));
    if (h->d.rng_mode == CTF_RNG_COUNTER) HIP_TRY(ctf_launch_rng_refill(h->d, h->p, 0, h->d.n_envs, 1, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_reset(ctf_env* h, const uint8_t* mask_dev, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "null handle");
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_reset(h->d, h->p, mask_dev, 0, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_step(ctf_env* h, const int8_t* actions, float* rw32, double* rw64, uint8_t* done, uint32_t flags, void* stream) {
    if (!h || !actions) return fail(CTF_E_INVALID, "null argument");
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_step(h->d, h->p, StepArgs{actions, rw32, rw64, done, flags}, 1, (hipStream_t)stream));
    return CTF_OK;
}

static uint32_t resolve_reverse(const ctf_env* h, uint32_t reverse_mask) {
    return reverse_mask == CTF_REVERSE_DEFAULT ? (uint32_t)h->d.default_reverse : (reverse_mask & ((1u << h->d.N) - 1u));
}
static RenderArgs render_args(const ctf_env* h, uint8_t* obs, uint16_t* meta, uint32_t reverse_mask) {
    return RenderArgs{obs, meta, resolve_reverse(h, reverse_mask), h->sync, h->spin_ticks};
}

// whether a render into `obs` is the delta render: the caller has retained exactly this buffer (pointer equality alone proves
// nothing about a buffer's contents — the opt-in does, and the shadow's keys on the device say what is known of them)
static bool retained_here(const ctf_env* h, const uint8_t* obs) { return obs && obs == h->retained; }

// The delta render's store hint: the full render's rule (hinted while the live handles' observations exceed 320 MB).  Measured at
// 65 536 arena envs, interleaved in one process: step + delta render 0.2227 ms hinted against 0.2249 ms plain, hinted ahead in
// every round (profiles/r11_retained_render.md); small batches keep their observations in the caches for their consumer as before.
static int delta_hint(const ctf_env* h) { return h->delta_nt >= 0 ? h->delta_nt : store_hint(h); }

// the metadata rows leave as 8-byte stores (obs_build_env): a caller's meta_dev is refused unless it is 8-byte aligned
static int meta_arg(const uint16_t* meta, const char* what) {
    if ((uintptr_t)meta % 8) return fail(CTF_E_INVALID, "%s: meta_dev must be 8-byte aligned", what);
    return CTF_OK;
}

extern "C" int ctf_observe(ctf_env* h, uint8_t* obs, uint16_t* meta, uint32_t reverse_mask, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "null handle");
    if (int rc = meta_arg(meta, "ctf_observe")) return rc;
    if (!obs && !meta) return CTF_OK;
    DeviceScope guard(h->device);
    if (retained_here(h, obs)) {
        HIP_TRY(ctf_launch_observe_delta(h->d, h->p, h->shadow, render_args(h, obs, meta, reverse_mask), delta_hint(h), h->delta_bitmap, h->delta_flags, (hipStream_t)stream));
        return CTF_OK;
    }
    h->d.obs_store_nt = store_hint(h);
    HIP_TRY(ctf_launch_observe(h->d, h->p, render_args(h, obs, meta, reverse_mask), h->n_cus, (hipStream_t)stream));
    return CTF_OK;
}

// ---- the retained observation buffer (include/ctf_env.h: ctf_obs_retain)
static bool retain_enabled() {  // CTF_OBS_RETAIN=0: ctf_obs_retain is a no-op (A/B runs, tests); read at every call
    const char* e = getenv("CTF_OBS_RETAIN");
    return !e || atoi(e) != 0;
}
extern "C" int ctf_obs_retain(ctf_env* h, uint8_t* obs, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "null handle");
    if (!retain_enabled()) return CTF_OK;
    DeviceScope guard(h->device);
    h->retained = nullptr;
    if (!obs || !ctf_observe_delta_applies(h->d, obs)) return CTF_OK;  // released / a block the delta render does not take
    {   // a stream that is being captured can neither be waited for nor allocate: the buffer stays the caller's (full renders)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return CTF_OK;
    }
    const size_t E = (size_t)h->d.n_envs;
    if (!h->shadow.key) {
        ObsShadow s{nullptr, nullptr, nullptr, nullptr};
        const size_t image_bytes = 16 * (size_t)obsc_image_dwords(h->d.CGG);  // four slot images per env
        if (hipMalloc((void**)&s.grid, E * h->d.GS) != hipSuccess || hipMalloc((void**)&s.pos, E * CTF_MAX_AGENTS * 2) != hipSuccess ||
            hipMalloc((void**)&s.key, E * 4) != hipSuccess || hipMalloc((void**)&s.images, E * image_bytes) != hipSuccess) {
            (void)hipFree(s.grid); (void)hipFree(s.pos); (void)hipFree(s.key); (void)hipFree(s.images);
            return fail(CTF_E_NOMEM, "ctf_obs_retain: hipMalloc of the shadow (%zu bytes) failed",
                        E * ((size_t)h->d.GS + CTF_MAX_AGENTS * 2 + 4 + image_bytes));
        }
        h->shadow = s;
    }
    {
        const char* ov = getenv("CTF_OBS_DELTA_NT");
        h->delta_nt = ov ? (atoi(ov) != 0) : -1;
        const char* bm = getenv("CTF_OBS_DELTA_BITMAP");
        h->delta_bitmap = bm && atoi(bm) != 0;
        const char* rb = getenv("CTF_OBS_DELTA_REBUILD");
        const char* ad = getenv("CTF_OBS_DELTA_ALL_DIRTY");
        h->delta_flags = (rb && atoi(rb) != 0 ? CTF_OBS_DELTA_F_REBUILD : 0u) | (ad && atoi(ad) != 0 ? CTF_OBS_DELTA_F_ALL_DIRTY : 0u);
    }
    // nothing is known about the buffer; the clear has landed before the call returns, so the first render may come on any stream
    HIP_TRY(ctf_launch_obs_key_clear(h->shadow, h->d.n_envs, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    h->retained = obs;
    return CTF_OK;
}
extern "C" int ctf_obs_invalidate(ctf_env* h, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "null handle");
    if (!h->shadow.key) return CTF_OK;  // never retained: nothing is known anyway
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_obs_key_clear(h->shadow, h->d.n_envs, (hipStream_t)stream));
    return CTF_OK;
}
extern "C" int32_t ctf_observe_retained(const ctf_env* h, const uint8_t* obs) {
    if (!h) return -1;
    return retained_here(h, obs) ? 1 : 0;
}

// A test hook, deliberately not in include/ctf_env.h: the shadow copied out device to device, stream-ordered — grid u8 [E][GS],
// pos u16 [E][CTF_MAX_AGENTS], key u32 [E], images u32 [E][4][obsc_image_dwords(CGG)]; NULL = not wanted.
// tests/test_gpu_delta_planted.py compares the shadow a handle has carried forward over its steps with one built afresh.
extern "C" int ctf_debug_obs_shadow(ctf_env* h, uint8_t* grid, uint16_t* pos, uint32_t* key, uint32_t* images, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "null handle");
    if (!h->shadow.key) return fail(CTF_E_INVALID, "ctf_debug_obs_shadow: no buffer was ever retained");
    DeviceScope guard(h->device);
    const size_t E = (size_t)h->d.n_envs;
    hipStream_t st = (hipStream_t)stream;
    if (grid) HIP_TRY(hipMemcpyAsync(grid, h->shadow.grid, E * h->d.GS, hipMemcpyDeviceToDevice, st));
    if (pos) HIP_TRY(hipMemcpyAsync(pos, h->shadow.pos, E * CTF_MAX_AGENTS * 2, hipMemcpyDeviceToDevice, st));
    if (key) HIP_TRY(hipMemcpyAsync(key, h->shadow.key, E * 4, hipMemcpyDeviceToDevice, st));
    if (images) HIP_TRY(hipMemcpyAsync(images, h->shadow.images, E * 16 * (size_t)obsc_image_dwords(h->d.CGG), hipMemcpyDeviceToDevice, st));
    return CTF_OK;
}

extern "C" int32_t ctf_observe_kernel(const ctf_env* h, const uint8_t* obs) {
    if (!h) return -1;
    return ctf_observe_uses_tiles(h->d, obs) ? 1 : 0;
}

extern "C" int32_t ctf_observe_stores_hinted(const ctf_env* h, const uint8_t* obs) {
    if (!h) return -1;
    return ctf_observe_uses_tiles(h->d, obs) && store_hint(h) ? 1 : 0;
}

extern "C" int ctf_observe_codes(ctf_env* h, uint8_t* codes, uint16_t* meta, uint16_t* selfcells, uint32_t reverse_mask, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "null handle");
    if (int rc = meta_arg(meta, "ctf_observe_codes")) return rc;
    if (!codes && !meta && !selfcells) return CTF_OK;
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_observe_codes(h->d, h->p, codes, meta, selfcells, resolve_reverse(h, reverse_mask), h->n_cus, (hipStream_t)stream));
    return CTF_OK;
}

// CTF_STEP_META=0: the two-launch ctf_step_observe leaves the metadata rows to its render (A/B runs, tests); read at every call
static bool step_meta_enabled() {
    const char* e = getenv("CTF_STEP_META");
    return !e || atoi(e) != 0;
}

extern "C" int ctf_step_observe(ctf_env* h, const int8_t* actions, float* rw32, double* rw64, uint8_t* done, uint8_t* obs,
                                uint16_t* meta, uint32_t reverse_mask, uint32_t flags, void* stream) {
    if (!h || !actions) return fail(CTF_E_INVALID, "null argument");
    if (int rc = meta_arg(meta, "ctf_step_observe")) return rc;  // before the step: a refused call changes nothing
    DeviceScope guard(h->device);
    // (The ring regeneration rides at the tail of the step launch.  Running it as a launch of its own on a second stream, beside
    // the render, was built and measured in round 3: the render lost more than the step kernel gained — 189-191 M against 198 M
    // env-steps/s, profiles/r03_side_stream_ablation.md.)
    if (ctf_step_observe_one_launch(h->d, obs)) {
        h->d.obs_store_nt = store_hint(h);
        HIP_TRY(ctf_launch_step_observe(h->d, h->p, StepArgs{actions, rw32, rw64, done, flags}, render_args(h, obs, meta, reverse_mask),
                                        (hipStream_t)stream));
        // (the explicit switch wins over retention: a full render the shadow knows nothing of, so its keys go)
        if (retained_here(h, obs)) HIP_TRY(ctf_launch_obs_key_clear(h->shadow, h->d.n_envs, (hipStream_t)stream));
        return CTF_OK;
    }
    // The metadata rows come from the step kernel, which holds every env's final record in LDS and makes the rows of a wave's envs
    // at once (ctf_meta.h); the render then runs without them — k_observe_delta as the instantiation that has none of their code —
    // and with obs == NULL there is no second launch at all.  CTF_STEP_META=0: the render makes them, as it always did.
    uint16_t* step_rows = step_meta_enabled() ? meta : nullptr;
    uint16_t* render_rows = step_rows ? nullptr : meta;
    StepArgs sa{actions, rw32, rw64, done, flags};
    sa.meta = step_rows;
    HIP_TRY(ctf_launch_step(h->d, h->p, sa, 1, (hipStream_t)stream));
    if (retained_here(h, obs)) {
        HIP_TRY(ctf_launch_observe_delta(h->d, h->p, h->shadow, render_args(h, obs, render_rows, reverse_mask), delta_hint(h), h->delta_bitmap, h->delta_flags, (hipStream_t)stream));
    } else if (obs || render_rows) {
        h->d.obs_store_nt = store_hint(h);
        HIP_TRY(ctf_launch_observe(h->d, h->p, render_args(h, obs, render_rows, reverse_mask), h->n_cus, (hipStream_t)stream));
    }
    return CTF_OK;
}

extern "C" int32_t ctf_step_observe_launches(const ctf_env* h, const uint8_t* obs) {
    if (!h) return -1;
    return ctf_step_observe_one_launch(h->d, obs) ? 1 : 2;
}

extern "C" int ctf_action_mask(const ctf_env* h, uint8_t* mask_host) {
    if (!h || !mask_host) return fail(CTF_E_INVALID, "null argument");
    static const int type_flag[4] = {1, 1, 0, 0};  // AGENT_TYPE_ACTION_MASK, gridworld_ctf.py:218-223
    for (int i = 0; i < h->d.N; i++)
        for (int a = 0; a < CTF_N_ACTIONS; a++) mask_host[i * CTF_N_ACTIONS + a] = (type_flag[h->d.type[i]] && a >= 5) ? 0 : 1;
    return CTF_OK;
}

extern "C" int ctf_get_state(ctf_env* h, int32_t e, ctf_state_view* out) {
    if (!h || !out) return fail(CTF_E_INVALID, "null argument");
    if (e < 0 || e >= h->d.n_envs) return fail(CTF_E_RANGE, "env index %d", e);
    DeviceScope guard(h->device);
    const DevCfg& d = h->d;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint8_t> rec((size_t)d.RS), grid((size_t)d.GS);
    HIP_TRY(hipMemcpy(grid.data(), h->p.grid + (size_t)e * d.GS, (size_t)d.GS, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rec.data(), h->p.rec + (size_t)e * d.RS, (size_t)d.RS, hipMemcpyDeviceToHost));
    std::vector<int32_t> m((size_t)CTF_N_METRICS * d.N);
    if (d.log_metrics) HIP_TRY(hipMemcpy(m.data(), h->p.metrics + (size_t)e * CTF_N_METRICS * d.N, m.size() * 4, hipMemcpyDeviceToHost));
    int32_t misc[4];
    sv_from_env(state_shape(d), rec.data(), grid.data(), d.log_metrics ? m.data() : nullptr, out, misc);
    if (d.log_metrics) {
        std::vector<uint32_t> v((size_t)d.N * d.GS, 0);
        if (!(misc[3] & CTF_F_BASE_ZERO))
            HIP_TRY(hipMemcpy(v.data(), h->p.vis + (size_t)e * d.N * d.GS, v.size() * 4, hipMemcpyDeviceToHost));
        // the env's whole log, so that the ONE walk (sv_visitation) indexes it by slot as it does ctf_host_step's; only the window's slots are filled, and read
        std::unique_ptr<uint16_t[]> ring(new uint16_t[(size_t)CTF_VIS_LOG * d.N]);
        const size_t pitch = (size_t)d.n_envs * d.N * 2, width = (size_t)d.N * 2;
        for (int r = 0, rows, count = sv_log_count(misc); r < count; r += rows) {  // at most two runs: the ring may wrap
            const int slot = sv_log_slot(misc, r);
            rows = std::min(count - r, CTF_VIS_LOG - slot);
            HIP_TRY(hipMemcpy2D(ring.get() + (size_t)slot * d.N, width, h->p.vislog + ((size_t)slot * d.n_envs + e) * d.N, pitch, width,
                                (size_t)rows, hipMemcpyDeviceToHost));
        }
        sv_visitation(state_shape(d), d.start_pos, misc, v.data(), ring.get(), (size_t)d.N, out);
    }
    return CTF_OK;
}

// ---- ctf_host_step: one env, host memory on both sides ------------------------------------------------------------------------
// Gathers what a host view of env 0 needs (grid, record, counters, visitation base maps and log) next to the step's outputs, so
// that ONE device-to-host copy brings everything back; reads and clears the sticky status word.
// py_out / np_out: also the two generators in the standard form (624 words of the current ring + the position: what k_export_rng
// writes), so that the hand-back needs no launch of its own.
__global__ void __launch_bounds__(256) k_host_pack(DevCfg d, DevPtrs p, uint8_t* io, HostIo L, uint32_t* py_out, uint32_t* np_out) {
    const int t = threadIdx.x;
    {
        uint32_t* dst[2] = {py_out, np_out};
        const uint32_t* src[2] = {p.mt_py, p.mt_np};
        for (int k = 0; k < 2; k++) {
            if (!dst[k]) continue;  // uniform
            const uint32_t rp = p.rngpos[k];
            const uint32_t* in = src[k] + (size_t)CTF_RP_CUR(rp) * CTF_MT_N;
            for (int i = t; i < CTF_MT_N; i += 256) dst[k][i] = in[i];
            if (t == 0) dst[k][CTF_MT_N] = CTF_RP_POS(rp);
        }
    }
    for (int k = t; k < d.GS; k += 256) io[L.grid + k] = p.grid[k];
    for (int k = t; k < d.RS; k += 256) io[L.rec + k] = p.rec[k];
    if (d.log_metrics) {
        uint32_t* m = (uint32_t*)(io + L.metrics);
        for (int k = t; k < CTF_N_METRICS * d.N; k += 256) m[k] = (uint32_t)p.metrics[k];
        uint32_t* v = (uint32_t*)(io + L.vis);
        for (int k = t; k < d.N * d.GS; k += 256) v[k] = p.vis[k];  // ALL N * GS words, in every call: ctf_host_step counts in them in place
        uint32_t* lg = (uint32_t*)(io + L.vislog);
        const uint32_t* src = (const uint32_t*)p.vislog;  // n_envs == 1: the ring [512][N] u16 is contiguous, N even or odd: 512 * N * 2 bytes
        for (int k = t; k < CTF_VIS_LOG * d.N / 2; k += 256) lg[k] = src[k];
    }
    if (t == 0) {
        uint32_t* ds = (uint32_t*)(io + L.done_status);
        ds[1] = *p.status;
        *p.status = 0;
    }
}

extern "C" int ctf_host_step(ctf_env* h, const int8_t* actions, const uint32_t* py_in, const uint32_t* np_in, uint32_t reverse_mask,
                             uint32_t flags, double* rewards, int32_t* done, uint32_t* status, ctf_state_view* view, uint32_t* py_out,
                             uint32_t* np_out, uint8_t* obs, uint16_t* meta, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "null handle");
    if (h->d.n_envs != 1) return fail(CTF_E_INVALID, "ctf_host_step serves a handle of ONE env (this one has %d): batches use ctf_step / ctf_observe", h->d.n_envs);
    const bool rng_io = py_in || np_in || py_out || np_out;
    if (rng_io)
        if (int rc = need_mode(h, MODE_MT, "ctf_host_step with generator states")) return rc;
    for (const uint32_t* s : {py_in, np_in})
        if (s && s[CTF_MT_N] > CTF_MT_N) return fail(CTF_E_INVALID, "MT position %u > 624", s[CTF_MT_N]);
    DeviceScope guard(h->device);
    const DevCfg& d = h->d;
    const HostIo L = host_io_layout(d);
    if (!h->hio_host) {
        // pinned, mapped, coherent host memory: the kernels below read their inputs from it and write their outputs into it across the
        // bus (a few KB in, ~50 KB out) — no copy operations in the stream; a kernel's stores are visible to the host when the stream
        // has been waited for
        void* dev = nullptr;
        if (hipHostMalloc((void**)&h->hio_host, L.end, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
            return fail(CTF_E_NOMEM, "hipHostMalloc(%zu) failed", L.end);
        if (hipHostGetDevicePointer(&dev, h->hio_host, 0) != hipSuccess) {
            (void)hipHostFree(h->hio_host);
            h->hio_host = nullptr;
            return fail(CTF_E_HIP, "hipHostGetDevicePointer failed");
        }
        h->hio_dev = (uint8_t*)dev;
        memset(h->hio_host, 0, L.end);
    }
    hipStream_t st = (hipStream_t)stream;
    uint8_t *hd = h->hio_dev, *hh = h->hio_host;
    // inputs: actions and the generator states to install (the previous call has waited for the stream: nothing reads the block now)
    if (actions) memcpy(hh + L.actions, actions, (size_t)d.N);
    if (py_in) memcpy(hh + L.py_in, py_in, (CTF_MT_N + 1) * 4);
    if (np_in) memcpy(hh + L.np_in, np_in, (CTF_MT_N + 1) * 4);
    if (py_in || np_in) {
        HIP_TRY(ctf_launch_import_rng(d, h->p, py_in ? (const uint32_t*)(hd + L.py_in) : nullptr,
                                      np_in ? (const uint32_t*)(hd + L.np_in) : nullptr, 0, 1, st));
        HIP_TRY(ctf_launch_rng_refill(d, h->p, 0, 1, 1, st));
    }
    if (actions)
        HIP_TRY(ctf_launch_step(d, h->p, StepArgs{(const int8_t*)(hd + L.actions), nullptr, (double*)(hd + L.rw64), hd + L.done_status, flags},
                                1, st));
    if (obs || meta)
        HIP_TRY(ctf_launch_observe(d, h->p, render_args(h, obs ? hd + L.obs : nullptr, meta ? (uint16_t*)(hd + L.meta) : nullptr, reverse_mask),
                                   h->n_cus, st));
    hipLaunchKernelGGL(k_host_pack, dim3(1), dim3(256), 0, st, d, h->p, hd, L, py_out ? (uint32_t*)(hd + L.py_out) : nullptr,
                       np_out ? (uint32_t*)(hd + L.np_out) : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));  // the only wait of the call: every output already lies in host memory
    if (rewards && actions) memcpy(rewards, hh + L.rw64, (size_t)d.N * 8);
    const uint32_t* ds = (const uint32_t*)(hh + L.done_status);
    if (status) *status = ds[1];
    if (py_out) memcpy(py_out, hh + L.py_out, (CTF_MT_N + 1) * 4);
    if (np_out) memcpy(np_out, hh + L.np_out, (CTF_MT_N + 1) * 4);
    if (obs) memcpy(obs, hh + L.obs, (size_t)d.obs_bytes);
    if (meta) memcpy(meta, hh + L.meta, (size_t)d.N * d.M * 2);
    int32_t misc[4];
    ctf_state_view local;
    ctf_state_view* out = view ? view : &local;
    sv_from_env(state_shape(d), hh + L.rec, hh + L.grid, d.log_metrics ? (const int32_t*)(hh + L.metrics) : nullptr, out, misc);
    if (done) *done = out->done;
    if (view && d.log_metrics) {  // (the block's base maps become the counts in place: k_host_pack writes them afresh in every call)
        sv_visitation(state_shape(d), d.start_pos, misc, (uint32_t*)(hh + L.vis), (const uint16_t*)(hh + L.vislog), (size_t)d.N, out);
    }
    return CTF_OK;
}

// the text of a view's refusal: the first value, in the view's order, that breaks one of ctf_states.h's rules
static int refused_view(const DevCfg& d, const ctf_state_view* in) {
    for (int i = 0; i < d.N; i++) {
        if (!st_ok_coord(in->pos[i][0], d.G) || !st_ok_coord(in->pos[i][1], d.G)) return fail(CTF_E_INVALID, "pos[%d] outside the grid", i);
        if (!st_ok_perm(in->perm[i], d.N)) return fail(CTF_E_INVALID, "perm[%d]", i);
        if (!st_ok_inventory(in->inventory[i])) return fail(CTF_E_INVALID, "inventory[%d]", i);
    }
    for (int k = 0; k < d.GG; k++) if (!st_ok_tile(in->grid[k])) return fail(CTF_E_INVALID, "grid[%d]", k);
    return st_ok_step(in->step_count) ? fail(CTF_E_INVALID, "invalid view") : fail(CTF_E_INVALID, "step_count %d", in->step_count);
}

extern "C" int ctf_set_state(ctf_env* h, int32_t e, const ctf_state_view* in) {
    if (!h || !in) return fail(CTF_E_INVALID, "null argument");
    if (e < 0 || e >= h->d.n_envs) return fail(CTF_E_RANGE, "env index %d", e);
    DeviceScope guard(h->device);
    const DevCfg& d = h->d;
    std::vector<uint8_t> rec((size_t)d.RS), grid((size_t)d.GS);
    std::vector<int32_t> m(d.log_metrics ? (size_t)CTF_N_METRICS * d.N : 0);
    std::vector<uint32_t> v(d.log_metrics ? (size_t)d.N * d.GS : 0);
    if (!sv_to_env(state_shape(d), in, rec.data(), grid.data(), d.log_metrics ? m.data() : nullptr, d.log_metrics ? v.data() : nullptr))
        return refused_view(d, in);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h->p.grid + (size_t)e * d.GS, grid.data(), (size_t)d.GS, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->p.rec + (size_t)e * d.RS, rec.data(), (size_t)d.RS, hipMemcpyHostToDevice));
    if (d.log_metrics) {
        HIP_TRY(hipMemcpy(h->p.metrics + (size_t)e * CTF_N_METRICS * d.N, m.data(), m.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->p.vis + (size_t)e * d.N * d.GS, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    }
    return CTF_OK;
}

extern "C" int ctf_export_counters(ctf_env* h, int32_t* metrics_dev, int32_t* captures_dev, int32_t* steps_dev, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "null handle");
    if (!metrics_dev && !captures_dev && !steps_dev) return CTF_OK;
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_export_counters(h->d, h->p, metrics_dev, captures_dev, steps_dev, (hipStream_t)stream));
    return CTF_OK;
}

// ---- snapshot records (ctf_snapshot.h / ctf_snapshot.hip) ----------------------------------------------------------------------
extern "C" int64_t ctf_snapshot_bytes(const ctf_env* h) { return h ? snap_layout(h->d, h->p, h->fingerprint).bytes : 0; }
extern "C" uint64_t ctf_snapshot_fingerprint(const ctf_env* h) { return h ? h->fingerprint : 0; }

static int snap_args(const ctf_env* h, int32_t n, const void* buf, const char* what) {
    if (!h || !buf) return fail(CTF_E_INVALID, "%s: null argument", what);
    if (n < 0) return fail(CTF_E_INVALID, "%s: n = %d", what, n);
    if ((uintptr_t)buf % 16) return fail(CTF_E_INVALID, "%s: the record buffer must be 16-byte aligned", what);
    return CTF_OK;
}

extern "C" int ctf_save_states(ctf_env* h, const int32_t* src_idx, int32_t n, uint8_t* dst, void* stream) {
    if (int rc = snap_args(h, n, dst, "ctf_save_states")) return rc;
    if (!src_idx && n > h->d.n_envs) return fail(CTF_E_RANGE, "ctf_save_states: n = %d > %d envs", n, h->d.n_envs);
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_save_states(snap_layout(h->d, h->p, h->fingerprint), src_idx, n, dst, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_load_states(ctf_env* h, const uint8_t* src, const int32_t* dst_idx, int32_t n, void* stream) {
    if (int rc = snap_args(h, n, src, "ctf_load_states")) return rc;
    if (n > h->d.n_envs) return fail(CTF_E_RANGE, "ctf_load_states: n = %d > %d envs", n, h->d.n_envs);
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_load_states(snap_layout(h->d, h->p, h->fingerprint), src, dst_idx, n, (hipStream_t)stream));
    return CTF_OK;
}

// ---- episode harvest (ctf_harvest.h / ctf_harvest.hip) -------------------------------------------------------------------------
extern "C" int32_t ctf_harvest_words(const ctf_env* h) { return h ? harvest_words(h->d.N) : 0; }

extern "C" int ctf_harvest_episodes(ctf_env* h, const int32_t* group_dev, int32_t n_groups, const uint8_t* env_mask_dev, uint32_t flags,
                                    int64_t* acc_dev, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "ctf_harvest_episodes: null handle");
    if (n_groups < 1) return fail(CTF_E_INVALID, "ctf_harvest_episodes: n_groups = %d", n_groups);
    if (!acc_dev) return fail(CTF_E_INVALID, "ctf_harvest_episodes: null table");
    if ((uintptr_t)acc_dev % 8) return fail(CTF_E_INVALID, "ctf_harvest_episodes: the table must be 8-byte aligned");
    if (flags & ~CTF_HARVEST_ALL) return fail(CTF_E_INVALID, "ctf_harvest_episodes: unknown flags 0x%x", flags);
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_harvest(harvest_args(h->d, h->p), group_dev, n_groups, env_mask_dev, flags, acc_dev, (hipStream_t)stream));
    return CTF_OK;
}

// ---- visitation maps (ctf_visitation.h / ctf_visitation.hip) --------------------------------------------------------------------
extern "C" int32_t ctf_visitation_words(const ctf_env* h) { return h ? visitation_words(h->d) : 0; }

extern "C" int ctf_harvest_visitation(ctf_env* h, const int32_t* group_dev, int32_t n_groups, const uint8_t* env_mask_dev, uint32_t flags,
                                      int64_t* acc_dev, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "ctf_harvest_visitation: null handle");
    if (!h->d.log_metrics) return fail(CTF_E_INVALID, "ctf_harvest_visitation: the handle keeps no visitation maps (log_metrics == 0)");
    if (n_groups < 1) return fail(CTF_E_INVALID, "ctf_harvest_visitation: n_groups = %d", n_groups);
    if (!acc_dev) return fail(CTF_E_INVALID, "ctf_harvest_visitation: null table");
    if ((uintptr_t)acc_dev % 8) return fail(CTF_E_INVALID, "ctf_harvest_visitation: the table must be 8-byte aligned");
    if (flags & ~CTF_HARVEST_ALL) return fail(CTF_E_INVALID, "ctf_harvest_visitation: unknown flags 0x%x", flags);
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_visit_harvest(visit_args(h->d, h->p), group_dev, n_groups, env_mask_dev, flags, acc_dev, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_export_visitation(ctf_env* h, const int32_t* idx_dev, int32_t n, uint32_t* out_dev, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "ctf_export_visitation: null handle");
    if (!h->d.log_metrics) return fail(CTF_E_INVALID, "ctf_export_visitation: the handle keeps no visitation maps (log_metrics == 0)");
    if (n < 0) return fail(CTF_E_INVALID, "ctf_export_visitation: n = %d", n);
    if (!idx_dev && n > h->d.n_envs) return fail(CTF_E_INVALID, "ctf_export_visitation: n = %d > %d envs", n, h->d.n_envs);
    if (!out_dev && n > 0) return fail(CTF_E_INVALID, "ctf_export_visitation: null output");
    if ((uintptr_t)out_dev % 4) return fail(CTF_E_INVALID, "ctf_export_visitation: the output must be 4-byte aligned");
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_visit_export(visit_args(h->d, h->p), idx_dev, n, out_dev, (hipStream_t)stream));
    return CTF_OK;
}

// ---- env states as plain arrays (ctf_states.h / ctf_states.hip) -------------------------------------------------------------------
static const char* const k_state_names[ST_FIELDS] = {"grid", "pos", "hp", "has_flag", "inventory", "perm", "step_count", "team_captures", "done",
                                                     "metrics", "visitation"};
static int state_args(const ctf_env* h, const ctf_state_arrays* a, int32_t n, bool have_idx, const char* what, StateArrays* out) {
    if (!h || !a) return fail(CTF_E_INVALID, "%s: null argument", what);
    if (n < 0) return fail(CTF_E_INVALID, "%s: n = %d", what, n);
    if (!have_idx && n > h->d.n_envs) return fail(CTF_E_INVALID, "%s: n = %d > %d envs", what, n, h->d.n_envs);
    uint8_t* const ptrs[ST_FIELDS] = {a->grid, (uint8_t*)a->pos, (uint8_t*)a->hp, a->has_flag, (uint8_t*)a->inventory, a->perm, (uint8_t*)a->step_count,
                                      (uint8_t*)a->team_captures, a->done, (uint8_t*)a->metrics, a->visitation};
    for (int f = 0; f < ST_FIELDS; f++) {
        if ((uintptr_t)ptrs[f] % 16) return fail(CTF_E_INVALID, "%s: %s must be 16-byte aligned", what, k_state_names[f]);
        out->arr[f] = ptrs[f];
    }
    if (a->metrics && !h->d.log_metrics) return fail(CTF_E_INVALID, "%s: metrics on a handle that keeps no counters (log_metrics == 0)", what);
    return CTF_OK;
}

extern "C" int ctf_export_states(ctf_env* h, const int32_t* idx_dev, int32_t n, const ctf_state_arrays* out, void* stream) {
    StateArrays A;
    if (int rc = state_args(h, out, n, idx_dev != nullptr, "ctf_export_states", &A)) return rc;
    if (out->visitation) return fail(CTF_E_INVALID, "ctf_export_states: visitation must be NULL (ctf_export_visitation exports the maps)");
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_export_states(state_shape(h->d), state_dev(h->d, h->p), idx_dev, n, A, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_import_states(ctf_env* h, const ctf_state_arrays* in, const int32_t* idx_dev, int32_t n, void* stream) {
    StateArrays A;
    if (int rc = state_args(h, in, n, false, "ctf_import_states", &A)) return rc;
    for (int f = 0; f < ST_METRICS; f++)
        if (!A.arr[f]) return fail(CTF_E_INVALID, "ctf_import_states: %s is required", k_state_names[f]);
    if (in->visitation && !h->d.log_metrics) return fail(CTF_E_INVALID, "ctf_import_states: visitation on a handle that keeps no maps (log_metrics == 0)");
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_import_states(state_shape(h->d), state_dev(h->d, h->p), A, idx_dev, n, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_status(ctf_env* h, uint32_t* out_bits, void* stream) {
    if (!h || !out_bits) return fail(CTF_E_INVALID, "null argument");
    DeviceScope guard(h->device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(out_bits, h->p.status, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemsetAsync(h->p.status, 0, 4, st));
    HIP_TRY(hipStreamSynchronize(st));
    return CTF_OK;
}

extern "C" int ctf_random_actions(ctf_env* h, int8_t* actions, uint64_t seed, uint32_t step, uint32_t env_offset, void* stream) {
    if (!h || !actions) return fail(CTF_E_INVALID, "null argument");
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_random_actions(h->d, actions, seed, step, env_offset, (hipStream_t)stream));
    return CTF_OK;
}

// ---- scripted opponents (ctf_scripted.h / ctf_scripted.hip) ----------------------------------------------------------------------
extern "C" int ctf_scripted_actions(ctf_env* h, int8_t* actions, uint32_t agent_mask, uint32_t kind, uint32_t epsilon_q32, uint64_t seed,
                                    uint32_t step, uint32_t env_offset, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "ctf_scripted_actions: null handle");
    if (!actions) return fail(CTF_E_INVALID, "ctf_scripted_actions: null actions");
    if (kind != CTF_SCRIPT_RUNNER) return fail(CTF_E_INVALID, "ctf_scripted_actions: unknown kind %u", kind);
    if (h->d.N < 32 && (agent_mask >> h->d.N)) return fail(CTF_E_INVALID, "ctf_scripted_actions: agent_mask 0x%x names an agent >= %d", agent_mask, h->d.N);
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_scripted_actions(script_args(h->d, h->p), actions, agent_mask, epsilon_q32, seed, step, env_offset, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_scripted_roles(ctf_env* h, int8_t* actions, uint32_t agent_mask, uint64_t role_pack, uint32_t epsilon_q32, uint64_t seed,
                                  uint32_t step, uint32_t env_offset, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "ctf_scripted_roles: null handle");
    if (!actions) return fail(CTF_E_INVALID, "ctf_scripted_roles: null actions");
    if (h->d.N < 32 && (agent_mask >> h->d.N)) return fail(CTF_E_INVALID, "ctf_scripted_roles: agent_mask 0x%x names an agent >= %d", agent_mask, h->d.N);
    for (int i = 0; i < 16; i++) {
        const uint32_t role = scr_role_of(role_pack, i);
        if (role > CTF_ROLE_GUARD) return fail(CTF_E_INVALID, "ctf_scripted_roles: unknown role %u of agent %d", role, i);
        if (role && i >= h->d.N) return fail(CTF_E_INVALID, "ctf_scripted_roles: a role for agent %d >= %d", i, h->d.N);
    }
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_scripted_roles(script_args(h->d, h->p), actions, agent_mask, role_pack, epsilon_q32, seed, step, env_offset, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_scripted_abilities(ctf_env* h, int8_t* actions, uint32_t agent_mask, uint64_t role_pack, uint32_t ability_mask, uint32_t epsilon_q32,
                                      uint64_t seed, uint32_t step, uint32_t env_offset, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "ctf_scripted_abilities: null handle");
    if (!actions) return fail(CTF_E_INVALID, "ctf_scripted_abilities: null actions");
    if (h->d.N < 32 && (agent_mask >> h->d.N)) return fail(CTF_E_INVALID, "ctf_scripted_abilities: agent_mask 0x%x names an agent >= %d", agent_mask, h->d.N);
    if (h->d.N < 32 && (ability_mask >> h->d.N))
        return fail(CTF_E_INVALID, "ctf_scripted_abilities: ability_mask 0x%x names an agent >= %d", ability_mask, h->d.N);
    for (int i = 0; i < 16; i++) {
        const uint32_t role = scr_role_of(role_pack, i);
        if (role > CTF_ROLE_GUARD) return fail(CTF_E_INVALID, "ctf_scripted_abilities: unknown role %u of agent %d", role, i);
        if (role && i >= h->d.N) return fail(CTF_E_INVALID, "ctf_scripted_abilities: a role for agent %d >= %d", i, h->d.N);
    }
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_scripted_abilities(script_args(h->d, h->p), script_abil(h->d), actions, agent_mask, role_pack, ability_mask, epsilon_q32, seed, step,
                                          env_offset, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_scripted_costs(ctf_env* h, int16_t* costs, uint32_t agent_mask, uint64_t role_pack, uint32_t ability_mask, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "ctf_scripted_costs: null handle");
    if (!costs) return fail(CTF_E_INVALID, "ctf_scripted_costs: null costs");
    if ((uintptr_t)costs & 1u) return fail(CTF_E_INVALID, "ctf_scripted_costs: costs is not 2-byte aligned");
    if (h->d.N < 32 && (agent_mask >> h->d.N)) return fail(CTF_E_INVALID, "ctf_scripted_costs: agent_mask 0x%x names an agent >= %d", agent_mask, h->d.N);
    if (h->d.N < 32 && (ability_mask >> h->d.N))
        return fail(CTF_E_INVALID, "ctf_scripted_costs: ability_mask 0x%x names an agent >= %d", ability_mask, h->d.N);
    for (int i = 0; i < 16; i++) {
        const uint32_t role = scr_role_of(role_pack, i);
        if (role > CTF_ROLE_GUARD) return fail(CTF_E_INVALID, "ctf_scripted_costs: unknown role %u of agent %d", role, i);
        if (role && i >= h->d.N) return fail(CTF_E_INVALID, "ctf_scripted_costs: a role for agent %d >= %d", i, h->d.N);
    }
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_scripted_costs(script_args(h->d, h->p), script_abil(h->d), costs, agent_mask, role_pack, ability_mask, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_action_effects(ctf_env* h, uint16_t* mask, uint8_t* effects, uint32_t agent_mask, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "ctf_action_effects: null handle");
    if (!mask && !effects) return fail(CTF_E_INVALID, "ctf_action_effects: both outputs are null");
    if ((uintptr_t)mask & 1u) return fail(CTF_E_INVALID, "ctf_action_effects: mask is not 2-byte aligned");
    if (h->d.N < 32 && (agent_mask >> h->d.N)) return fail(CTF_E_INVALID, "ctf_action_effects: agent_mask 0x%x names an agent >= %d", agent_mask, h->d.N);
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_action_effects(effect_args(h->d, h->p), mask, effects, agent_mask, (hipStream_t)stream));
    return CTF_OK;
}

extern "C" int ctf_random_effective_actions(ctf_env* h, int8_t* actions, uint32_t agent_mask, uint64_t seed, uint32_t step, uint32_t env_offset,
                                            void* stream) {
    if (!h) return fail(CTF_E_INVALID, "ctf_random_effective_actions: null handle");
    if (!actions) return fail(CTF_E_INVALID, "ctf_random_effective_actions: null actions");
    if (h->d.N < 32 && (agent_mask >> h->d.N))
        return fail(CTF_E_INVALID, "ctf_random_effective_actions: agent_mask 0x%x names an agent >= %d", agent_mask, h->d.N);
    DeviceScope guard(h->device);
    HIP_TRY(ctf_launch_random_effective(effect_args(h->d, h->p), actions, agent_mask, seed, step, env_offset, (hipStream_t)stream));
    return CTF_OK;
}

// ---- randomised episode starts (ctf_scatter.h / ctf_scatter.hip) -------------------------------------------------------------------
extern "C" int ctf_reset_scattered(ctf_env* h, const uint8_t* mask_dev, uint32_t agent_mask, int32_t radius, uint32_t flags, uint64_t seed, uint32_t round,
                                   uint32_t* episode_dev, uint32_t env_offset, void* stream) {
    if (!h) return fail(CTF_E_INVALID, "ctf_reset_scattered: null handle");
    if (radius < 0) return fail(CTF_E_INVALID, "ctf_reset_scattered: radius %d < 0", radius);
    if (h->d.N < 32 && (agent_mask >> h->d.N)) return fail(CTF_E_INVALID, "ctf_reset_scattered: agent_mask 0x%x names an agent >= %d", agent_mask, h->d.N);
    if (flags & ~CTF_SCATTER_OWN_SIDE) return fail(CTF_E_INVALID, "ctf_reset_scattered: unknown flags 0x%x", flags);
    if ((uintptr_t)episode_dev & 3u) return fail(CTF_E_INVALID, "ctf_reset_scattered: episode_dev is not 4-byte aligned");
    DeviceScope guard(h->device);
    const bool plain = radius == 0 || agent_mask == 0;  // nobody can move: ctf_reset's result
    if (plain && !episode_dev) HIP_TRY(ctf_launch_reset(h->d, h->p, mask_dev, 0, (hipStream_t)stream));
    else  // (k_reset knows no episode counter: the placement kernel with nobody asked writes the same bytes and advances it, in one launch)
        HIP_TRY(ctf_launch_reset_scattered(scatter_args(h->d, h->p), mask_dev, plain ? 0u : agent_mask, radius, flags, seed, round, episode_dev, env_offset,
                                           (hipStream_t)stream));
    return CTF_OK;
}
