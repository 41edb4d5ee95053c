// ctf_rng.hip — the random generators' kernels off the step's path: seeding, the bulk ring refill and the hand-over of the
// generator states.  (The per-step ring regeneration rides in k_step's tail blocks, ctf_kernels.hip; both use ctf_ring_dev.h.)
//
//   k_seed                           twin MT19937 seeding per env (CPython init_by_array / NumPy init_genrand), or the counter streams
//   k_rng_refill                     every stale ring of a range of envs, one wave per ring
//   k_import_rng / k_export_rng      the generators in their standard form (624 words + position)
//   k_get_counters / k_set_counters  the two counter modes: words consumed per stream
#include <hip/hip_runtime.h>

#include "ctf_launch.h"
#include "ctf_ring_dev.h"

// ------------------------------------------------------------------------------------------------
// seeding
// ------------------------------------------------------------------------------------------------
__device__ void mt_init_genrand(uint32_t* mt, uint32_t s) {
    mt[0] = s;
    uint32_t prev = s;
    for (int i = 1; i < CTF_MT_N; i++) {
        prev = 1812433253u * (prev ^ (prev >> 30)) + (uint32_t)i;
        mt[i] = prev;
    }
}
__device__ void mt_init_by_array(uint32_t* mt, const uint32_t* key, int len) {
    mt_init_genrand(mt, 19650218u);
    int i = 1, j = 0;
    uint32_t prev = mt[0];
    for (int k = CTF_MT_N > len ? CTF_MT_N : len; k; k--) {
        prev = (mt[i] ^ ((prev ^ (prev >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
        mt[i] = prev;
        i++; j++;
        if (i >= CTF_MT_N) { mt[0] = prev; i = 1; }
        if (j >= len) j = 0;
    }
    for (int k = CTF_MT_N - 1; k; k--) {
        prev = (mt[i] ^ ((prev ^ (prev >> 30)) * 1566083941u)) - (uint32_t)i;
        mt[i] = prev;
        i++;
        if (i >= CTF_MT_N) { mt[0] = prev; i = 1; }
    }
    mt[0] = 0x80000000u;
}

// py_seeds / np_seeds: device arrays [E].  After this (and the k_rng_refill(init) launch that follows it), env e ==
// random.seed(py) ; np.random.seed(np) (MT19937 mode: ring 0 = the seeded state, position 624, as CPython / NumPy hold it), or
// its two streams are the counter streams of these seeds at word 0 (counter mode).
extern "C" __global__ void k_seed(DevCfg cfg, DevPtrs p, const uint64_t* py_seeds, const uint64_t* np_seeds) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= cfg.n_envs) return;
    uint32_t* a_py = p.mt_py + (size_t)e * 2 * CTF_MT_N;
    uint32_t* a_np = p.mt_np + (size_t)e * 2 * CTF_MT_N;
    const uint64_t ps = py_seeds[e], ns = np_seeds[e];
    if (cfg.rng_mode == CTF_RNG_COUNTER_DIRECT) {  // both tapes at word 0: that is all there is (the rings are placeholders)
        unsigned long long* ctr = p.rngctr + 4 * (size_t)e;
        ctr[0] = 0; ctr[1] = 0; ctr[2] = ps; ctr[3] = ns;
        return;
    }
    if (cfg.rng_mode == CTF_RNG_COUNTER) {
        for (unsigned long long blk = 0; blk < CTF_MT_N / 4; blk++) {
            ctr_block(ps, blk, 0u, a_py + 4 * blk);
            ctr_block(ns, blk, 1u, a_np + 4 * blk);
        }
        unsigned long long* ctr = p.rngctr + 6 * (size_t)e;
        ctr[0] = 0; ctr[2] = 0; ctr[4] = ps; ctr[5] = ns;  // ring 0 of either stream starts at word 0
        p.rngpos[2 * e + 0] = CTF_RP_MAKE(0, 0);
        p.rngpos[2 * e + 1] = CTF_RP_MAKE(0, 0);
    } else {
        uint32_t key[2] = {(uint32_t)ps, (uint32_t)(ps >> 32)};
        mt_init_by_array(a_py, key, key[1] ? 2 : 1);
        mt_init_genrand(a_np, (uint32_t)ns);
        p.rngpos[2 * e + 0] = CTF_RP_MAKE(CTF_MT_N, 0);  // both generators start exhausted: the first draw comes from the next block
        p.rngpos[2 * e + 1] = CTF_RP_MAKE(CTF_MT_N, 0);
    }
}

// ------------------------------------------------------------------------------------------------
// the bulk ring refill (ctf_mt.h) and the hand-over of the generator states
// ------------------------------------------------------------------------------------------------
#define RNG_PAIRS_PER_WAVE 16  // (env, stream) pairs a wave looks after: their flags arrive in one load

// One wave per ring to regenerate: the ring the consumer has left becomes the block after the current one, with its digests, and
// the current ring is linked to it (mirror, hit bit of its last position).  Envs [e0, e0 + count).  `init`: every stream of
// the range is treated as not ready and the CURRENT ring's digests are made first (after a seed or a state import).
// Whole blocks, staged in LDS: 2.5 KB read, 2.5 KB + the digests written per ring, every access of a wave contiguous.
extern "C" __global__ void __launch_bounds__(256) k_rng_refill(DevCfg cfg, DevPtrs p, int e0, int count, int init) {
    __shared__ uint32_t sh[4][2 * CTF_MT_N];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    uint32_t* src = sh[wave];
    uint32_t* dst = src + CTF_MT_N;
    const int first = (blockIdx.x * 4 + wave) * RNG_PAIRS_PER_WAVE;  // pair t = env e0 + t / 2, stream t % 2
    if (first >= 2 * count) return;
    uint32_t flag = 1;
    if (lane < RNG_PAIRS_PER_WAVE && first + lane < 2 * count) flag = init ? 0u : p.rngready[2 * (size_t)e0 + first + lane];
    const bool todo = flag != 1u;
    unsigned long long work = __ballot(todo);
    while (work) {  // uniform
        const int k = __ffsll((long long)work) - 1;
        work &= work - 1;
        const int t = first + k, e = e0 + (t >> 1), stream = t & 1;
        refill_ring(cfg, p, e, stream, ring_fetch(cfg, p, e, stream, (uint32_t)__shfl((int)flag, k, WAVE), lane), lane, src, dst, init != 0);
    }
}

// Standard form per env and generator: 624 state words + the position (0..624), as random.getstate()[1] /
// np.random.get_state()[1:3] give them — which is what ring `cur` and the stream position ARE.  One block per env: block b
// handles env e0 + b and record b of the arrays.  An import is followed by k_rng_refill(init) over the same envs.
extern "C" __global__ void __launch_bounds__(256) k_import_rng(DevCfg cfg, DevPtrs p, const uint32_t* __restrict__ py,
                                                               const uint32_t* __restrict__ np_, int e0) {
    const int e = e0 + (int)blockIdx.x, t = threadIdx.x;
    const uint32_t* src[2] = {py, np_};
    uint32_t* dst[2] = {p.mt_py, p.mt_np};
    for (int k = 0; k < 2; k++) {
        if (!src[k]) continue;  // uniform
        const uint32_t* in = src[k] + (size_t)blockIdx.x * (CTF_MT_N + 1);
        uint32_t* out = dst[k] + (size_t)e * 2 * CTF_MT_N;
        for (int i = t; i < CTF_MT_N; i += blockDim.x) out[i] = in[i];
        if (t == 0) p.rngpos[2 * e + k] = CTF_RP_MAKE(in[CTF_MT_N] > CTF_MT_N ? CTF_MT_N : in[CTF_MT_N], 0);
    }
}
extern "C" __global__ void __launch_bounds__(256) k_export_rng(DevCfg cfg, DevPtrs p, uint32_t* __restrict__ py, uint32_t* __restrict__ np_, int e0) {
    const int e = e0 + (int)blockIdx.x, t = threadIdx.x;
    uint32_t* dst[2] = {py, np_};
    const uint32_t* src[2] = {p.mt_py, p.mt_np};
    for (int k = 0; k < 2; k++) {
        if (!dst[k]) continue;  // uniform
        const uint32_t rp = p.rngpos[2 * e + k];
        const uint32_t* in = src[k] + ((size_t)e * 2 + CTF_RP_CUR(rp)) * CTF_MT_N;
        uint32_t* out = dst[k] + (size_t)blockIdx.x * (CTF_MT_N + 1);
        for (int i = t; i < CTF_MT_N; i += blockDim.x) out[i] = in[i];
        if (t == 0) out[CTF_MT_N] = CTF_RP_POS(rp);
    }
}
// counter mode: (words consumed from the `random` stream, ... from the np.random stream) of every env
extern "C" __global__ void k_get_counters(DevCfg cfg, DevPtrs p, unsigned long long* out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= cfg.n_envs) return;
    if (cfg.rng_mode == CTF_RNG_COUNTER_DIRECT) {
        out[2 * (size_t)e] = p.rngctr[4 * (size_t)e];
        out[2 * (size_t)e + 1] = p.rngctr[4 * (size_t)e + 1];
        return;
    }
    for (int k = 0; k < 2; k++) {
        const uint32_t rp = p.rngpos[2 * e + k];
        out[2 * (size_t)e + k] = p.rngctr[6 * (size_t)e + 2 * k + CTF_RP_CUR(rp)] + CTF_RP_POS(rp);
    }
}
// ... and the way back (a checkpoint restore; followed by k_rng_refill(init)): ring 0 = the block that holds word n
extern "C" __global__ void k_set_counters(DevCfg cfg, DevPtrs p, const unsigned long long* in) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= cfg.n_envs) return;
    if (cfg.rng_mode == CTF_RNG_COUNTER_DIRECT) {
        p.rngctr[4 * (size_t)e] = in[2 * (size_t)e];
        p.rngctr[4 * (size_t)e + 1] = in[2 * (size_t)e + 1];
        return;
    }
    unsigned long long* ctr = p.rngctr + 6 * (size_t)e;
    for (int k = 0; k < 2; k++) {
        const unsigned long long n = in[2 * (size_t)e + k], blk = n / CTF_MT_N;
        ctr[2 * k] = blk * CTF_MT_N;
        uint32_t* a = (k ? p.mt_np : p.mt_py) + (size_t)e * 2 * CTF_MT_N;
        for (unsigned long long b = 0; b < CTF_MT_N / 4; b++) ctr_block(ctr[4 + k], blk * (CTF_MT_N / 4) + b, (uint32_t)k, a + 4 * b);
        p.rngpos[2 * e + k] = CTF_RP_MAKE((uint32_t)(n - blk * CTF_MT_N), 0);
    }
}

// ------------------------------------------------------------------------------------------------
// launchers (ctf_launch.h; called from ctf_abi.hip)
// ------------------------------------------------------------------------------------------------
extern "C" hipError_t ctf_launch_seed(const DevCfg& cfg, const DevPtrs& p, const uint64_t* py, const uint64_t* np_, hipStream_t st) {
    hipLaunchKernelGGL(k_seed, dim3((cfg.n_envs + 63) / 64), dim3(64), 0, st, cfg, p, py, np_);
    return hipGetLastError();
}
// envs [e0, e0 + count): record b of the arrays belongs to env e0 + b
extern "C" hipError_t ctf_launch_import_rng(const DevCfg& cfg, const DevPtrs& p, const uint32_t* py, const uint32_t* np_, int e0, int count,
                                            hipStream_t st) {
    hipLaunchKernelGGL(k_import_rng, dim3(count), dim3(256), 0, st, cfg, p, py, np_, e0);
    return hipGetLastError();
}
extern "C" hipError_t ctf_launch_export_rng(const DevCfg& cfg, const DevPtrs& p, uint32_t* py, uint32_t* np_, int e0, int count, hipStream_t st) {
    hipLaunchKernelGGL(k_export_rng, dim3(count), dim3(256), 0, st, cfg, p, py, np_, e0);
    return hipGetLastError();
}
extern "C" hipError_t ctf_launch_rng_refill(const DevCfg& cfg, const DevPtrs& p, int e0, int count, int init, hipStream_t st) {
    const int waves = (2 * count + RNG_PAIRS_PER_WAVE - 1) / RNG_PAIRS_PER_WAVE;
    hipLaunchKernelGGL(k_rng_refill, dim3((waves + 3) / 4), dim3(256), 0, st, cfg, p, e0, count, init);
    return hipGetLastError();
}
extern "C" hipError_t ctf_launch_get_counters(const DevCfg& cfg, const DevPtrs& p, unsigned long long* out, hipStream_t st) {
    hipLaunchKernelGGL(k_get_counters, dim3((cfg.n_envs + 63) / 64), dim3(64), 0, st, cfg, p, out);
    return hipGetLastError();
}
extern "C" hipError_t ctf_launch_set_counters(const DevCfg& cfg, const DevPtrs& p, const unsigned long long* in, hipStream_t st) {
    hipLaunchKernelGGL(k_set_counters, dim3((cfg.n_envs + 63) / 64), dim3(64), 0, st, cfg, p, in);
    return hipGetLastError();
}
