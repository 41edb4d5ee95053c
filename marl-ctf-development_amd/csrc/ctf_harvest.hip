// ctf_harvest.hip — the episode harvest (ctf_harvest_episodes, ctf_harvest.h has the row): one launch that finds the envs whose
// episode has just ended and adds their results into the caller's table of 64-bit accumulators, one row per group of envs.
//
// A wave scans HV_EPW consecutive envs, one per lane: the 16 misc bytes of the env's record (step count, both teams' captures,
// the done flag), its mask byte and its group id.  The ballot of the lanes whose env is taken is walked in env order, HV_BATCH
// envs at a time (then one at a time): the loads of the batch's contiguous metric[e] blocks (13 x N int32, lane l takes words
// l, l + 64, ...) are issued together, unconditionally (a lane past the end of the block reads the block's last word and drops
// it), then the envs are added one after the other into the wave's accumulator row, which lives in registers — lane l
// holds word l of the row's scalars (l < 7) and counter words l, l + 64, l + 128, l + 192 — for the wave's CURRENT group.  The row
// goes out with 64-bit vector atomicAdds (zero words skipped) when the group id changes and when the wave is done.  So the steady
// state (one env in GAME_STEPS ends per step) costs the scan plus a few dozen atomics per ended env, and a lockstep batch whose
// groups are runs of envs reads its counters once, coalesced, and sends one row per wave; any other assignment of group ids gives
// the same sums (integer additions: the order does not matter) with more flushes.  One kernel per count NR of counter words a lane
// holds (ceil(13 N / 64); 0 = log_metrics off), so that the batch's loads are straight-line code.  Env state is only read.  Plain C++ loads and
// vector atomics throughout; the status bit is raised with a vector atomic OR like every other one.
#include <hip/hip_runtime.h>

#include "ctf_harvest.h"
#include "ctf_launch.h"

#define HV_WAVE 64
#define HV_THREADS 256
#ifndef HV_EPW
#define HV_EPW 32   // envs one wave scans (<= 64): 2 048 waves at 65 536 envs, so that a lockstep batch keeps every CU reading
#endif
#ifndef HV_BATCH
#define HV_BATCH 8  // envs whose counter blocks are in flight together
#endif
#define HV_ROUNDS ((CTF_N_METRICS * CTF_MAX_AGENTS + HV_WAVE - 1) / HV_WAVE)  // counter words per lane

struct HvRow {
    int64_t head;            // lane l < CTF_HV_SCALARS: word l of the row
    int64_t ctr[HV_ROUNDS];  // counter words l + 64 r
};

__device__ __forceinline__ void hv_add(int64_t* dst, int64_t v) {
    if (v) atomicAdd((unsigned long long*)dst, (unsigned long long)v);
}

template <int NR>
__device__ __forceinline__ void hv_flush(int64_t* row, int lane, int MN, HvRow& a) {
    if (lane < CTF_HV_SCALARS) hv_add(row + lane, a.head);
    a.head = 0;
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const int w = lane + HV_WAVE * r;
        if (w < MN) hv_add(row + CTF_HV_HEAD + w, a.ctr[r]);
        a.ctr[r] = 0;
    }
}

// What the scan found, lane = env e0 + lane; the row being summed and the group it belongs to (-1: none yet).
struct HvWave {
    int32_t g, steps, c0, c1;
    HvRow a;
    int cur;
};

// B envs of `todo` (the lowest set bits: at least B are set), NR counter words per lane.  Every load is unconditional — a lane
// past the end of the block reads its last word and drops it — so the B x NR loads are in flight together.
template <int B, int NR>
__device__ __forceinline__ void hv_batch(const HarvestArgs& A, HvWave& s, unsigned long long& todo, int e0, int lane, int MN, int64_t* acc) {
    int j[B];
#pragma unroll
    for (int k = 0; k < B; k++) {
        j[k] = (int)__builtin_ctzll(todo);
        todo &= todo - 1;
    }
    int32_t v[B][NR > 0 ? NR : 1];
#pragma unroll
    for (int k = 0; k < B; k++) {
        const int32_t* m = A.metrics + (size_t)(e0 + j[k]) * MN;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int w = lane + HV_WAVE * r;
            const int32_t x = m[w < MN ? w : MN - 1];
            v[k][r] = w < MN ? x : 0;
        }
    }
#pragma unroll
    for (int k = 0; k < B; k++) {
        const int gk = __builtin_amdgcn_readlane(s.g, j[k]);
        const int32_t sk = __builtin_amdgcn_readlane(s.steps, j[k]);
        const int32_t ak = __builtin_amdgcn_readlane(s.c0, j[k]);
        const int32_t bk = __builtin_amdgcn_readlane(s.c1, j[k]);
        if (gk != s.cur) {
            if (s.cur >= 0) hv_flush<NR>(acc + (size_t)s.cur * (CTF_HV_HEAD + MN), lane, MN, s.a);
            s.cur = gk;
        }
        // this env's seven scalars, word `lane` of them
        int32_t h = 1;               // [0] episodes
        if (lane == 1) h = ak > bk;  // [1] team 0 wins
        if (lane == 2) h = ak == bk; // [2] draws
        if (lane == 3) h = ak < bk;  // [3] team 1 wins
        if (lane == 4) h = ak;       // [4] [5] captures
        if (lane == 5) h = bk;
        if (lane == 6) h = sk;       // [6] steps
        s.a.head += h;
#pragma unroll
        for (int r = 0; r < NR; r++) s.a.ctr[r] += v[k][r];
    }
}

// NR = counter words per lane = ceil(13 N / 64), 0 = no counters (log_metrics off)
template <int NR>
__device__ __forceinline__ void hv_kernel(const HarvestArgs& A, const int32_t* group, int n_groups, const uint8_t* mask, uint32_t flags,
                                          int64_t* acc) {
    const int lane = threadIdx.x & (HV_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (HV_THREADS / HV_WAVE) + threadIdx.x / HV_WAVE));
    const int e0 = wave * HV_EPW;
    const int e = e0 + lane;
    const int MN = CTF_N_METRICS * A.N;

    // the scan: is this lane's env taken, and into which group
    HvWave s;
    s.g = s.steps = s.c0 = s.c1 = 0;
    bool take = false;
    if (lane < HV_EPW && e < A.n_envs) {
        const uint8_t* rec = A.rec + (size_t)e * A.RS + A.off_misc;
        const uint8_t on = mask ? mask[e] : (uint8_t)1;
        s.g = group ? group[e] : 0;
        int32_t misc3;
        if ((A.off_misc & 15) == 0) {  // uniform (RS is a multiple of 16)
            const int4 m = *(const int4*)rec;
            s.steps = m.x, s.c0 = m.y, s.c1 = m.z, misc3 = m.w;
        } else {
            const int32_t* m = (const int32_t*)rec;
            s.steps = m[0], s.c0 = m[1], s.c1 = m[2], misc3 = m[3];
        }
        take = on && ((flags & CTF_HARVEST_ALL) || ((misc3 & CTF_F_DONE) && s.steps == A.game_steps));
        if (take && (s.g < 0 || s.g >= n_groups)) {
            atomicOr(A.status, CTF_ST_BAD_GROUP);
            take = false;
        }
    }
    unsigned long long todo = __ballot(take);
    if (!todo) return;

    s.a.head = 0;
#pragma unroll
    for (int r = 0; r < HV_ROUNDS; r++) s.a.ctr[r] = 0;
    s.cur = -1;
    while (__popcll(todo) >= HV_BATCH) hv_batch<HV_BATCH, NR>(A, s, todo, e0, lane, MN, acc);
    while (todo) hv_batch<1, NR>(A, s, todo, e0, lane, MN, acc);
    hv_flush<NR>(acc + (size_t)s.cur * (CTF_HV_HEAD + MN), lane, MN, s.a);
}

#define HV_KERNEL(NR)                                                                                                                      \
    extern "C" __global__ void __launch_bounds__(HV_THREADS) k_harvest_##NR(HarvestArgs A, const int32_t* group, int n_groups,             \
                                                                            const uint8_t* mask, uint32_t flags, int64_t* acc) {          \
        hv_kernel<NR>(A, group, n_groups, mask, flags, acc);                                                                               \
    }
HV_KERNEL(0)
HV_KERNEL(1)
HV_KERNEL(2)
HV_KERNEL(3)
HV_KERNEL(4)
static_assert(HV_ROUNDS == 4 && HV_EPW <= HV_WAVE, "one kernel per count of counter words a lane holds");

extern "C" hipError_t ctf_launch_harvest(const HarvestArgs& A, const int32_t* group, int n_groups, const uint8_t* mask, uint32_t flags,
                                         int64_t* acc, hipStream_t st) {
    const int waves = (A.n_envs + HV_EPW - 1) / HV_EPW;
    const int per_block = HV_THREADS / HV_WAVE;
    const int nr = A.metrics ? (CTF_N_METRICS * A.N + HV_WAVE - 1) / HV_WAVE : 0;
    void (*const kernels[HV_ROUNDS + 1])(HarvestArgs, const int32_t*, int, const uint8_t*, uint32_t, int64_t*) = {
        k_harvest_0, k_harvest_1, k_harvest_2, k_harvest_3, k_harvest_4};
    hipLaunchKernelGGL(kernels[nr], dim3((unsigned)((waves + per_block - 1) / per_block)), dim3(HV_THREADS), 0, st, A, group, n_groups, mask,
                       flags, acc);
    return hipGetLastError();
}
