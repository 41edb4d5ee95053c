// ctf_visitation.hip — visitation maps on the device (ctf_harvest_visitation, ctf_export_visitation; ctf_visitation.h defines the
// map of one env, the LDS histogram's cell type and its sizing): one core that adds the maps of a set of envs into an LDS
// histogram, and two sinks.
//
// A workgroup is ONE wave with a histogram u32 [tile_agents][G * G] in dynamic LDS.
// The core walks an env's log column — env_step_count - folded pieces of 2N bytes, E * 2N bytes apart — with a lane per (step,
// agent) pair, VS_UNROLL x 64 pairs in flight: every load is unconditional (a lane past the end reads the column's first slot and
// drops it: slot < 512, e < E, i < N, always inside the log) and only then come the LDS atomics.  The loop over the envs of the set
// is the INNER one: 64 consecutive envs' pieces of one slot are contiguous, so a lockstep run reads each cache line of the log
// while it is hot instead of once per env.
// Sink A, the harvest: the scan of k_harvest_* (a wave looks at VS_EPW consecutive envs: 16 misc bytes, mask byte, group id; ballot;
// no env taken — the common case — exits at once).  The taken envs are cut into RUNS that share a group id; a run is accumulated
// into the histogram and flushed, non-zero cells only, with 64-bit vector atomicAdds: a lockstep batch whose groups are runs of
// envs sends one histogram per wave, any other assignment gives the same integer sums with more flushes.
// Sink B, the export: one wave per listed env, coalesced u32 stores, no atomics.
// Plain C++ loads, LDS atomics and vector atomics only; env state is only read; the status bit is raised with a vector atomic OR.
#include <hip/hip_runtime.h>

#include "ctf_launch.h"
#include "ctf_visitation.h"

#define VS_WAVE 64
#ifndef VS_EPW
#define VS_EPW 32  // envs one wave scans (<= 64), as the episode harvest
#endif
#ifndef VS_UNROLL
#define VS_UNROLL 8  // wave-wide loads of log entries in flight together
#endif

extern __shared__ uint32_t vs_hist[];

// Adds the maps of agents [i0, i0 + tn) of the envs e0 + j, j in `seg`, into hist [tn][GG].  steps / misc3: lane j holds the
// words of env e0 + j (every lane the same words when the set is one env at e0, j = 0).
__device__ __forceinline__ void vs_accumulate(const VisitArgs& A, uint32_t* hist, int i0, int tn, unsigned long long seg, int e0, int lane,
                                              int32_t steps, int32_t misc3) {
    const int N = A.N, GG = A.GG;
    const size_t E = (size_t)A.n_envs;
    int maxc = 0;
    // base maps
    for (unsigned long long b = seg; b; b &= b - 1) {
        const int j = (int)__builtin_ctzll(b);
        const int32_t fl = __builtin_amdgcn_readlane(misc3, j);
        int cnt = __builtin_amdgcn_readlane(steps, j) - (fl >> CTF_F_FOLDED_SHIFT);
        cnt = cnt < 0 ? 0 : (cnt > CTF_VIS_LOG - 1 ? CTF_VIS_LOG - 1 : cnt);
        maxc = cnt > maxc ? cnt : maxc;
        if (fl & CTF_F_BASE_ZERO) {
            for (int a = 0; a < tn; a++)
                if (lane == a) atomicAdd(&hist[(size_t)a * GG + A.start_cell[i0 + a]], 1u);
        } else {
            const uint32_t* base = A.vis + ((size_t)(e0 + j) * N + (size_t)i0) * (size_t)A.GS;
            for (int a = 0; a < tn; a++)
                for (int c = lane; c < GG; c += VS_WAVE) {
                    const uint32_t v = base[(size_t)a * A.GS + c];
                    if (v) atomicAdd(&hist[(size_t)a * GG + c], v);
                }
        }
    }
    // the log: pair p = (entry r, agent i) of an env's column, r = 0 is step folded + 1
    const int items = maxc * N;
    for (int p0 = 0; p0 < items; p0 += VS_WAVE * VS_UNROLL) {
        int r[VS_UNROLL], i[VS_UNROLL];
#pragma unroll
        for (int u = 0; u < VS_UNROLL; u++) {
            const int p = p0 + u * VS_WAVE + lane;
            r[u] = p / N;
            i[u] = p - r[u] * N;
        }
        for (unsigned long long b = seg; b; b &= b - 1) {
            const int j = (int)__builtin_ctzll(b);
            const int32_t fl = __builtin_amdgcn_readlane(misc3, j);
            const int folded = fl >> CTF_F_FOLDED_SHIFT;
            int cnt = __builtin_amdgcn_readlane(steps, j) - folded;
            cnt = cnt < 0 ? 0 : (cnt > CTF_VIS_LOG - 1 ? CTF_VIS_LOG - 1 : cnt);
            const size_t e = (size_t)(e0 + j);
            uint16_t cell[VS_UNROLL];
#pragma unroll
            for (int u = 0; u < VS_UNROLL; u++) {
                const int rr = r[u] < cnt ? r[u] : 0;
                const size_t slot = (size_t)((folded + 1 + rr) & (CTF_VIS_LOG - 1));
                cell[u] = A.vislog[(slot * E + e) * (size_t)N + (size_t)i[u]];
            }
#pragma unroll
            for (int u = 0; u < VS_UNROLL; u++) {
                const int a = i[u] - i0;
                if (r[u] < cnt && a >= 0 && a < tn && (int)cell[u] < GG) atomicAdd(&hist[(size_t)a * GG + cell[u]], 1u);
            }
        }
    }
}

// the env's misc words: step count and flags
__device__ __forceinline__ void vs_misc(const VisitArgs& A, size_t e, int32_t& steps, int32_t& misc3) {
    const uint8_t* rec = A.rec + e * (size_t)A.RS + A.off_misc;
    if ((A.off_misc & 15) == 0) {  // uniform (RS is a multiple of 16)
        const int4 m = *(const int4*)rec;
        steps = m.x, misc3 = m.w;
    } else {
        const int32_t* m = (const int32_t*)rec;
        steps = m[0], misc3 = m[3];
    }
}

extern "C" __global__ void __launch_bounds__(VS_WAVE) k_visit_harvest(VisitArgs A, const int32_t* group, int n_groups, const uint8_t* mask,
                                                                      uint32_t flags, int64_t* acc) {
    const int lane = threadIdx.x;
    const int e0 = (int)blockIdx.x * VS_EPW;
    const int e = e0 + lane;
    const int N = A.N, GG = A.GG;

    // the scan: is this lane's env taken, and into which group (the rule of k_harvest_*)
    int32_t g = 0, steps = 0, misc3 = 0;
    bool take = false;
    if (lane < VS_EPW && e < A.n_envs) {
        const uint8_t on = mask ? mask[e] : (uint8_t)1;
        g = group ? group[e] : 0;
        vs_misc(A, (size_t)e, steps, misc3);
        take = on && ((flags & CTF_HARVEST_ALL) || ((misc3 & CTF_F_DONE) && steps == A.game_steps));
        if (take && (g < 0 || g >= n_groups)) {
            atomicOr(A.status, CTF_ST_BAD_GROUP);
            take = false;
        }
    }
    const unsigned long long todo = __ballot(take);
    if (!todo) return;

    for (int c = lane; c < A.tile_agents * GG; c += VS_WAVE) vs_hist[c] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < N; i0 += A.tile_agents) {
        const int tn = N - i0 < A.tile_agents ? N - i0 : A.tile_agents;
        unsigned long long rest = todo;
        while (rest) {
            // the next run: the taken envs, in env order, that share the first one's group id — cut before a cell could pass 2^32 - 1
            const int cur = __builtin_amdgcn_readlane(g, (int)__builtin_ctzll(rest));
            unsigned long long seg = 0, bound = 0;
            for (unsigned long long t = rest; t; t &= t - 1) {
                const int j = (int)__builtin_ctzll(t);
                if (__builtin_amdgcn_readlane(g, j) != cur) break;
                const unsigned long long need = 256ull + (unsigned long long)(uint32_t)__builtin_amdgcn_readlane(steps, j);
                if (seg && bound + need > 0xFFFFFFFFull) break;
                seg |= 1ull << j;
                bound += need;
            }
            rest &= ~seg;
            vs_accumulate(A, vs_hist, i0, tn, seg, e0, lane, steps, misc3);
            __syncthreads();
            int64_t* row = acc + ((size_t)cur * N + (size_t)i0) * (size_t)GG;
            for (int c = lane; c < tn * GG; c += VS_WAVE) {
                const uint32_t v = vs_hist[c];
                if (v) {
                    atomicAdd((unsigned long long*)(row + c), (unsigned long long)v);
                    vs_hist[c] = 0;
                }
            }
            __syncthreads();
        }
    }
}

extern "C" __global__ void __launch_bounds__(VS_WAVE) k_visit_export(VisitArgs A, const int32_t* idx, int n, uint32_t* out) {
    const int lane = threadIdx.x;
    const int k = (int)blockIdx.x;
    const int N = A.N, GG = A.GG;
    if (k >= n) return;
    const int e = idx ? idx[k] : k;
    if (e < 0 || e >= A.n_envs) {
        if (lane == 0) atomicOr(A.status, CTF_ST_BAD_GROUP);
        return;
    }
    int32_t steps, misc3;
    vs_misc(A, (size_t)e, steps, misc3);  // every lane: the same words
    for (int c = lane; c < A.tile_agents * GG; c += VS_WAVE) vs_hist[c] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < N; i0 += A.tile_agents) {
        const int tn = N - i0 < A.tile_agents ? N - i0 : A.tile_agents;
        vs_accumulate(A, vs_hist, i0, tn, 1ull, e, lane, steps, misc3);
        __syncthreads();
        uint32_t* dst = out + ((size_t)k * N + (size_t)i0) * (size_t)GG;
        for (int c = lane; c < tn * GG; c += VS_WAVE) {
            dst[c] = vs_hist[c];
            vs_hist[c] = 0;
        }
        __syncthreads();
    }
}

extern "C" hipError_t ctf_launch_visit_harvest(const VisitArgs& A, const int32_t* group, int n_groups, const uint8_t* mask, uint32_t flags,
                                               int64_t* acc, hipStream_t st) {
    const int waves = (A.n_envs + VS_EPW - 1) / VS_EPW;
    hipLaunchKernelGGL(k_visit_harvest, dim3((unsigned)waves), dim3(VS_WAVE), visit_lds_bytes(A), st, A, group, n_groups, mask, flags, acc);
    return hipGetLastError();
}

extern "C" hipError_t ctf_launch_visit_export(const VisitArgs& A, const int32_t* idx, int n, uint32_t* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_visit_export, dim3((unsigned)n), dim3(VS_WAVE), visit_lds_bytes(A), st, A, idx, n, out);
    return hipGetLastError();
}
static_assert(VS_EPW <= VS_WAVE && CTF_VIS_LDS_CAP / 4 / CTF_MAX_CELLS >= 1, "a tile holds at least one agent's map");
