// ctf_step_block.h — one STEP BLOCK of the step kernels: the wave stages its envs' grids, records and actions into LDS, every
// group runs group_step (ctf_step_core.h) and the wave writes the envs back.  Shared by k_step / k_step_observe (ctf_kernels.hip:
// the two ring modes, RNG = GroupRng<W>) and k_step_direct (ctf_step_direct.hip: CTF_RNG_COUNTER_DIRECT, RNG = GroupRngDirect).
// The including file defines STEP_STAMP (profiling builds) before it includes this.
#pragma once
#include <type_traits>

#include "ctf_ring_dev.h"  // WAVE, u32x4_t (and through it ctf_step_core.h)
#include "ctf_meta.h"      // the metadata rows a step block writes (META)
#include "ctf_launch.h"    // StepArgs

#ifndef STEP_STAMP
#define STEP_STAMP(k) do { } while (0)
#endif

#define STEP_LDS_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_s_waitcnt(0xC07F); \
        __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)


// ---- hand-off of a step block's envs to the render tiles of the same launch (k_step_observe).  The two usually sit on different
// XCDs, whose L2s are not coherent: the step block stores the grids and records write-through (agent-scope stores: `sc1`), waits
// for them (vmcnt(0)), then ONE lane stores the block's flag (agent scope); a tile polls the flag with agent-scope loads and reads
// the envs' grid and record with agent-scope loads only (`sc1`: served past this CU's L1 from a coherent level), so no acquire
// fence is needed.  The flags hold a generation number (StepSync), never a per-call launch argument: a captured launch replays.
typedef __attribute__((address_space(1))) uint32_t gu32_t;
typedef __attribute__((address_space(1))) unsigned long long gu64_t;
__device__ __forceinline__ uint32_t ld_sc1(const uint32_t* a) {
    return __hip_atomic_load((gu32_t*)(uint32_t*)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(uint32_t* a, uint32_t v) { __hip_atomic_store((gu32_t*)a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_sc1_x4(void* dst, u32x4_t v) {  // 16 bytes as two 8-byte write-through stores
    gu64_t* g = (gu64_t*)dst;
    __hip_atomic_store(g, (unsigned long long)v.x | ((unsigned long long)v.y << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(g + 1, (unsigned long long)v.z | ((unsigned long long)v.w << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
struct StepPub {
    uint32_t* flags;
    uint32_t value;  // seq + 1
};
__device__ __forceinline__ void step_publish(const StepPub& pub, int sb, int lane) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every write-through store of the block has landed
    if (lane == 0) st_sc1(pub.flags + sb, pub.value);
}

// where a step block's metadata rows go (META): f16 [E][N][M], and ctf_meta.h's reciprocal of an env's 8-byte chunks
struct StepMeta {
    uint16_t* out;
    uint32_t chunk_div;
};
static inline StepMeta step_meta(const DevCfg& cfg, const StepArgs& a) { return StepMeta{a.meta, a.meta ? meta_chunk_div(cfg.N, cfg.M) : 0u}; }

// The step of the EPW envs of step block sb (k_step, and the step blocks of k_step_observe).  PUBLISH (k_step_observe): the
// grids and records leave write-through and the block's flag follows them (StepPub).  DIRECT: the streams of
// CTF_RNG_COUNTER_DIRECT (ctf_step_core.h) in place of the rings' digest windows.  META: the wave also writes its envs' metadata
// rows, made from the final records while they are in LDS (ctf_meta.h) — a template argument, so that the kernels without it are
// instruction for instruction what they were: k_step<true, 4> is short of registers as it is.
template <bool METRICS, int W, bool PUBLISH, bool DIRECT = false, bool META = false>
__device__ __forceinline__ void step_block(const DevCfg& cfg, const DevPtrs& p, const int8_t* __restrict__ actions, float* __restrict__ rw32,
                                           double* __restrict__ rw64, uint8_t* __restrict__ done_out, uint32_t flags, int sb, int lane,
                                           uint32_t* lds, const StepPub& pub, const StepMeta& sm = StepMeta{nullptr, 0u}) {
    constexpr int EPW = WAVE / W;  // envs per wave
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const int g = lane / W, j = lane % W;
    const int env0 = sb * EPW;
    const int nvalid = min(EPW, cfg.n_envs - env0);
    const int SLB = step_slot_bytes(cfg.GS, cfg.RS, cfg.N, METRICS);
    const int SLW = SLB / 4, GW = cfg.GS / 4, RW = cfg.RS / 4;
    const int AW = 4, WW = STEP_RNG_WORDS;  // action words, digest-window words per slot
    const int N = cfg.N;
    const int e = env0 + g;
    const bool live = g < nvalid;
    const int e_ld = live ? e : cfg.n_envs - 1;  // the idle groups of a ragged last block shadow a valid env: every load below is
                                                 // unconditional, so that the compiler can count them (a load under a branch makes
                                                 // every later wait a full drain: two serialised round trips instead of one)
    // the two stream positions: the addresses of the step's random digests depend on them, so they go first
    uint32_t rp_py = 0, rp_np = 0, ready2 = 0;
    if constexpr (!DIRECT) {
        rp_py = p.rngpos[2 * e_ld]; rp_np = p.rngpos[2 * e_ld + 1];
        ready2 = *(const uint16_t*)(p.rngready + 2 * (size_t)e_ld);
    }

    // ---- stage the wave's envs' grids, records and actions into LDS.  Flat, coalesced 16-byte loads, the first 4 + 2 per lane
    // issued before anything waits; the digest windows' loads follow them as soon as the stream positions are there.
    const u32x4* gsrc = (const u32x4*)(p.grid + (size_t)env0 * cfg.GS);
    const u32x4* rsrc = (const u32x4*)(p.rec + (size_t)env0 * cfg.RS);
    const int GQ = GW / 4, RQ = RW / 4;  // 16-byte quads per env (GS and RS are multiples of 16)
    const int ng = nvalid * GQ, nr = nvalid * RQ;
    u32x4 gv[4], rv[2];
#pragma unroll
    for (int u = 0; u < 4; u++) gv[u] = gsrc[min(lane + WAVE * u, ng - 1)];
#pragma unroll
    for (int u = 0; u < 2; u++) rv[u] = rsrc[min(lane + WAVE * u, nr - 1)];
    const int na = nvalid * N;
    const int8_t* asrc = actions + (size_t)env0 * N;
    int8_t av[2];
#pragma unroll
    for (int u = 0; u < 2; u++) av[u] = asrc[min(lane + WAVE * u, na - 1)];
    typename std::conditional<DIRECT, GroupRngDirect, GroupRng<W>>::type R;
    if constexpr (DIRECT) group_issue_loads(R, cfg, p, e_ld);
    else group_issue_loads<W>(R, cfg, p, e_ld, j, live, rp_py, rp_np, ready2);
    {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int q = lane + WAVE * u;
            if (q < ng) {
                const int el = (int)fdiv((uint32_t)q, cfg.div_gq), w = (q - el * GQ) * 4;
                uint32_t* slot = lds + el * SLW + w;
                slot[0] = gv[u].x; slot[1] = gv[u].y; slot[2] = gv[u].z; slot[3] = gv[u].w;
            }
        }
        for (int q = lane + WAVE * 4; q < ng; q += WAVE) {  // G > 16 only
            const u32x4 v = gsrc[q];
            const int el = (int)fdiv((uint32_t)q, cfg.div_gq), w = (q - el * GQ) * 4;
            uint32_t* slot = lds + el * SLW + w;
            slot[0] = v.x; slot[1] = v.y; slot[2] = v.z; slot[3] = v.w;
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int q = lane + WAVE * u;
            if (q < nr) {
                const int el = (int)fdiv((uint32_t)q, cfg.div_rq), w = (q - el * RQ) * 4;
                uint32_t* slot = lds + el * SLW + GW + w;
                slot[0] = rv[u].x; slot[1] = rv[u].y; slot[2] = rv[u].z; slot[3] = rv[u].w;
            }
        }
        for (int q = lane + WAVE * 2; q < nr; q += WAVE) {  // N > 8 only
            const u32x4 v = rsrc[q];
            const int el = (int)fdiv((uint32_t)q, cfg.div_rq), w = (q - el * RQ) * 4;
            uint32_t* slot = lds + el * SLW + GW + w;
            slot[0] = v.x; slot[1] = v.y; slot[2] = v.z; slot[3] = v.w;
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int idx = lane + WAVE * u;
            if (idx < na) {
                const int el = (int)fdiv((uint32_t)idx, cfg.div_n), i = idx - el * N;
                ((int8_t*)(lds + el * SLW + GW + RW))[i] = av[u];
            }
        }
        for (int idx = lane + WAVE * 2; idx < na; idx += WAVE) {  // W = 1 with N > 2 only
            const int el = (int)fdiv((uint32_t)idx, cfg.div_n), i = idx - el * N;
            ((int8_t*)(lds + el * SLW + GW + RW))[i] = asrc[idx];
        }
        if (METRICS) {
            const int MW = (CTF_N_METRICS * N + 3) / 4;
            for (int idx = lane; idx < nvalid * MW; idx += WAVE) {
                const int el = (int)fdiv((uint32_t)idx, cfg.div_mw), w = idx - el * MW;
                lds[el * SLW + GW + RW + AW + WW + w] = 0;
            }
        }
    }
    // a block is ONE wave: LDS operations of a wave complete in order, so the staged bytes only need the wave's own LDS
    // counter — a __syncthreads() would also drain every outstanding global load (the random words') and store
    STEP_LDS_SYNC();
    STEP_STAMP(1);

    uint32_t left_ring = 0;
    if (live) group_step<METRICS, W>(R, cfg, p, (uint8_t*)(lds + g * SLW), e, j, g * W, flags, rw32, rw64, done_out, left_ring);
    (void)left_ring;
    STEP_LDS_SYNC();
    STEP_STAMP(2);

    // ---- the metadata values of the wave's envs, flat over the lanes (one f64 division sequence per 64 (env, value) pairs, where
    // the render spent one per env), parked in each slot's action and digest-window bytes: the step is through with those
    const MetaSlots mslots = {(uint8_t*)lds, SLB, cfg.GS, cfg.GS + cfg.RS};
    static_assert(2 * META_MV_COUNT <= 4 * (4 + STEP_RNG_WORDS), "an env's metadata values do not fit its slot's dead words");
    if constexpr (META) {
        meta_park_fracs(cfg, mslots, nvalid, lane, WAVE);
        meta_park_agents(cfg, mslots, nvalid, lane, WAVE);
    }

    // ---- write the envs back (flat, coalesced 16-byte stores)
    {
        u32x4* gdst = (u32x4*)(p.grid + (size_t)env0 * cfg.GS);
        u32x4* rdst = (u32x4*)(p.rec + (size_t)env0 * cfg.RS);
#pragma unroll 2
        for (int q = lane; q < ((STEP_ABLATE & 64) ? 0 : ng); q += WAVE) {
            const int el = (int)fdiv((uint32_t)q, cfg.div_gq), w = (q - el * GQ) * 4;
            const uint32_t* slot = lds + el * SLW + w;
            const u32x4 v = {slot[0], slot[1], slot[2], slot[3]};
            if (PUBLISH) store_sc1_x4(gdst + q, v);
            else gdst[q] = v;
        }
#pragma unroll 2
        for (int q = lane; q < nr; q += WAVE) {
            const int el = (int)fdiv((uint32_t)q, cfg.div_rq), w = (q - el * RQ) * 4;
            const uint32_t* slot = lds + el * SLW + GW + w;
            const u32x4 v = {slot[0], slot[1], slot[2], slot[3]};
            if (PUBLISH) store_sc1_x4(rdst + q, v);
            else rdst[q] = v;
        }
        if (PUBLISH) step_publish(pub, sb, lane);
        if constexpr (META) {  // the rows: every element one of the parked values (which one: meta_lut), 8 bytes per lane and pass
            STEP_LDS_SYNC();
            meta_gather_store(cfg, mslots, p.meta_lut, sm.chunk_div, nvalid, lane, WAVE, sm.out + (size_t)env0 * N * cfg.M);
        }
        if (METRICS && !(STEP_ABLATE & 32)) {
            // this step's u8 deltas are added to the i32 counters with no-return atomics (nothing to wait for); two
            // neighbouring counters share one 64-bit add (a counter never carries out of its 32 bits)
            const int MN = CTF_N_METRICS * N;
            int32_t* mdst = p.metrics + (size_t)env0 * MN;
            if ((MN & 1) == 0) {
                for (int idx = lane; idx < nvalid * MN / 2; idx += WAVE) {
                    const int el = (int)fdiv((uint32_t)(2 * idx), cfg.div_mn), w = 2 * idx - el * MN;
                    const uint8_t* d = (const uint8_t*)(lds + el * SLW + GW + RW + AW + WW) + w;
                    const unsigned long long inc = (unsigned long long)d[0] | ((unsigned long long)d[1] << 32);
                    if (inc) atomicAdd((unsigned long long*)(mdst + 2 * idx), inc);
                }
            } else {
                for (int idx = lane; idx < nvalid * MN; idx += WAVE) {
                    const int el = (int)fdiv((uint32_t)idx, cfg.div_mn), w = idx - el * MN;
                    const uint8_t inc = ((const uint8_t*)(lds + el * SLW + GW + RW + AW + WW))[w];
                    if (inc) atomicAdd(mdst + idx, (int32_t)inc);
                }
            }
        }
    }
    STEP_STAMP(4);
}


// ---- host side: // run-time switches -> template arguments: f gets std::integral_constant values
template <typename F>
static void with_bool(bool b, F f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
template <typename F>
static void with_step_variant(bool log_metrics, int w, F f) {  // f(METRICS, W)
    with_bool(log_metrics, [&](auto m) {
        if (w <= 1) f(m, std::integral_constant<int, 1>{});
        else if (w == 2) f(m, std::integral_constant<int, 2>{});
        else if (w == 4) f(m, std::integral_constant<int, 4>{});
        else f(m, std::integral_constant<int, 8>{});
    });
}
