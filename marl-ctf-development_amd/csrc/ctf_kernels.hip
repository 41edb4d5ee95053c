// ctf_kernels.hip — hand-written gfx950 (CDNA4) kernels of the batched GridworldCtf hot path.
//
//   k_reset           GridworldCtf.reset()                       (reference gridworld_ctf.py:383-477)
//   k_step            GridworldCtf.step(actions)                 (reference gridworld_ctf.py:849-918); its tail blocks
//                     regenerate the MT19937 rings (ctf_ring_dev.h)
//   k_observe         standardise_state + get_env_metadata, all agents (gridworld_ctf.py:975-1069), one wave per env at a time
//   k_observe_tiles   the same render as one-shot 8 KiB tiles of the flat buffer (the default where it applies)
//   k_step_observe    k_step and k_observe_tiles in ONE launch (opt-in) — why step and render share this translation unit
//                     (k_step_direct, the step of CTF_RNG_COUNTER_DIRECT: ctf_step_direct.hip)
//   k_observe_codes   the compact observation: one byte per (agent, cell)
//   k_export_counters bulk export of the evaluation counters
//   k_random_actions  synthetic Philox4x32-10 action stream for bench / tests
// and their launchers (ctf_launch.h).  Seeding, the bulk ring refill and the generators' import / export: ctf_rng.hip.
// The retained render (k_observe_delta, k_observe_delta_bitmap, k_obs_key_clear and their launchers) is ctf_observe_delta.hip, a
// translation unit of its own: work on it leaves this file's code objects alone.  What both share: ctf_render_dev.h.
//
// Integer / byte work, HBM-bound: no MFMA anywhere.  Wavefront = 64 lanes is assumed throughout.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "ctf_launch.h"
// Profiling-only phase trace of the step kernel (tools/trace_step.py): lane 0 of every block stamps the 100 MHz wall clock at
// fixed points (0 start, 1 staged, 7 hit bits, 5 ring, 6 shuffle 1, 8/9/10 + 3 k act / tagging / metrics of turn k, 32 turns
// done, 33 shuffle 2, 34 stepped, 2 barrier, 3 written back, 4 end); never defined in the shipped build.
#ifndef STEP_TRACE
#define STEP_TRACE 0
#endif
#if STEP_TRACE
__device__ unsigned long long g_step_trace[8192][40];
#ifndef STEP_TRACE_MASK
#define STEP_TRACE_MASK 0xFFFFFFFFFFull
#endif
#define CTF_STAMP(k) do { if (((STEP_TRACE_MASK >> (k)) & 1ull) && threadIdx.x == 0 && blockIdx.x < 8192) g_step_trace[blockIdx.x][(k)] = wall_clock64(); } while (0)
#endif
#include "ctf_ring_dev.h"  // (and through it ctf_step_core.h: both after CTF_STAMP)
#include "ctf_meta.h"

// ------------------------------------------------------------------------------------------------
// small helpers (fdiv, cheb, the SGPR-pinned config lookups, MT19937: ctf_step_core.h / ctf_mt.h)
// ------------------------------------------------------------------------------------------------
// (the metadata values and f64_to_f16: ctf_meta.h)

// ------------------------------------------------------------------------------------------------
// reset
// ------------------------------------------------------------------------------------------------
// One 64-lane block per env; mask == nullptr resets every env.  init_perm is set only by ctf_create.
extern "C" __global__ void __launch_bounds__(WAVE) k_reset(DevCfg cfg, DevPtrs p, const uint8_t* mask, int init_perm) {
    int e = blockIdx.x, lane = threadIdx.x;
    if (mask && !mask[e]) return;
    uint32_t* g = (uint32_t*)(p.grid + (size_t)e * cfg.GS);
    const uint32_t* src = (const uint32_t*)p.init_grid;
    for (int w = lane; w < cfg.GS / 4; w += WAVE) g[w] = src[w];
    uint8_t* sr = p.rec + (size_t)e * cfg.RS;
    if (lane == 0) {
        reset_record(cfg, sr);
        if (init_perm)
            for (int i = 0; i < cfg.N; i++) sr[cfg.off_perm + i] = (uint8_t)i;
    }
    if (cfg.log_metrics) {
        int32_t* m = p.metrics + (size_t)e * CTF_N_METRICS * cfg.N;
        for (int w = lane; w < CTF_N_METRICS * cfg.N; w += WAVE) m[w] = 0;
        // visitation: reset_record flagged the base maps as zero and emptied the log — nothing to clear
    }
}

// ------------------------------------------------------------------------------------------------
// step — W lanes per env (W = 1, 2, 4 or 8 >= opponents per team), 64 / W envs per 64-thread block
// ------------------------------------------------------------------------------------------------
// The per-agent loop of GridworldCtf.step is inherently sequential (later agents see earlier agents' moves, tags and
// respawns), so parallelism is across envs — but one lane per env leaves one wave per SIMD and a kernel bound by the
// dependent LDS / VALU chain.  Here the W lanes of a group run the env's control flow redundantly (state reads are LDS
// broadcasts; state writes are the same store from every lane) and split the work that is parallel inside an agent's turn:
//   - tagging: every lane holds the rand() < TAG_PROBABILITY bits of its share of the step's np.random window and evaluates
//     one opponent; __ballot finds the first hit, which is applied (possibly respawning, which consumes extra words) before
//     the remaining opponents are re-evaluated from the shifted stream position — exactly the reference's draw order;
//   - adjacency / zone metrics, healing, rewards, visitation: one agent per sub-lane;
//   - the digests of the step's random words (ctf_mt.h) arrive with the staging loads; the MT19937 blocks themselves are
//     regenerated by the launch's tail blocks.
// 64 / W envs per wave means W times more waves (4 per SIMD for the arena) to hide the latency chain.
// The logic itself — env_step, the two streams, group_step — is ctf_step_core.h.
//
#if STEP_TRACE
#define STEP_STAMP(k) CTF_STAMP(k)
extern "C" int ctf_debug_step_trace(unsigned long long* host_out) {
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_step_trace), sizeof(g_step_trace));
}
#else
#define STEP_STAMP(k) do { } while (0)
#endif

#include "ctf_step_block.h"  // step_block: the staging, group_step and the write-back of one step block
#include "ctf_render_dev.h"  // what the renders share (behind STEP_STAMP, like ctf_step_block.h, which it includes)

#ifndef STEP_TAIL_PAIRS
#define STEP_TAIL_PAIRS 16  // (env, stream) pairs a tail block looks after (ring regeneration)
#endif

// A TAIL block of k_step: regenerates rings whose consumers have moved on (rngready says
// which).  It looks after STEP_TAIL_PAIRS (env, stream) pairs; a stale ring of env e is taken by the launch that finds it at
// the age (launches waited so far) with (e + age) % rng_spread == 0, because the envs' stream positions move in step (every env
// draws the same words per step, give or take a respawn): most of them leave their block in the same step, and that burst is
// spread over rng_spread launches — always before the ring is needed.  The ages live in device memory (rngage, written by the
// pair's tail block only), not in a launch argument: a launch is the same whichever step it is, so a caller may capture
// ctf_step / ctf_step_observe into a hipGraph and replay it.  A tail block touches nothing a step block reads: an env whose ring
// is stale stands at the head of its new block and looks at neither the other ring nor its mirror.
__device__ __forceinline__ void tail_block(const DevCfg& cfg, const DevPtrs& p, int tb, int lane, uint32_t* lds) {
    const int first = tb * STEP_TAIL_PAIRS;
    const bool mine = lane < STEP_TAIL_PAIRS && first + lane < 2 * cfg.n_envs;
    uint32_t flag = 1, age = 0;
    if (mine) {
        flag = p.rngready[first + lane];
        age = p.rngage[first + lane];
    }
    const uint32_t spread = (uint32_t)cfg.rng_spread;
    const bool take = flag >= 2u && (((uint32_t)((first + lane) >> 1) + age) % spread == 0u || age >= spread);
    {   // a ring that goes on waiting is a launch older; everything else is new again
        const uint32_t older = (flag >= 2u && !take) ? age + 1u : 0u;
        if (mine && older != age) p.rngage[first + lane] = (uint8_t)older;
    }
    unsigned long long work = __ballot(take);
    STEP_STAMP(0);
    int n_done = 0;
    if (work) {  // uniform
        int k = __ffsll((long long)work) - 1;
        work &= work - 1;
        RingIn cur = ring_fetch(cfg, p, (first + k) >> 1, (first + k) & 1, (uint32_t)__shfl((int)flag, k, WAVE), lane);
        for (;;) {
            // the next ring's words set out before this one is worked on (its loads land during the ~3 us of twisting and digesting)
            const int kn = work ? __ffsll((long long)work) - 1 : k;
            const bool more = work != 0;
            work &= work - 1;
            RingIn nxt = cur;
            if (more) nxt = ring_fetch(cfg, p, (first + kn) >> 1, (first + kn) & 1, (uint32_t)__shfl((int)flag, kn, WAVE), lane);
            refill_ring(cfg, p, (first + k) >> 1, (first + k) & 1, cur, lane, lds, lds + CTF_MT_N, false);
            n_done++;
            if (!more) break;
            cur = nxt;
            k = kn;
        }
    }
    STEP_STAMP(4);
#if STEP_TRACE
    if (threadIdx.x == 0 && blockIdx.x < 8192) g_step_trace[blockIdx.x][5] = (unsigned long long)n_done;
#else
    (void)n_done;
#endif
}
// 16 blocks (= waves) per CU fit by LDS: the register budget is held to the matching 4 waves per SIMD (128 VGPRs)
// META: the step blocks also write their envs' metadata rows (StepArgs.meta; step_block)
template <bool METRICS, int W, bool META>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_step(DevCfg cfg, DevPtrs p, const int8_t* __restrict__ actions, float* __restrict__ rw32, double* __restrict__ rw64,
       uint8_t* __restrict__ done_out, uint32_t flags, int n_step_blocks, StepMeta sm) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x;
    const int sb = (int)blockIdx.x;  // this step block's index
    if (sb >= n_step_blocks) {
        // ---- a TAIL block (see tail_block): these start as step blocks retire — the LDS is full until then.  (Tried: the tail
        // blocks at the HEAD of the grid instead — not faster, profiles/r03_tail_block_ablation.txt.)
        tail_block(cfg, p, sb - n_step_blocks, lane, lds);
        return;
    }
    STEP_STAMP(0);
#if STEP_TRACE
    if (threadIdx.x == 0 && blockIdx.x < 8192)
        g_step_trace[blockIdx.x][39] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) |
                                       ((unsigned long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) << 32);
#endif
    step_block<METRICS, W, false, false, META>(cfg, p, actions, rw32, rw64, done_out, flags, sb, lane, lds, StepPub{}, sm);
}

// ------------------------------------------------------------------------------------------------
// observe — one wave per env at a time; the env's whole one-hot block is first built as a BITMAP in LDS
// ------------------------------------------------------------------------------------------------
// The observation block u8 [N][C][G][G] of one env is ~98 % zeros.  Per env a wave
//   1. zeroes a bitmap of N*C*G*G bits in LDS (one bit per output byte),
//   2. sets the hot bits: for every non-empty grid cell and every agent, bit
//      i*C*G*G + channel(viewer team, tile)*G*G + (reversed ? flip(cell) : cell), plus the own-position
//      bit of plane 0 — LDS atomic ORs, relabelling via the SGPR-resident channel LUT,
//   3. streams the block out: 16-byte chunk k of the output is halfword k of the bitmap with every bit
//      expanded to a byte (3 full-rate VALU ops per 4 bytes), one 1-KiB-aligned coalesced store
//      instruction per 64 chunks.
// Metadata rows (f16 [N][2N+6]) are assembled in LDS and leave as 8-byte stores.
// (The per-wave LDS sizes of the renders, expand4, flip_cell, obs_meta_lut and obs_build_env: ctf_render_dev.h.)

#ifndef OBS_TILES_DEFAULT
#define OBS_TILES_DEFAULT 1  // ctf_launch_observe takes the tile render whenever it applies (CTF_OBS_TILES=0 / 1 overrides)
#endif
#ifndef STEP_OBSERVE_ONE_LAUNCH_DEFAULT
// ctf_step_observe is k_step_observe only when CTF_STEP_OBSERVE_ONE_LAUNCH=1 (and the tile render applies): measured at 65 536
// arena envs it is 9 % SLOWER than the two launches (0.325 against 0.298 ms, profiles/r06_one_launch_step_observe.md)
#define STEP_OBSERVE_ONE_LAUNCH_DEFAULT 0
#endif
// A load the compiler does not track: issued one env ahead of its use, waited for by obs_prefetch_wait.
// (vmcnt retires in issue order, so a compiler-placed wait for next env's state would first drain every
// store of the current env; issued BEFORE those stores and waited for with a counted vmcnt a few
// stores later, the data is simply there when the wave reaches the next env.)
__device__ __forceinline__ uint32_t obs_prefetch_dword(const uint32_t* ptr) {
    uint32_t v;
    asm volatile("global_load_dword %0, %1, off" : "=v"(v) : "v"(ptr) : "memory");
    return v;
}
#ifndef OBS_PREFETCH
#define OBS_PREFETCH 1  // 0 = profiling comparison only (tools/ablate.sh)
#endif
#ifndef OBS_UNROLL
#define OBS_UNROLL 8    // store instructions per pass of the stream loop
#endif
#define OBS_PF_WAIT 16  // stream iteration (a multiple of OBS_UNROLL) at which the prefetched state is waited for ...
// ... with vmcnt(8): the two prefetch loads are older than the >= OBS_PF_WAIT stores issued since
#define OBS_PREFETCH_WAIT(a, b) asm volatile("s_waitcnt vmcnt(8)" : "+v"(a), "+v"(b)::"memory")
#define OBS_PREFETCH_DRAIN(a, b) asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b)::"memory")

// one 16-byte chunk of the observation block: h = halfword k of the bitmap, every bit expanded to a byte
template <int ALIGN>
__device__ __forceinline__ void obs_store_chunk(uint8_t* out, uint32_t h, int k, int nfull, int tail, uint32_t& ablate_acc) {
    const uint32_t o = (uint32_t)k << 4;
    uint32_t x[4];
    if (OBS_ABLATE & 1) { x[0] = x[1] = x[2] = x[3] = h; }
    else {
#pragma unroll
        for (int j = 0; j < 4; j++) x[j] = expand4(h, j);
    }
    if (OBS_ABLATE & 2) { ablate_acc ^= x[0] ^ x[1] ^ x[2] ^ x[3]; return; }
    if (k < nfull) {
        if (ALIGN >= 4) {
            typedef typename OutVec<(ALIGN >= 16 ? 16 : 4)>::type V;
            const V v = {x[0], x[1], x[2], x[3]};
            *(V*)(out + o) = v;  // plain store: measured faster than nontemporal for this pattern
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) out[o + j] = (uint8_t)(x[j >> 2] >> ((j & 3) * 8));
        }
    } else {
        for (int j = 0; j < tail; j++) out[o + j] = (uint8_t)(x[j >> 2] >> ((j & 3) * 8));
    }
}

// Every wave builds and streams its own envs.  (A builder / streamer split — one wave of a block building the next
// three envs' bitmaps while the other three stream — was tried and measured 15-25 % slower: a single builder wave's
// dependent chain is too long, and 24 streaming waves per CU drive the store path less well than 32.)
template <int ALIGN>
__global__ void __launch_bounds__(256) k_observe(DevCfg cfg, DevPtrs p, uint8_t* __restrict__ obs,
                                                 uint16_t* __restrict__ meta, uint32_t reverse_mask, uint32_t xcd_map) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int wpb = blockDim.x / WAVE;
    const int N = cfg.N, M = cfg.M;
    uint8_t* wl = (uint8_t*)lds + wave * obs_wave_bytes(cfg.RS, N, M, cfg.obs_bytes);
    uint8_t* srec = wl;
    uint16_t* mv = (uint16_t*)(wl + cfg.RS);
    uint16_t* mstage = (uint16_t*)(wl + cfg.RS + OBS_MV_BYTES);
    uint8_t* mlut = wl + cfg.RS + OBS_MV_BYTES + obs_meta_stage_bytes(N, M);
    uint32_t* bits = (uint32_t*)(mlut + obs_meta_lut_bytes(N, M));
    const ObsSlots slots = obs_slots(cfg, reverse_mask);
    if (meta) obs_meta_lut(cfg, mlut, mv, lane);
    const int GW = cfg.GS / 4;
    const int rec_lane = min(lane, cfg.RS / 4 - 1), grid_lane = min(lane, GW - 1);
    // Consecutive workgroups go to consecutive XCDs: with xcd_map (grid a multiple of 8 blocks) XCD x renders ITS OWN contiguous
    // eighth of the envs instead of every XCD writing into every page of the buffer (see k_observe_tiles).
    int e_first = blockIdx.x * wpb + wave, e_stride = gridDim.x * wpb, e_end = cfg.n_envs;
    if (xcd_map) {
        const int chunk = (cfg.n_envs + 7) >> 3, lo = (int)(blockIdx.x & 7u) * chunk;
        e_first = lo + (int)(blockIdx.x >> 3) * wpb + wave;
        e_stride = (int)(gridDim.x >> 3) * wpb;
        e_end = min(lo + chunk, cfg.n_envs);
    }
    // the first env's state: ordinary loads; every later env's state arrives through the prefetch below
    // (Tried: no compiler-tracked load anywhere in the render loop, these two as prefetches too — wrong results beyond G = 16
    // and no timing recorded.)
    uint32_t recw = 0, cells = 0;
    if (e_first < e_end) {
        recw = ((const uint32_t*)(p.rec + (size_t)e_first * cfg.RS))[rec_lane];
        cells = ((const uint32_t*)(p.grid + (size_t)e_first * cfg.GS))[grid_lane];
    }

    for (int e = e_first; e < e_end; e += e_stride) {
        obs_build_env(cfg, p, e, recw, cells, srec, mv, mstage, mlut, bits, slots, reverse_mask, lane, obs != nullptr, meta);

        // ---- stream the observation block: 16 bytes per lane per store.  Wave store instructions are
        // aligned to 1 KiB of the flat output (k starts negative), so only an env's first and last
        // instruction touch a partial line.
        if (obs) {
            const size_t base = (size_t)e * cfg.obs_bytes;
            uint8_t* out = obs + base;
            const uint16_t* hb = (const uint16_t*)bits;
            const int nfull = cfg.obs_bytes >> 4;
            const int tail = cfg.obs_bytes & 15;
            const int nchunks = nfull + (tail ? 1 : 0);
            const int k0 = (ALIGN >= 16) ? -(int)(((base + (uintptr_t)obs) >> 4) & 63) : 0;
            uint32_t ablate_acc = 0;
            const int niter = (nchunks - k0 + WAVE - 1) / WAVE;
            const int e_next = min(e + e_stride, e_end - 1);
            uint32_t nrec = 0, ncells = 0;
            // OBS_UNROLL store instructions per pass, their bitmap halfwords read first: the stores then issue back to back
            // instead of each waiting for its own LDS round trip
            for (int it0 = 0; it0 < niter; it0 += OBS_UNROLL) {
                if (OBS_PREFETCH && it0 == 0) {  // next env's state: issued before this env's first store
                    nrec = obs_prefetch_dword((const uint32_t*)(p.rec + (size_t)e_next * cfg.RS) + rec_lane);
                    ncells = obs_prefetch_dword((const uint32_t*)(p.grid + (size_t)e_next * cfg.GS) + grid_lane);
                }
                if (OBS_PREFETCH && it0 == OBS_PF_WAIT) OBS_PREFETCH_WAIT(nrec, ncells);
                uint32_t h[OBS_UNROLL];
#pragma unroll
                for (int u = 0; u < OBS_UNROLL; u++) {
                    const int k = k0 + lane + (it0 + u) * WAVE;
                    h[u] = (k >= 0 && k < nchunks) ? hb[k] : 0u;
                }
#pragma unroll
                for (int u = 0; u < OBS_UNROLL; u++) {
                    const int k = k0 + lane + (it0 + u) * WAVE;
                    if (k >= 0 && k < nchunks) obs_store_chunk<ALIGN>(out, h[u], k, nfull, tail, ablate_acc);
                }
            }
            if ((OBS_ABLATE & 2) && ablate_acc == 0x12345678u) out[lane] = 1;  // keeps the ablated work alive
            if (OBS_PREFETCH) {
                if (niter <= OBS_PF_WAIT) OBS_PREFETCH_DRAIN(nrec, ncells);
                recw = nrec;
                cells = ncells;
            } else if (e + e_stride < e_end) {
                recw = ((const uint32_t*)(p.rec + (size_t)(e + e_stride) * cfg.RS))[rec_lane];
                cells = ((const uint32_t*)(p.grid + (size_t)(e + e_stride) * cfg.GS))[grid_lane];
            }
        } else if (e + e_stride < e_end) {
            recw = ((const uint32_t*)(p.rec + (size_t)(e + e_stride) * cfg.RS))[rec_lane];
        }
        __builtin_amdgcn_s_waitcnt(LGKM_ONLY);  // this env's LDS reads are done before the next env reuses the bitmap
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------------
// observe as one-shot TILES — the same bitmap idea, organised by output address instead of by env
// ------------------------------------------------------------------------------------------------
// Wave t of the grid renders CTF_OBS_TILE (8 192) consecutive bytes of the FLAT observation buffer and exits: it loads the
// grid of the (at most two) envs its tile touches, builds only the bits of its own tile — for each of the agent views whose
// blocks intersect the tile, every non-empty cell gives one candidate bit — and issues eight store instructions.  Why:
// the chip then writes a compact window that moves linearly through the buffer and a wave issues few stores.  On MI355X a
// wave that issues 1 / 4 / 8 / 25 store instructions in a row sustains 6.9 / 5.9 / 5.7 / 5.5 TB/s chip-wide, and the long
// per-wave streams of k_observe lose another 15 % on the "slow" kind of allocation (on some boxes: every allocation) while
// one-shot tiles do not (profiles/r02_store_bw8_tiles.txt).  The price: the cell scan is repeated by
// every tile of an env (3.1 tiles per arena env) for the views the tile holds, and every wave pays the prologue — so both are
// kept lean: envs come in groups whose blocks fill a whole number of tiles (no 64-bit division), a cell's flipped index and
// its channel code for either viewing team are worked out once per grid dword, a view costs ~7 instructions per cell, and
// the metadata LUT comes from a table the host built.
// The 1-D grid is walked XCD-contiguously (block b -> logical block (b % 8) * (blocks / 8) + b / 8): each of the 8 XCDs writes
// its own eighth of the buffer front to back, 0.306 -> 0.259 ms on the arena (profiles/r02_store_bw9_xcd.txt for the bare pattern).
// Metadata rows: written by the wave whose tile holds an env's first byte.
// Used when an env's block is a multiple of 16 bytes and >= one tile and the buffer is 16-byte aligned (ctf_launch_observe).
#ifndef OBS_TILE_BLOCK_LDS
#define OBS_TILE_BLOCK_LDS (10 * 1024)  // dynamic LDS of a k_observe_tiles block at least: 160 KiB / 10 KiB = 16 blocks (waves) per CU
#endif

// What a tile of k_step_observe waits for: the flags of the (one or two) step blocks of its envs (EPW = 1 << epw_shift envs each).
struct TileWait {
    const uint32_t* sync;  // the handle's sync words: seq, then (from CTF_SYNC_FLAGS) the step blocks' flags
    int epw_shift;
    uint64_t ticks;        // bound of the wait (wall clock): then CTF_ST_SYNC_TIMEOUT and the tile goes on
};
// One lane: seq and the two flags are loaded together (one round trip in the common case, the step blocks long done); then the
// flags alone are polled until both hold seq + 1.
__device__ __forceinline__ bool wait_flags(const TileWait& tw, int sa, int sz) {
    const uint32_t* fa = tw.sync + CTF_SYNC_FLAGS + sa;
    const uint32_t* fz = tw.sync + CTF_SYNC_FLAGS + sz;
    const uint32_t seq = ld_sc1(tw.sync);
    uint32_t a = ld_sc1(fa), z = ld_sc1(fz);
    const uint32_t value = seq + 1u;
    if (a == value && z == value) return true;
    const uint64_t t0 = wall_clock64();
    for (;;) {
        __builtin_amdgcn_s_sleep(2);
        if (a != value) a = ld_sc1(fa);
        if (z != value) z = ld_sc1(fz);
        if (a == value && z == value) return true;
        if (wall_clock64() - t0 > tw.ticks) return false;
    }
}
// the state of the envs the tile reads: with SYNC (k_step_observe) agent-scope (`sc1`) loads, see StepPub
template <bool SYNC>
__device__ __forceinline__ uint32_t ld_state(const uint32_t* a) { return SYNC ? ld_sc1(a) : *a; }

// One tile: logical block lb (XCD map applied), wave `wave` of it; wl = the wave's LDS.  SYNC: k_step_observe's tile (TileWait).
template <int STORE_NT, bool SYNC>
__device__ __forceinline__ void tile_render(const DevCfg& cfg, const DevPtrs& p, uint8_t* __restrict__ obs, uint16_t* __restrict__ meta,
                                            uint32_t reverse_mask, uint32_t lb, int wave, int lane, uint8_t* wl, const TileWait& tw) {
    const int N = cfg.N, G = cfg.G, GG = cfg.GG, CGG = cfg.CGG, OB = cfg.obs_bytes;
    const uint32_t grp = fdiv(lb, cfg.div_tile_bx);
    const int tt = (int)(lb - grp * (uint32_t)cfg.tile_bx) * CTF_OBS_TILE_WPB + wave;
    if (tt >= cfg.tile_tpg) return;
    const int env_base = (int)grp * cfg.tile_k;
    if (env_base >= cfg.n_envs) return;
    const uint32_t lo_local = (uint32_t)tt * OBS_TILE;                  // < tile_k * obs_bytes
    const int el = (int)fdiv(lo_local, cfg.div_ob_tile);
    const int off0 = (int)(lo_local - (uint32_t)el * (uint32_t)OB);    // the tile starts at byte off0 of env e0's block
    const int e0 = env_base + el;
    if (e0 >= cfg.n_envs) return;
    const bool two = off0 + OBS_TILE > OB && e0 + 1 < cfg.n_envs;       // the tile runs into env e0 + 1 (obs_bytes >= tile: never further)
    if (SYNC) {  // the step blocks of e0 (and e0 + 1) must have published this launch's state
        if (lane == 0) {
            if (!wait_flags(tw, e0 >> tw.epw_shift, (two ? e0 + 1 : e0) >> tw.epw_shift)) atomicOr(p.status, CTF_ST_SYNC_TIMEOUT);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (no instruction: the loads below stay behind the poll)
    }
    uint32_t* bits = (uint32_t*)wl;
    const int GW = cfg.GS / 4;
    // ---- the views (flat agent blocks) the tile intersects; the last ones may lie in env e0 + 1
    const int ia0 = (int)fdiv((uint32_t)off0, cfg.div_cgg);
    const int last = off0 + OBS_TILE - 1;  // relative to env e0's block
    const int ia1 = last < OB ? (int)fdiv((uint32_t)last, cfg.div_cgg) : N + (int)fdiv((uint32_t)(last - OB), cfg.div_cgg);
    // ---- loads, all issued before anything waits: the grids' dwords and (lane k: view k) the viewer's two position bytes
    const uint32_t* g0 = (const uint32_t*)(p.grid + (size_t)e0 * cfg.GS);
    const uint32_t* g1 = (const uint32_t*)(p.grid + (size_t)(two ? e0 + 1 : e0) * cfg.GS);
    uint32_t c0[4], c1[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {  // G <= 32: at most 256 grid dwords (uniform conditions)
        c0[j] = (GW > WAVE * j) ? ld_state<SYNC>(g0 + min(lane + WAVE * j, GW - 1)) : 0u;
        c1[j] = (GW > WAVE * j && two) ? ld_state<SYNC>(g1 + min(lane + WAVE * j, GW - 1)) : 0u;
    }
    uint32_t own_bit = 0xFFFFFFFFu;
    {
        const int fa = ia0 + lane;
        const bool nxt = fa >= N;
        if (fa <= ia1 && !(nxt && !two)) {
            const int ik = nxt ? fa - N : fa;
            const uint8_t* rp = p.rec + (size_t)(nxt ? e0 + 1 : e0) * cfg.RS + cfg.off_pos + 2 * ik;
            const uint16_t rc = SYNC ? (uint16_t)(ld_sc1((const uint32_t*)((uintptr_t)rp & ~(uintptr_t)3)) >> (8 * ((uintptr_t)rp & 2)))
                                     : *(const uint16_t*)rp;
            const int r = (int)(int8_t)(rc & 0xFFu), c = (int)(int8_t)(rc >> 8);
            const int cell = ((reverse_mask >> ik) & 1u) ? flip_cell(cfg, r * G + c, r, c) : r * G + c;
            own_bit = (uint32_t)((nxt ? OB : 0) + ik * CGG - off0 + cell);
        }
    }
    for (int q = lane; q < OBS_TILE / 8 / 16; q += WAVE) ((u32x4_t*)bits)[q] = u32x4_t{0u, 0u, 0u, 0u};
    __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
    __builtin_amdgcn_wave_barrier();
    if (own_bit < (uint32_t)OBS_TILE) atomicOr(bits + (own_bit >> 5), 1u << (own_bit & 31u));
    if (!(OBS_ABLATE & 4)) {
        const uint32_t lut0_lo = (uint32_t)cfg.chan_lut[0], lut0_hi = (uint32_t)(cfg.chan_lut[0] >> 32);
        const uint32_t lut1_lo = (uint32_t)cfg.chan_lut[1], lut1_hi = (uint32_t)(cfg.chan_lut[1] >> 32);
#pragma unroll 1
        for (int j = 0; j * WAVE < GW; j++) {  // uniform; one pass for G <= 16
            const int w = lane + WAVE * j;
            const uint32_t cw0 = j == 0 ? c0[0] : (j == 1 ? c0[1] : (j == 2 ? c0[2] : c0[3]));
            const uint32_t cw1 = j == 0 ? c1[0] : (j == 1 ? c1[1] : (j == 2 ? c1[2] : c1[3]));
            // once per grid dword: for its 4 cells the plain and the flipped index and, per env, the channel code for either
            // viewing team (code NONE also for an empty cell)
            uint32_t plain[4], flipped[4], code0 = 0, code1 = 0;  // code0 / code1: byte b = (team-1 code << 4 | team-0 code) of env e0 / e0 + 1
            {
                int r = (int)fdiv((uint32_t)(w * 4), cfg.div_g), c = w * 4 - r * G;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int cell = w * 4 + b;
                    const bool in = w < GW && cell < GG;
                    plain[b] = (uint32_t)cell;
                    flipped[b] = (uint32_t)flip_cell(cfg, cell, r, c);
                    const uint32_t v0 = in ? (cw0 >> (8 * b)) & 0xFFu : 0u, v1 = in ? (cw1 >> (8 * b)) & 0xFFu : 0u;
                    const uint32_t sh0 = 4 * (v0 & 7u), sh1 = 4 * (v1 & 7u);
                    const uint32_t k00 = v0 ? (((v0 & 8u) ? lut0_hi : lut0_lo) >> sh0) & 15u : CTF_TILE_NONE;
                    const uint32_t k01 = v0 ? (((v0 & 8u) ? lut1_hi : lut1_lo) >> sh0) & 15u : CTF_TILE_NONE;
                    const uint32_t k10 = v1 ? (((v1 & 8u) ? lut0_hi : lut0_lo) >> sh1) & 15u : CTF_TILE_NONE;
                    const uint32_t k11 = v1 ? (((v1 & 8u) ? lut1_hi : lut1_lo) >> sh1) & 15u : CTF_TILE_NONE;
                    code0 |= (k00 | (k01 << 4)) << (8 * b);
                    code1 |= (k10 | (k11 << 4)) << (8 * b);
                    if (++c == G) { c = 0; r++; }
                }
            }
#pragma unroll 1
            for (int fa = ia0; fa <= ia1; fa++) {  // uniform: the views
                const bool nxt = fa >= N;
                if (nxt && !two) break;
                const int ik = nxt ? fa - N : fa;
                const int tsh = (int)((cfg.team_mask >> ik) & 1u) * 4;
                const bool rev = (reverse_mask >> ik) & 1u;
                const int base = (nxt ? OB : 0) + ik * CGG - off0;  // the view's block starts at tile bit `base` (may be negative)
                const uint32_t codes = nxt ? code1 : code0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const uint32_t code = (codes >> (8 * b + tsh)) & 15u;
                    const uint32_t bit = (uint32_t)(base + (int)(code * (uint32_t)GG + (rev ? flipped[b] : plain[b])));
                    if (code != CTF_TILE_NONE && bit < (uint32_t)OBS_TILE) atomicOr(bits + (bit >> 5), 1u << (bit & 31u));
                }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(LGKM_ONLY);  // the atomic ORs have landed
    __builtin_amdgcn_wave_barrier();
    // ---- stream: TILE / 1 KiB store instructions, their bitmap halfwords read first (obs_bytes % 16 == 0: whole chunks)
    {
        const uint16_t* hb = (const uint16_t*)bits;
        const unsigned long long lo = (unsigned long long)env_base * (unsigned long long)OB + lo_local;
        const unsigned long long left = (unsigned long long)cfg.n_envs * (unsigned long long)OB - lo;
        const int nchunk = (int)((left < (unsigned long long)OBS_TILE ? left : (unsigned long long)OBS_TILE) >> 4);
        uint8_t* out = obs + lo;
        uint32_t h[OBS_TILE / 1024];
#pragma unroll
        for (int u = 0; u < OBS_TILE / 1024; u++) h[u] = hb[u * WAVE + lane];
#pragma unroll
        for (int u = 0; u < OBS_TILE / 1024; u++) {
            const int k = u * WAVE + lane;
            const u32x4_t v = {expand4(h[u], 0), expand4(h[u], 1), expand4(h[u], 2), expand4(h[u], 3)};
            if (k < nchunk && !(OBS_ABLATE & 2)) {
                if (STORE_NT) __builtin_nontemporal_store(v, (u32x4_t*)(out + ((size_t)k << 4)));
                else *(u32x4_t*)(out + ((size_t)k << 4)) = v;
            }
        }
    }
    // ---- metadata rows of the env whose block starts in this tile (behind the stores: off the stream's path)
    const bool starts0 = off0 == 0;
    if (meta && (starts0 || two) && !(OBS_ABLATE & 8)) {
        const int em = starts0 ? e0 : e0 + 1;
        uint8_t* srec = wl + OBS_TILE / 8;
        uint16_t* mv = (uint16_t*)(srec + cfg.RS);
        uint16_t* mstage = (uint16_t*)(srec + cfg.RS + OBS_MV_BYTES);
        const uint32_t recw = ld_state<SYNC>((const uint32_t*)(p.rec + (size_t)em * cfg.RS) + min(lane, cfg.RS / 4 - 1));
        if (lane == 0) { mv[40] = 0x3C00u; mv[41] = 0u; }
        const ObsSlots none = {{0u, 0u, 0u, 0u}};
        obs_build_env(cfg, p, em, recw, 0u, srec, mv, mstage, p.meta_lut, nullptr, none, reverse_mask, lane, false, meta);
    }
}

template <int STORE_NT>  // 1 (batches whose observations exceed the memory-side cache, ctf_derive.h): the tile's stores carry the nontemporal hint
__global__ void __launch_bounds__(CTF_OBS_TILE_WPB * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) k_observe_tiles(DevCfg cfg, DevPtrs p, uint8_t* __restrict__ obs, uint16_t* __restrict__ meta,
                                                       uint32_t reverse_mask, uint32_t xcd_map) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    // ---- which tile of which group of envs (uniform, 32-bit)
    // The launch is 1-D and consecutive workgroups go to consecutive XCDs (8 of them).  Block b therefore takes logical
    // block (b % 8) * (blocks / 8) + b / 8: every XCD writes ITS OWN contiguous eighth of the buffer front to back instead of
    // every XCD touching every page — a constant 8 KiB-tile fill measures 6.2 instead of 5.6 TB/s that way (profiles/r02_store_bw9_xcd.txt).
    const uint32_t b = blockIdx.x;
    const uint32_t lb = xcd_map ? (b & 7u) * ((uint32_t)cfg.tile_nb >> 3) + (b >> 3) : b;
    tile_render<STORE_NT, false>(cfg, p, obs, meta, reverse_mask, lb, wave, lane, (uint8_t*)lds + wave * tiles_wave_bytes(cfg.RS, cfg.N, cfg.M),
                                 TileWait{});
}

// ------------------------------------------------------------------------------------------------
// step_observe — ONE launch of one-wave blocks: [step blocks | ring-regenerating tail blocks | render tiles]
// ------------------------------------------------------------------------------------------------
// ctf_step followed by ctf_observe's tile render, without the kernel boundary between them: the render no longer waits for the
// slowest of the step's waves and its tail (p50 43.8 / max 62 us, tail to 79 us: profiles/r03_kstep_phase_trace.txt) with most
// CUs idle.  A tile waits only for the flags of the (one or two) step blocks whose envs it renders (StepPub / TileWait); the
// blocks it waits for have lower indices, so under the in-order dispatch of a 1-D grid they are resident before it is (the
// wait is bounded all the same: CTF_ST_SYNC_TIMEOUT).  The tail blocks sit between the two so that their ring regeneration
// overlaps the render instead of trailing it.  One block shape for all three roles: one wave, the step's 128-VGPR budget
// (4 waves per SIMD) and the step's LDS; tile t takes the render's tile (t % 8) * (T / 8) + t / 8 (the XCD-contiguous walk of
// k_observe_tiles: the tiles start at a multiple of 8 blocks).  Results are those of k_step + k_observe_tiles, bit for bit.
// Measured (8_arena, 65 536 envs, in one process on shared buffers): 0.325 ms against 0.298 for the two launches.  Without any
// of the hand-off (no count, no waits, plain loads and stores: wrong results, timing only) the same shape takes 0.284: the
// generation's reader count costs ≈ 20 us (at the start or at the end of a block, over 16 … 1 024 counter lines alike), the
// waits and write-through accesses ≈ 15 more (profiles/r06_one_launch_step_observe.md).  Hence opt-in only.
template <bool METRICS, int W, int STORE_NT>
__global__ void __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_step_observe(DevCfg cfg, DevPtrs p, const int8_t* __restrict__ actions, float* __restrict__ rw32, double* __restrict__ rw64,
               uint8_t* __restrict__ done_out, uint32_t flags, uint8_t* __restrict__ obs, uint16_t* __restrict__ meta,
               uint32_t reverse_mask, uint32_t xcd_map, uint32_t* __restrict__ sync, int n_step, int n_tail, int tile0,
               uint64_t spin_ticks) {
    constexpr int EPW = WAVE / W;
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x;
    const int b = (int)blockIdx.x;
    if (b >= n_step && b < tile0) {
        if (b < n_step + n_tail) tail_block(cfg, p, b - n_step, lane, lds);  // (the rest pads the tiles' start to a multiple of 8)
        return;
    }
    // Every step and tile block counts itself on a shard once it has read seq — as its LAST instruction: an atomic is counted by
    // vmcnt, so one issued before the block's own loads would put its device-scope round trip in front of their first wait
    // (measured: 20 us of the 0.3 ms launch; sharding the count over 16 ... 1024 lines did not help).
    gu32_t* shard = (gu32_t*)(sync + CTF_SYNC_LINE * (1 + (b & (CTF_SYNC_SHARDS - 1))));
    if (b < n_step) {
        const uint32_t seq = __builtin_amdgcn_readfirstlane(ld_sc1(sync));
        step_block<METRICS, W, true>(cfg, p, actions, rw32, rw64, done_out, flags, b, lane, lds, StepPub{sync + CTF_SYNC_FLAGS, seq + 1u});
        if (b == 0) {
            // once every reader of seq has been counted (itself included): zero the counters and move to the next generation
            const uint32_t readers = (uint32_t)n_step + (gridDim.x - (uint32_t)tile0);
            if (lane == 0) __hip_atomic_fetch_add(shard, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t t0 = wall_clock64();
            for (;;) {
                __builtin_amdgcn_s_sleep(32);
                uint32_t n = 0;
#pragma unroll
                for (int k = 0; k < CTF_SYNC_SHARDS / WAVE; k++) n += ld_sc1(sync + CTF_SYNC_LINE * (1 + lane + WAVE * k));
#pragma unroll
                for (int o = WAVE / 2; o > 0; o >>= 1) n += (uint32_t)__shfl_xor((int)n, o, WAVE);
                if (__builtin_amdgcn_readfirstlane(n) == readers) break;
                if (wall_clock64() - t0 > 20 * spin_ticks) {  // (blocks not scheduled in index order: see CTF_ST_SYNC_TIMEOUT)
                    if (lane == 0) atomicOr(p.status, CTF_ST_SYNC_TIMEOUT);
                    break;
                }
            }
#pragma unroll
            for (int k = 0; k < CTF_SYNC_SHARDS / WAVE; k++) st_sc1(sync + CTF_SYNC_LINE * (1 + lane + WAVE * k), 0u);
            if (lane == 0) st_sc1(sync, seq + 1u);
            return;
        }
    } else {
        const uint32_t T = gridDim.x - (uint32_t)tile0, t = (uint32_t)(b - tile0);  // T: a multiple of 8
        const uint32_t lt = xcd_map ? (t & 7u) * (T >> 3) + (t >> 3) : t;
        tile_render<STORE_NT, true>(cfg, p, obs, meta, reverse_mask, lt / CTF_OBS_TILE_WPB, (int)(lt % CTF_OBS_TILE_WPB), lane, (uint8_t*)lds,
                                    TileWait{sync, __builtin_ctz(EPW), spin_ticks});
    }
    if (lane == 0) __hip_atomic_fetch_add(shard, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------
// compact observation: one byte per (agent, cell)
// ------------------------------------------------------------------------------------------------
// standardise_state's planes 1..C-1 are one-hot per cell (plane k+1 = (relabelled grid == TILES_USED[k]),
// gridworld_ctf.py:990-1001) and plane 0 has the single own-position bit, so a whole [C][G][G] block is carried by
// G*G bytes: codes[e][i][d] = index of the tile plane that is 1 at cell d of agent i's view (0 = none), bit 7 = plane 0.
// A policy that consumes the codes directly (ctf_policy.hip) never needs the 14x larger one-hot block.
// Per env a wave builds the (viewer team, reversed?) code maps that are in use (at most 4) in LDS; every agent's row is
// its map plus the own-position bit: an output dword is two aligned dwords of the map funnel-shifted (v_alignbyte_b32).
// The metadata rows leave in the same launch.  Per-wave LDS: see the size functions above k_observe.

template <bool DWORDS>
__global__ void __launch_bounds__(256) k_observe_codes(DevCfg cfg, DevPtrs p, uint8_t* __restrict__ codes,
                                                       uint16_t* __restrict__ meta, uint16_t* __restrict__ selfcells,
                                                       uint32_t reverse_mask) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int wpb = blockDim.x / WAVE;
    const int N = cfg.N, M = cfg.M, G = cfg.G, GG = cfg.GG, MS = codes_map_stride(GG);
    uint8_t* wl = (uint8_t*)lds + wave * codes_wave_bytes(cfg.GS, cfg.RS, GG, N, M);
    uint8_t* srec = wl;
    uint16_t* mv = (uint16_t*)(wl + cfg.RS);
    uint16_t* mstage = (uint16_t*)(wl + cfg.RS + OBS_MV_BYTES);
    uint8_t* mlut = wl + cfg.RS + OBS_MV_BYTES + obs_meta_stage_bytes(N, M);
    uint8_t* sgrid = mlut + obs_meta_lut_bytes(N, M);
    uint16_t* selfc = (uint16_t*)(sgrid + cfg.GS);
    uint8_t* maps = (uint8_t*)(selfc + 16);
    const ObsSlots slots = obs_slots(cfg, reverse_mask);
    uint32_t slot_pack = 0;  // 2 bits per agent
    for (int i = 0; i < N; i++) slot_pack |= (uint32_t)(cfg.team[i] * 2 + (int)((reverse_mask >> i) & 1u)) << (2 * i);
    if (meta) obs_meta_lut(cfg, mlut, mv, lane);
    const int row = N * GG;
    const int GW = cfg.GS / 4;
    const int rec_lane = min(lane, cfg.RS / 4 - 1), grid_lane = min(lane, GW - 1);
    const int e_first = blockIdx.x * wpb + wave, e_stride = gridDim.x * wpb;
    // a wave's envs are a dependent chain of load -> build -> store: the next env's state is loaded while this one is built
    uint32_t recw_n = 0, cells_n = 0;
    if (e_first < cfg.n_envs) {
        recw_n = ((const uint32_t*)(p.rec + (size_t)e_first * cfg.RS))[rec_lane];
        cells_n = ((const uint32_t*)(p.grid + (size_t)e_first * cfg.GS))[grid_lane];
    }
    for (int e = e_first; e < cfg.n_envs; e += e_stride) {
        const uint32_t recw = recw_n, cells = cells_n;
        const int e_next = min(e + e_stride, cfg.n_envs - 1);
        recw_n = ((const uint32_t*)(p.rec + (size_t)e_next * cfg.RS))[rec_lane];
        cells_n = ((const uint32_t*)(p.grid + (size_t)e_next * cfg.GS))[grid_lane];
        if (lane < GW) ((uint32_t*)sgrid)[lane] = cells;
        for (int w = lane + WAVE; w < GW; w += WAVE) ((uint32_t*)sgrid)[w] = ((const uint32_t*)(p.grid + (size_t)e * cfg.GS))[w];  // G > 16
        // parks the record in LDS and, when asked for, writes this env's metadata rows
        obs_build_env(cfg, p, e, recw, 0u, srec, mv, mstage, mlut, nullptr, slots, reverse_mask, lane, false, meta);
        if (!codes && !selfcells) continue;
        if (lane < N) {
            const int8_t* ps = (const int8_t*)(srec + cfg.off_pos);
            const int r = ps[2 * lane], c = ps[2 * lane + 1];
            const uint16_t sc = (uint16_t)(((reverse_mask >> lane) & 1u) ? flip_cell(cfg, r * G + c, r, c) : r * G + c);
            selfc[lane] = sc;
            if (selfcells) selfcells[(size_t)e * N + lane] = sc;  // where bit 7 sits in this agent's row
        }
        if (!codes) continue;
#pragma unroll
        for (int slot = 0; slot < 4; slot++) {
            if (!slots.a[slot]) continue;  // uniform
            const uint64_t lut = pin64(cfg.chan_lut[slot >> 1]);
            for (int d = lane; d < GG; d += WAVE) {
                const int r = (int)fdiv((uint32_t)d, cfg.div_g), c = d - r * G;
                const int src = (slot & 1) ? flip_cell(cfg, d, r, c) : d;  // every flip is an involution
                const uint32_t v = sgrid[src];
                uint32_t code = (((v & 8u) ? (uint32_t)(lut >> 32) : (uint32_t)lut) >> (4 * (v & 7u))) & 15u;
                if (v == 0 || code == CTF_TILE_NONE) code = 0;
                maps[slot * MS + d] = (uint8_t)code;
            }
        }
        __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
        __builtin_amdgcn_wave_barrier();
        uint8_t* out = codes + (size_t)e * row;
        for (int q = lane; q < (row + 3) / 4; q += WAVE) {
            const int f0 = 4 * q;
            const int i0 = (int)fdiv((uint32_t)f0, cfg.div_gg_row), d0 = f0 - i0 * GG;
            if (DWORDS) {
                // bytes d0 .. d0 + 3 of agent i0's row: two aligned dwords of its map, funnel-shifted (past the row's end the
                // map's padding shows up and is masked off below)
                const uint32_t* m32 = (const uint32_t*)(maps + ((slot_pack >> (2 * i0)) & 3u) * MS);
                uint32_t word = __builtin_amdgcn_alignbyte(m32[(d0 >> 2) + 1], m32[d0 >> 2], (uint32_t)(d0 & 3));
                const uint32_t sd = (uint32_t)((int)selfc[i0] - d0);
                if (sd < 4u) word |= 0x80u << (8 * sd);
                const int nb = GG - d0;  // bytes left in this agent's row
                if (nb < 4) {            // the dword runs into the next agent's row (never past the env: N * GG is a multiple of 4)
                    const int i1 = i0 + 1;
                    uint32_t nxt = *(const uint32_t*)(maps + ((slot_pack >> (2 * i1)) & 3u) * MS);
                    const uint32_t s1 = selfc[i1];
                    if (s1 < (uint32_t)(4 - nb)) nxt |= 0x80u << (8 * s1);
                    word = (word & ((1u << (8 * nb)) - 1u)) | (nxt << (8 * nb));
                }
                ((uint32_t*)out)[q] = word;
            } else {
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int f = f0 + b;
                    if (f < row) {
                        const int i = (d0 + b >= GG) ? i0 + 1 : i0, d = (d0 + b >= GG) ? d0 + b - GG : d0 + b;
                        uint32_t v = maps[((slot_pack >> (2 * i)) & 3u) * MS + d];
                        if (d == (int)selfc[i]) v |= 0x80u;
                        out[f] = (uint8_t)v;
                    }
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------------
// bulk export of the evaluation counters
// ------------------------------------------------------------------------------------------------
extern "C" __global__ void k_export_counters(DevCfg cfg, DevPtrs p, int32_t* metrics, int32_t* captures, int32_t* steps) {
    const int MN = CTF_N_METRICS * cfg.N;
    const size_t total = (size_t)cfg.n_envs * MN;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        if (metrics) metrics[idx] = cfg.log_metrics ? p.metrics[idx] : 0;
        if (idx < (size_t)cfg.n_envs) {
            const int32_t* misc = (const int32_t*)(p.rec + idx * cfg.RS + cfg.off_misc);
            if (captures) { captures[2 * idx] = misc[1]; captures[2 * idx + 1] = misc[2]; }
            if (steps) steps[idx] = misc[0];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// synthetic actions: Philox4x32-10 (Salmon et al. 2011), one lane per (env, block of 8 agents)
// ------------------------------------------------------------------------------------------------
extern "C" __global__ void k_random_actions(DevCfg cfg, int8_t* actions, uint64_t seed, uint32_t step, uint32_t env_offset) {
    const int nblk = (cfg.N + 7) / 8;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= cfg.n_envs * nblk) return;
    const int e = idx / nblk, blk = idx - e * nblk;
    uint32_t c0 = env_offset + (uint32_t)e, c1 = step, c2 = (uint32_t)blk, c3 = 0;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const uint32_t w[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (blk * 8 + j < cfg.N) {
            const uint32_t h = (w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
            actions[(size_t)e * cfg.N + blk * 8 + j] = (int8_t)((h * 9u) >> 16);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// launchers (ctf_launch.h; called from ctf_abi.hip)
// ------------------------------------------------------------------------------------------------
// (env_int, obs_xcd_knob, obs_waves_per_block — the knobs the retained render's launcher reads too: ctf_render_dev.h)
static int obs_reserve_blocks() {  // read once
    static const int v = env_int("CTF_OBS_RESERVE_BLOCKS", 0);
    return v < 0 ? 0 : v;
}
// (with_bool / with_step_variant, run-time switches -> template arguments: ctf_step_block.h)

extern "C" hipError_t ctf_launch_reset(const DevCfg& cfg, const DevPtrs& p, const uint8_t* mask, int init_perm, hipStream_t st) {
    hipLaunchKernelGGL(k_reset, dim3(cfg.n_envs), dim3(WAVE), 0, st, cfg, p, mask, init_perm);
    return hipGetLastError();
}
// lanes per env: the power of two that covers the larger opponents list (<= 8), so one tag pass per agent turn — and more
// (up to 8) as long as the waves that makes stay within 8 per CU (half of what is resident at once): fewer envs per wave then,
// i.e. a shorter divergent chain per wave (0_the_split at 4 096 envs: 2 -> 8 lanes, 0.0312 -> 0.0280 ms per env-step; the whole
// table, every width at 4 096 .. 131 072 envs of both workloads: profiles/r05_step_lanes_sweep.txt).  Results do not depend on it.
static int step_lanes(const DevCfg& cfg) {
    const int mo = cfg.n_opp[0] > cfg.n_opp[1] ? cfg.n_opp[0] : cfg.n_opp[1];
    int w = mo <= 1 ? 1 : (mo <= 2 ? 2 : (mo <= 4 ? 4 : 8));
    while (w < 8 && (long long)cfg.n_envs * (2 * w) / WAVE <= 8LL * cfg.n_cus) w *= 2;
    if (cfg.step_lanes_override) w = cfg.step_lanes_override;  // profiling / test knob (CTF_STEP_W)
    return w;
}
// The step part of a grid of one-wave blocks: nstep step blocks (WAVE / w envs each), then ntail ring-regenerating blocks, and
// the dynamic LDS they need.  A tail block stages two rings (4 992 bytes), which is MORE than the step blocks' slots whenever
// w = 8 meets a small grid (8 slots of GS + RS + 128 bytes or so), so whether that floor holds WITHOUT tail blocks
// (CTF_RNG_REFILL_EVERY=0) changes the launch: k_step has always taken it then, k_step_observe never.  Nothing reads the extra
// bytes; both are kept as they were (`tail_lds_always`) because this shape is compared launch for launch with its history.
struct StepShape {
    int nstep, ntail;
    size_t lds;
};
static StepShape step_shape(const DevCfg& cfg, int w, bool metrics, bool with_tail, bool tail_lds_always) {
    const int epw = WAVE / w;
    StepShape s;
    s.nstep = (cfg.n_envs + epw - 1) / epw;
    s.ntail = with_tail ? (2 * cfg.n_envs + STEP_TAIL_PAIRS - 1) / STEP_TAIL_PAIRS : 0;
    s.lds = (size_t)epw * step_slot_bytes(cfg.GS, cfg.RS, cfg.N, metrics);
    if ((s.ntail || tail_lds_always) && s.lds < 2 * CTF_MT_N * 4) s.lds = 2 * CTF_MT_N * 4;
    return s;
}
extern "C" int ctf_step_blocks(const DevCfg& cfg) { return step_shape(cfg, step_lanes(cfg), cfg.log_metrics != 0, false, false).nstep; }
// with_tail: the ring regeneration rides at the tail of this launch.  Nothing in the launch depends on how many went before it
// (see tail_block), so a captured launch can be replayed.
extern "C" hipError_t ctf_launch_step(const DevCfg& cfg, const DevPtrs& p, const StepArgs& a, int with_tail, hipStream_t st) {
    const int w = step_lanes(cfg);
    if (cfg.rng_mode == CTF_RNG_COUNTER_DIRECT) {  // no rings: no tail blocks, and no LDS floor of two rings (ctf_step_direct.hip)
        const StepShape s = step_shape(cfg, w, cfg.log_metrics != 0, false, false);
        return ctf_launch_step_direct(cfg, p, a, w, s.nstep, s.lds, st);
    }
    const StepShape s = step_shape(cfg, w, cfg.log_metrics != 0, with_tail && cfg.rng_refill_every, true);
    with_step_variant(cfg.log_metrics != 0, w, [&](auto M, auto W) {
        with_bool(a.meta != nullptr, [&](auto META) {
            hipLaunchKernelGGL((k_step<M.value, W.value, META.value>), dim3(s.nstep + s.ntail), dim3(WAVE), s.lds, st, cfg, p, a.actions, a.rw32,
                               a.rw64, a.done, a.flags, s.nstep, step_meta(cfg, a));
        });
    });
    return hipGetLastError();
}
#if STEP_TRACE
// what the runtime thinks fits: blocks of k_step<true, 4> per CU at `lds` bytes of dynamic LDS, and the device's LDS per CU
extern "C" int ctf_debug_step_occupancy(int lds, int* blocks_per_cu, int* lds_per_cu, int* lds_per_block) {
    hipDeviceProp_t prop;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 1;
    *lds_per_cu = (int)prop.maxSharedMemoryPerMultiProcessor;
    *lds_per_block = (int)prop.sharedMemPerBlock;
    return (int)hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k_step<true, 4, false>, WAVE, (size_t)lds);
}
#endif
static int observe_align(const DevCfg& cfg, const uint8_t* obs) {
    const uintptr_t a = (uintptr_t)obs;
    return ((cfg.obs_bytes % 16) == 0 && (a % 16) == 0) ? 16 : (((cfg.obs_bytes % 4) == 0 && (a % 4) == 0) ? 4 : 1);
}
// the one rule by which a render into `obs` is the tile kernel (1) or the wave-per-env kernel (0); CTF_OBS_TILES = 0 / 1: never /
// whenever possible (tests, profiling)
extern "C" int ctf_observe_uses_tiles(const DevCfg& cfg, const uint8_t* obs) {
    return obs && observe_align(cfg, obs) == 16 && cfg.tile_k > 0 && env_int("CTF_OBS_TILES", OBS_TILES_DEFAULT) != 0;
}
// the one rule by which ctf_step_observe is one launch (1: k_step_observe) or two (0): where the tile render applies and it is
// asked for (CTF_STEP_OBSERVE_ONE_LAUNCH = 0 / 1: never / whenever possible).  CTF_RNG_COUNTER_DIRECT has no one-launch form.
extern "C" int ctf_step_observe_one_launch(const DevCfg& cfg, const uint8_t* obs) {
    return cfg.rng_mode != CTF_RNG_COUNTER_DIRECT && ctf_observe_uses_tiles(cfg, obs) && env_int("CTF_STEP_OBSERVE_ONE_LAUNCH", STEP_OBSERVE_ONE_LAUNCH_DEFAULT) != 0;
}
// k_step_observe (the launch's shape: see the kernel)
extern "C" hipError_t ctf_launch_step_observe(const DevCfg& cfg, const DevPtrs& p, const StepArgs& a, const RenderArgs& r, hipStream_t st) {
    const int w = step_lanes(cfg);
    const StepShape s = step_shape(cfg, w, cfg.log_metrics != 0, cfg.rng_refill_every != 0, false);
    const int tile0 = (s.nstep + s.ntail + 7) / 8 * 8;
    const int ntiles = cfg.tile_nb * CTF_OBS_TILE_WPB;
    const size_t tile_lds = (size_t)tiles_wave_bytes(cfg.RS, cfg.N, cfg.M);
    const size_t sh = s.lds < tile_lds ? tile_lds : s.lds;
    const uint32_t xcd_map = obs_xcd_knob();
    with_step_variant(cfg.log_metrics != 0, w, [&](auto M, auto W) {
        with_bool(cfg.obs_store_nt != 0, [&](auto NT) {
            hipLaunchKernelGGL((k_step_observe<M.value, W.value, NT.value>), dim3((unsigned)(tile0 + ntiles)), dim3(WAVE), sh, st, cfg, p, a.actions,
                               a.rw32, a.rw64, a.done, a.flags, r.obs, r.meta, r.reverse_mask, xcd_map, r.sync, s.nstep, s.ntail, tile0,
                               r.spin_ticks);
        });
    });
    return hipGetLastError();
}
extern "C" hipError_t ctf_launch_observe(const DevCfg& cfg, const DevPtrs& p, const RenderArgs& r, int n_cus, hipStream_t st) {
    if (ctf_observe_uses_tiles(cfg, r.obs)) {
        // one wave per tile, CTF_OBS_TILE_WPB independent waves per block; tile_bx blocks per group of tile_k envs (whose blocks fill
        // tile_tpg tiles)
        const int wpb = CTF_OBS_TILE_WPB;
        size_t sh = (size_t)wpb * tiles_wave_bytes(cfg.RS, cfg.N, cfg.M);
        // At most 16 tile waves per CU, by the block's LDS (160 KiB per CU): fewer store streams in flight write the buffer
        // faster.  In one process on one buffer (8_arena, 65 536 envs) the render took 0.2353 ms this way, 0.2443 ms as one-wave
        // blocks without the cap and 0.2472 ms as the earlier blocks of 4 tiles; step + render 0.2790 / 0.2932 / 0.2980 ms
        // (profiles/r06_render_occupancy_cap.txt).
        if (sh < OBS_TILE_BLOCK_LDS) sh = OBS_TILE_BLOCK_LDS;
        const uint32_t xcd_map = obs_xcd_knob();
        with_bool(cfg.obs_store_nt != 0, [&](auto NT) {
            hipLaunchKernelGGL(k_observe_tiles<NT.value>, dim3((unsigned)cfg.tile_nb), dim3(wpb * WAVE), sh, st, cfg, p, r.obs, r.meta, r.reverse_mask,
                               xcd_map);
        });
        return hipGetLastError();
    }
    const int per_wave = obs_wave_bytes(cfg.RS, cfg.N, cfg.M, cfg.obs_bytes);
    const int wpb = obs_waves_per_block(per_wave);
    const size_t sh = (size_t)wpb * per_wave;
    int blocks = (cfg.n_envs + wpb - 1) / wpb;
    // the CU's 32-wave limit, grid-stride beyond that; a few block slots stay free so that a concurrent small kernel
    // (the RCCL all-gather of the rollout tensors) can start beside this launch instead of behind it
    int cap = n_cus * (32 / wpb);
    const int per_cu = env_int("CTF_OBS_BLOCKS_PER_CU", 0);  // profiling only: occupancy scaling of the render
    if (per_cu >= 1 && per_cu < 32 / wpb) cap = n_cus * per_cu;
    if (cap > 64) cap -= obs_reserve_blocks();
    if (blocks > cap) blocks = cap;
    const dim3 grid(blocks), block(wpb * WAVE);
    const uint32_t xcd_map = (blocks % 8 == 0 && obs_xcd_knob()) ? 1u : 0u;
    const int align = observe_align(cfg, r.obs);
    if (align == 16) hipLaunchKernelGGL(k_observe<16>, grid, block, sh, st, cfg, p, r.obs, r.meta, r.reverse_mask, xcd_map);
    else if (align == 4) hipLaunchKernelGGL(k_observe<4>, grid, block, sh, st, cfg, p, r.obs, r.meta, r.reverse_mask, xcd_map);
    else hipLaunchKernelGGL(k_observe<1>, grid, block, sh, st, cfg, p, r.obs, r.meta, r.reverse_mask, xcd_map);
    return hipGetLastError();
}
extern "C" hipError_t ctf_launch_observe_codes(const DevCfg& cfg, const DevPtrs& p, uint8_t* codes, uint16_t* meta, uint16_t* selfcells,
                                               uint32_t reverse_mask, int n_cus, hipStream_t st) {
    const int per_wave = codes_wave_bytes(cfg.GS, cfg.RS, cfg.GG, cfg.N, cfg.M);
    const int wpb = obs_waves_per_block(per_wave);
    const size_t sh = (size_t)wpb * per_wave;
    int blocks = (cfg.n_envs + wpb - 1) / wpb;
    if (blocks > n_cus * 8) blocks = n_cus * 8;
    with_bool(((cfg.N * cfg.GG) % 4) == 0 && ((uintptr_t)codes % 4) == 0, [&](auto DWORDS) {
        hipLaunchKernelGGL(k_observe_codes<DWORDS.value>, dim3(blocks), dim3(wpb * WAVE), sh, st, cfg, p, codes, meta, selfcells, reverse_mask);
    });
    return hipGetLastError();
}
extern "C" hipError_t ctf_launch_export_counters(const DevCfg& cfg, const DevPtrs& p, int32_t* metrics, int32_t* captures, int32_t* steps,
                                                 hipStream_t st) {
    const size_t total = (size_t)cfg.n_envs * CTF_N_METRICS * cfg.N;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_export_counters, dim3(blocks), dim3(256), 0, st, cfg, p, metrics, captures, steps);
    return hipGetLastError();
}
extern "C" hipError_t ctf_launch_random_actions(const DevCfg& cfg, int8_t* actions, uint64_t seed, uint32_t step,
                                                uint32_t env_offset, hipStream_t st) {
    const int n = cfg.n_envs * ((cfg.N + 7) / 8);
    hipLaunchKernelGGL(k_random_actions, dim3((n + 255) / 256), dim3(256), 0, st, cfg, actions, seed, step, env_offset);
    return hipGetLastError();
}
