// ctf_ring_dev.h — ring regeneration by ONE WAVE (ctf_mt.h): device code shared by the tail blocks of k_step / k_step_observe
// (ctf_kernels.hip) and by k_rng_refill (ctf_rng.hip).  Wavefront = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>

#include "ctf_step_core.h"

#define WAVE 64

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
#define RNG_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_s_waitcnt(0xC07F); \
        __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
// ---- the digests of ctf_mt.h as ONE WAVE makes them, from a block's OUTPUT words (tempered, or as they are in counter mode) in
// LDS: the hit bits of 64 positions are one ballot, a nibble / top-byte dword is a handful of LDS reads.  (ring_digest /
// ring_link in ctf_mt.h are the same arithmetic one word at a time: the step kernel's safety net and the host simulator use
// those, and tests run both against each other through CTF_RNG_REFILL_EVERY.)
__device__ __forceinline__ void wave_digest(int lane, const uint32_t* T, const RingPtrs& p, int r, const RingParams& q) {
    if (q.stream == 1) {
        uint32_t* hit = p.hit + r * CTF_HB_DW;
        uint32_t t0[10], t1[10];
#pragma unroll
        for (int c = 0; c < 10; c++) {  // 624 positions = 10 x 64 (the last 16 lanes of the last pass idle): the reads first
            const int i = 64 * c + lane;
            t0[c] = T[i < CTF_MT_N ? i : 0];
            t1[c] = T[i + 1 < CTF_MT_N ? i + 1 : 0];
        }
#pragma unroll
        for (int c = 0; c < 10; c++) {
            const int i = 64 * c + lane;
            const unsigned long long m = __ballot(i < CTF_MT_N - 1 && mt_lt53(t0[c] >> 5, t1[c] >> 6, q.th, q.tl));
            if (lane < 2 && 2 * c + lane < (CTF_MT_N + 31) / 32) hit[2 * c + lane] = (uint32_t)(m >> (32 * lane));
        }
        uint32_t* nib = p.nib + r * CTF_NB_DW;
        const u32x4_t* T4 = (const u32x4_t*)T;
#pragma unroll
        for (int it = 0; it < 2; it++) {  // 78 dwords of 8 nibbles
            const int d = lane + 64 * it;
            if (d < CTF_MT_N / 8) {
                const u32x4_t a = T4[2 * d], b = T4[2 * d + 1];
                nib[d] = (a.x & 15u) | ((a.y & 15u) << 4) | ((a.z & 15u) << 8) | ((a.w & 15u) << 12) | ((b.x & 15u) << 16) | ((b.y & 15u) << 20) |
                         ((b.z & 15u) << 24) | ((b.w & 15u) << 28);
            }
        }
    } else {
        uint32_t* top = p.top + r * CTF_P8_DW;
        const u32x4_t* T4 = (const u32x4_t*)T;
#pragma unroll
        for (int it = 0; it < 3; it++) {  // 156 dwords of 4 top bytes
            const int d = lane + 64 * it;
            if (d < CTF_MT_N / 4) {
                const u32x4_t a = T4[d];
                top[d] = (a.x >> 24) | ((a.y >> 24) << 8) | ((a.z >> 24) << 16) | ((a.w >> 24) << 24);
            }
        }
    }
}
// Tc: outputs of ring c (only words 608 .. 623 are read), To: outputs of its successor ring
__device__ __forceinline__ void wave_link(int lane, const uint32_t* Tc, const uint32_t* To, const RingPtrs& p, int c, const RingParams& q) {
    if (q.stream == 1) {
        uint32_t* hc = p.hit + c * CTF_HB_DW;
        constexpr int P0 = (CTF_MT_N >> 5) * 32;  // 608: the first position of dword 19
        uint32_t w0[4], w1[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {  // positions 608 .. 863, counted from ring c's start (dwords 19 .. 26: the array ends at 25)
            const int pc = P0 + 64 * k + lane;
            w0[k] = pc < CTF_MT_N ? Tc[pc] : To[pc - CTF_MT_N];
            w1[k] = pc + 1 < CTF_MT_N ? Tc[pc + 1] : To[pc + 1 - CTF_MT_N];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned long long m = __ballot(mt_lt53(w0[k] >> 5, w1[k] >> 6, q.th, q.tl));
            const int d = (CTF_MT_N >> 5) + 2 * k + lane;
            if (lane < 2 && d < CTF_HB_DW) hc[d] = (uint32_t)(m >> (32 * lane));
        }
        uint32_t* nc = p.nib + c * CTF_NB_DW;
        if (lane < CTF_NB_MIRROR / 8) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) v |= (To[8 * lane + k] & 15u) << (4 * k);
            nc[CTF_MT_N / 8 + lane] = v;
        }
    } else {
        uint32_t* tc = p.top + c * CTF_P8_DW;
        if (lane < CTF_P8_MIRROR / 4) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) v |= (To[4 * lane + k] >> 24) << (8 * k);
            tc[CTF_MT_N / 4 + lane] = v;
        }
    }
}
// the block after `src` into `dst` (both LDS) by one wave: ring_next_block of ctf_mt.h with the three dependent chunks unrolled, every
// chunk's LDS reads issued before its arithmetic
__device__ __forceinline__ void wave_next_block(int lane, const uint32_t* src, uint32_t* dst, const RingParams& q) {
    if (q.counter_mode) {
#pragma unroll 1
        for (int b = lane; b < CTF_MT_N / 4; b += WAVE) {
            uint32_t o[4];
            ctr_block(q.seed, (q.nbase + CTF_MT_N) / 4 + (unsigned long long)b, (uint32_t)q.stream, o);
            ((u32x4_t*)dst)[b] = u32x4_t{o[0], o[1], o[2], o[3]};
        }
        RNG_WAVE_SYNC();
        return;
    }
    constexpr int M = CTF_MT_N - 397;  // 227
#pragma unroll
    for (int chunk = 0; chunk < 3; chunk++) {
        const int lo = chunk * M, hi = chunk == 2 ? CTF_MT_N - 1 : lo + M;  // [0, 227), [227, 454), [454, 623)
        uint32_t x0[4], x1[4], m[4];
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int i = lo + lane + 64 * it, ic = i < hi ? i : lo;
            x0[it] = src[ic];
            x1[it] = src[ic + 1];
            m[it] = chunk == 0 ? src[ic + 397] : dst[ic - M];
        }
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const int i = lo + lane + 64 * it;
            if (i < hi) dst[i] = mt_twist(x0[it], x1[it], m[it]);
        }
        if (chunk == 2 && lane == 0) dst[CTF_MT_N - 1] = mt_twist(src[CTF_MT_N - 1], dst[0], dst[396]);
        RNG_WAVE_SYNC();
    }
}

// One ring, one wave: the ring the consumer has left becomes the block after the current one, with its digests, and the current
// ring is linked to it (mirror, hit bit of its last position).  src / dst: 2 x 624 words of the wave's LDS.  `init`: the CURRENT
// ring's digests are made too (after a seed or a state import).  2.5 KB read, 2.5 KB + the digests written, every access of the
// wave contiguous.
// (CTF_STAMP: nothing, except in a -DSTEP_TRACE build of ctf_kernels.hip — of a tail block's LAST ring, tools/trace_step.py)
#define RING_STAMP(k) CTF_STAMP(k)
// the ring's words on their way into the wave (issued early: the previous ring of the same tail block is still being worked on)
struct RingIn {
    StreamFull st;
    u32x4_t a, b, c;
};
__device__ __forceinline__ RingIn ring_fetch(const DevCfg& cfg, const DevPtrs& p, int e, int stream, uint32_t flag, int lane) {
    RingIn in;
    in.st.r = ring_ptrs(p, e, stream);
    in.st.q = ring_params(cfg, p, e, stream);
    // The flag says which ring is stale (the position word may be moving); only an init pass (flag 0) has to read the position word —
    // the branch is uniform, and without it every regeneration would wait for that load before it can even address its ring: one
    // more dependent memory round trip on a 5.65 us job.
    const uint32_t uflag = (uint32_t)__builtin_amdgcn_readfirstlane((int)flag);  // (the same in every lane: one ring per wave)
    if (uflag >= 2u) in.st.cur = 1u - (uflag - 2u);
    else in.st.cur = ring_source(uflag, p.rngpos[2 * (size_t)e + stream]);
    ring_counter_params(in.st.q, p, e, stream, in.st.cur);
    const u32x4_t* gsrc = (const u32x4_t*)(in.st.r.raw + in.st.cur * CTF_MT_N);
    constexpr int NQ = CTF_MT_N / 4;  // 156 quads: two full passes of the wave and 28 lanes of a third
    in.a = gsrc[lane];
    in.b = gsrc[lane + WAVE];
    in.c = gsrc[lane + 2 * WAVE < NQ ? lane + 2 * WAVE : 0];
    return in;
}
__device__ __forceinline__ void refill_ring(const DevCfg& cfg, const DevPtrs& p, int e, int stream, const RingIn& in, int lane, uint32_t* src,
                                            uint32_t* dst, bool init) {
    StreamFull st = in.st;
    u32x4_t* gdst = (u32x4_t*)(st.r.raw + (1 - st.cur) * CTF_MT_N);
    constexpr int NQ = CTF_MT_N / 4;
    ((u32x4_t*)src)[lane] = in.a;
    ((u32x4_t*)src)[lane + WAVE] = in.b;
    if (lane + 2 * WAVE < NQ) ((u32x4_t*)src)[lane + 2 * WAVE] = in.c;
    RING_STAMP(10);
    RNG_WAVE_SYNC();
    wave_next_block(lane, src, dst, st.q);
    RING_STAMP(11);
    {   // the new block's raw words leave; both LDS copies then become OUTPUT words (of ring c only what is looked at)
        u32x4_t v[3];
#pragma unroll
        for (int it = 0; it < 3; it++) v[it] = ((const u32x4_t*)dst)[lane + WAVE * it < NQ ? lane + WAVE * it : 0];
#pragma unroll
        for (int it = 0; it < 3; it++) {
            const int d = lane + WAVE * it;
            if (d < NQ) {
                gdst[d] = v[it];
                ((u32x4_t*)dst)[d] = u32x4_t{ring_out(st.q, v[it].x), ring_out(st.q, v[it].y), ring_out(st.q, v[it].z), ring_out(st.q, v[it].w)};
            }
        }
        if (init) {
#pragma unroll
            for (int it = 0; it < 3; it++) {
                const int d = lane + WAVE * it;
                if (d < NQ) {
                    const u32x4_t w = ((const u32x4_t*)src)[d];
                    ((u32x4_t*)src)[d] = u32x4_t{ring_out(st.q, w.x), ring_out(st.q, w.y), ring_out(st.q, w.z), ring_out(st.q, w.w)};
                }
            }
        } else if (lane < 16) {
            src[(CTF_MT_N >> 5) * 32 + lane] = ring_out(st.q, src[(CTF_MT_N >> 5) * 32 + lane]);
        }
    }
    RNG_WAVE_SYNC();
    RING_STAMP(12);
    if (init) wave_digest(lane, src, st.r, (int)st.cur, st.q);
    wave_digest(lane, dst, st.r, 1 - (int)st.cur, st.q);
    RING_STAMP(13);
    wave_link(lane, src, dst, st.r, (int)st.cur, st.q);
    RING_STAMP(14);
    if (lane == 0) {
        ring_counter_store(st.q, p, e, stream, 1u - st.cur);
        p.rngready[2 * (size_t)e + stream] = 1;
    }
    RNG_WAVE_SYNC();  // the LDS copies are reused by the wave's next ring
}
