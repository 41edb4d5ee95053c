// ctf_render_dev.h — what more than one render uses: the per-wave LDS sizes, the bit expansion, the flips, the metadata LUT and
// obs_build_env (an env's bitmap and metadata rows), and the host knobs both launch layers read.  Shared by the full renders
// (k_observe, k_observe_tiles / k_step_observe, k_observe_codes: ctf_kernels.hip) and the retained render (ctf_observe_delta.hip).
// Wavefront = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "ctf_ring_dev.h"    // WAVE, u32x4_t (and through it ctf_step_core.h: fdiv, pin64, the cfg lookups)
#include "ctf_meta.h"        // the metadata values and f64_to_f16
#include "ctf_step_block.h"  // with_bool

// ---- The per-wave LDS of the three full renders (bytes).  Each kernel carves its own up by these sizes, in this order:
//   k_observe        [rec RS][mvals 96][meta staging][meta source LUT][bitmap]
//   k_observe_codes  [rec RS][mvals 96][meta staging][meta source LUT][grid GS][self cell u16[16]][maps 4 x (GGp + 4)]
//   tile_render      [bitmap TILE / 8][rec RS][mvals 96][meta staging]          (its LUT is the host-built table in global memory)
// (the retained render's: ctf_observe_delta.hip)
#define OBS_MV_BYTES 96
#define OBS_TILE CTF_OBS_TILE
__host__ __device__ inline int obs_meta_stage_bytes(int N, int M) { return (N * M * 2 + 15) & ~15; }
__host__ __device__ inline int obs_bitmap_bytes(int obs_bytes) { return ((((obs_bytes + 31) / 32 + 1) * 4) + 15) & ~15; }
__host__ __device__ inline int obs_meta_lut_bytes(int N, int M) { return (N * M + 15) & ~15; }
__host__ __device__ inline int codes_map_stride(int GG) { return ((GG + 3) & ~3) + 4; }  // + 4: the funnel read's second dword
__host__ __device__ inline int obs_wave_bytes(int RS, int N, int M, int obs_bytes) {
    return RS + OBS_MV_BYTES + obs_meta_stage_bytes(N, M) + obs_meta_lut_bytes(N, M) + obs_bitmap_bytes(obs_bytes);
}
__host__ __device__ inline int codes_wave_bytes(int GS, int RS, int GG, int N, int M) {
    return RS + OBS_MV_BYTES + obs_meta_stage_bytes(N, M) + obs_meta_lut_bytes(N, M) + GS + 32 + 4 * codes_map_stride(GG);
}
__host__ __device__ inline int tiles_wave_bytes(int RS, int N, int M) {
    return OBS_TILE / 8 + RS + OBS_MV_BYTES + obs_meta_stage_bytes(N, M);
}

#define LGKM_ONLY 0xC07F  // s_waitcnt lgkmcnt(0): LDS traffic only — never drain the wave's outstanding stores
// Profiling-only ablations (never defined in the shipped build; see tools/ablate.sh):
//   bit0 no bit expansion, bit1 no chunk stores, bit2 no bitmap build, bit3 no metadata, bit4 metadata computed but not stored,
//   bit5 k_observe_delta's dirty-line list not compacted from the mask: an identity list of the same length (the wrong lines)
#ifndef OBS_ABLATE
#define OBS_ABLATE 0
#endif

template <int ALIGN>
struct OutVec;
template <>
struct OutVec<16> { typedef uint32_t type __attribute__((ext_vector_type(4))); };
template <>
struct OutVec<4> { typedef uint32_t type __attribute__((ext_vector_type(4), aligned(4))); };
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int flip_cell(const DevCfg& cfg, int cell, int r, int c) {
    // destination of cell (r, c) under reverse_grid (gridworld_ctf.py:1003-1007)
    const int G = cfg.G;
    if (cfg.flip_axis == -1) return cfg.GG - 1 - cell;      // np.flip over both axes
    if (cfg.flip_axis == 0) return (G - 1 - r) * G + c;     // np.flip(plane, 0)
    if (cfg.flip_axis == 1) return r * G + (G - 1 - c);     // np.flip(plane, 1)
    return (G - 1 - c) * G + (G - 1 - r);                   // np.rot90(plane.T, 2)
}

// 4 bits -> 4 bytes of 0/1: the four shifted copies of the nibble do not overlap, so no carries
__device__ __forceinline__ uint32_t expand4(uint32_t h, int j) {
    return (((h >> (4 * j)) & 15u) * 0x00204081u) & 0x01010101u;
}

struct ObsSlots {  // which agents look through each (viewer team, reversed?) view — uniform over the launch
    uint32_t a[4];
};
__device__ __forceinline__ ObsSlots obs_slots(const DevCfg& cfg, uint32_t reverse_mask) {
    ObsSlots s = {{0, 0, 0, 0}};
    for (int i = 0; i < cfg.N; i++) {
        const int sl = cfg.team[i] * 2 + (int)((reverse_mask >> i) & 1u);
        s.a[0] |= (sl == 0) ? (1u << i) : 0u;
        s.a[1] |= (sl == 1) ? (1u << i) : 0u;
        s.a[2] |= (sl == 2) ? (1u << i) : 0u;
        s.a[3] |= (sl == 3) ? (1u << i) : 0u;
    }
    return s;
}

// Which of the (at most 36 distinct + two constant) values mv[] each element of the N x M metadata block shows
// (gridworld_ctf.py:1044-1067): mv[0] step fraction, mv[1 + t] capture ratio for a viewer of team t, mv[4 + j] the
// uint8-truncated hp of agent j, mv[20 + j] has_flag[j], mv[40] = 1.0, mv[41] = 0.0.
__device__ __forceinline__ void obs_meta_lut(const DevCfg& cfg, uint8_t* mlut, uint16_t* mv, int lane) {
    const int N = cfg.N, M = cfg.M;
    for (int idx = lane; idx < N * M; idx += WAVE) {
        const int i = (int)fdiv((uint32_t)idx, cfg.div_m), k = idx - i * M;
        const int team = cfg_team(cfg, i);
        int src = 41;
        if (k == 0) src = 0;
        else if (k == 1) src = 1 + team;
        else if (k < 6) src = (k - 2 == cfg_type(cfg, i)) ? 40 : 41;
        else {
            // rows 6,7: the agent itself; then own-team list minus self, then the opponents list (:1053-1067)
            int who = i;
            if (k >= 8) {
                const int pidx = (k - 8) >> 1;
                const int n_own = cfg_nopp(cfg, 1 - team), n_op = cfg_nopp(cfg, team);
                const int self_idx = (int)((pin64(cfg.self_idx_pack) >> (4 * i)) & 15u);
                const int n_mates = n_own - (self_idx < n_own ? 1 : 0);
                if (pidx < n_mates) who = cfg_opp(cfg, 1 - team, pidx + (pidx >= self_idx ? 1 : 0));
                else if (pidx - n_mates < n_op) who = cfg_opp(cfg, team, pidx - n_mates);
                else who = -1;
            }
            if (who >= 0) src = ((k & 1) ? 20 : 4) + who;
        }
        mlut[idx] = (uint8_t)src;
    }
    if (lane == 0) { mv[40] = 0x3C00u; mv[41] = 0u; }
}

// Everything of one env except the streaming: bitmap (zero + hot bits + own-position bits) into `bits`, metadata rows
// to global memory.  `recw` / `cells` are the lane's dword of the env's record / grid (lane-clamped loads).
// srec / mv / mstage are the calling wave's scratch.  Ends with the wave's LDS traffic drained.
__device__ __forceinline__ void obs_build_env(const DevCfg& cfg, const DevPtrs& p, int e, uint32_t recw, uint32_t cells,
                                              uint8_t* srec, uint16_t* mv, uint16_t* mstage, const uint8_t* mlut, uint32_t* bits,
                                              const ObsSlots& slots, uint32_t reverse_mask, int lane, bool obs,
                                              uint16_t* __restrict__ meta) {
    const int N = cfg.N, G = cfg.G, GG = cfg.GG, M = cfg.M;
    const int BQ = obs_bitmap_bytes(cfg.obs_bytes) / 16;
    const int GW = cfg.GS / 4;  // <= 256 dwords: up to 4 passes of 64 lanes
    const bool has_cells = obs && !(OBS_ABLATE & 4);
    const uint32_t* slot_agents = slots.a;
    // ---- zero the bitmap, park the record in LDS
    if (obs) {
        const u32x4_t z = {0u, 0u, 0u, 0u};
        for (int q = lane; q < BQ; q += WAVE) ((u32x4_t*)bits)[q] = z;
    }
    if (lane < cfg.RS / 4) ((uint32_t*)srec)[lane] = recw;
    __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
    __builtin_amdgcn_wave_barrier();

    // ---- hot bits of every tile plane
    if (has_cells) {
        for (int w = lane; w < GW; w += WAVE) {
            if (w >= WAVE) cells = ((const uint32_t*)(p.grid + (size_t)e * cfg.GS))[w];  // G > 16 only
            int r = (int)fdiv((uint32_t)(w * 4), cfg.div_g), c = w * 4 - r * G;
            #pragma unroll
            for (int b = 0; b < 4; b++) {
                const int cell = w * 4 + b;
                const uint32_t v = (cells >> (8 * b)) & 0xFFu;
                if (v != 0 && cell < GG) {
                    const int fl = flip_cell(cfg, cell, r, c);
                    #pragma unroll
                    for (int slot = 0; slot < 4; slot++) {
                        if (slot_agents[slot]) {  // uniform
                            // nibble v of the 64-bit LUT with 32-bit ops (a 64-bit variable shift is several times slower)
                            const uint64_t lut = pin64(cfg.chan_lut[slot >> 1]);
                            const uint32_t code = (((v & 8u) ? (uint32_t)(lut >> 32) : (uint32_t)lut) >> (4 * (v & 7u))) & 15u;
                            if (code != CTF_TILE_NONE) {
                                const uint32_t q = code * (uint32_t)GG + (uint32_t)((slot & 1) ? fl : cell);
                                for (uint32_t m = slot_agents[slot]; m; m &= m - 1) {  // uniform loop over the slot's agents
                                    const uint32_t bit = (uint32_t)(__ffs((int)m) - 1) * (uint32_t)cfg.CGG + q;
                                    atomicOr(bits + (bit >> 5), 1u << (bit & 31u));
                                }
                            }
                        }
                    }
                }
                if (++c == G) { c = 0; r++; }
            }
        }
    }
    // ---- plane 0: the viewer's own position
    if (obs && lane < N) {
        const int8_t* ps = (const int8_t*)(srec + cfg.off_pos);
        const int r = ps[2 * lane], c = ps[2 * lane + 1];
        const int cell = ((reverse_mask >> lane) & 1u) ? flip_cell(cfg, r * G + c, r, c) : r * G + c;
        const uint32_t bit = (uint32_t)lane * (uint32_t)cfg.CGG + (uint32_t)cell;
        atomicOr(bits + (bit >> 5), 1u << (bit & 31u));
    }

    // ---- metadata (gridworld_ctf.py:1027-1069).  A: the few distinct values, as f16 bits
    if (meta && !(OBS_ABLATE & 8)) {
        const int32_t* misc = (const int32_t*)(srec + cfg.off_misc);
        if (lane < 36) {
            double val = 0.0;
            if (lane == META_MV_STEP) val = meta_step_fraction(misc[0], cfg.game_steps);
            else if (lane < META_MV_RATIO + 2) val = meta_capture_ratio(misc[lane], misc[3 - lane]);  // viewer team lane-1
            else if (lane >= META_MV_HP && lane < META_MV_HP + N) val = (double)meta_hp_u8(cfg, srec, lane - META_MV_HP);
            else if (lane >= META_MV_FLAG && lane < META_MV_FLAG + N) val = (double)srec[cfg.off_flag + lane - META_MV_FLAG];
            mv[lane] = f64_to_f16(val);
        }
        __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
        __builtin_amdgcn_wave_barrier();
        // B: every element of the N x M block is one of those values (which one: obs_meta_lut, built once per wave)
        for (int idx = lane; idx < N * M; idx += WAVE) mstage[idx] = mv[mlut[idx]];
        __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
        __builtin_amdgcn_wave_barrier();
        // C: N*M*2 = 4N(N+3) bytes, always a multiple of 8
        u32x2_t* mdst = (u32x2_t*)(meta + (size_t)e * N * M);
        if (!(OBS_ABLATE & 16))
        for (int q = lane; q < N * M / 4; q += WAVE) mdst[q] = ((const u32x2_t*)mstage)[q];
    }
    __builtin_amdgcn_s_waitcnt(LGKM_ONLY);  // the bitmap's atomic ORs have landed
    __builtin_amdgcn_wave_barrier();

}

// ---- host side: integer knobs of the environment (tests, profiling).  Read at every call unless said otherwise: tests flip
// them inside one process.
static inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
static inline bool obs_xcd_knob() { return env_int("CTF_OBS_XCD", 1) != 0; }  // 0: launch-order tiles / plain grid-stride envs (profiling); default: XCD-contiguous
// waves per block of the wave-per-env renders: 4 unless one env's LDS is so large that 4 of them would crowd the CU's LDS
static inline int obs_waves_per_block(int per_wave) {
    int wpb = 4;
    while (wpb > 1 && wpb * per_wave > 40 * 1024) wpb >>= 1;
    return wpb;
}
