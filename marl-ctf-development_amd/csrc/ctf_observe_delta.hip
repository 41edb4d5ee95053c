// ctf_observe_delta.hip — the RETAINED render: observe into a buffer the handle owns, rewriting only the 128-byte lines whose
// bytes changed since the last render into it.
//
//   k_observe_delta         the kernel ctf_observe / ctf_step_observe launch on a retained buffer
//   k_observe_delta_bitmap  its round-11 predecessor, selectable (CTF_OBS_DELTA_BITMAP=1 at ctf_obs_retain) for comparisons
//   k_obs_key_clear         ctf_obs_invalidate
// and their launchers (ctf_launch.h).  What the two kernels share with the full renders (obs_build_env, the LDS sizes, the host
// knobs): ctf_render_dev.h.  The dirty-line rule: ctf_obs_delta.h; the chunk rule: ctf_obs_chunk.h.
//
// A translation unit of its own so that work on the retained render leaves the code objects of the step and the full renders
// (ctf_kernels.hip) what they were.  Never built with STEP_TRACE.
//
// The caller has promised (ctf_obs_retain) that nobody but this handle writes the buffer, and the handle keeps a shadow of what it
// last rendered there (ObsShadow, ctf_device.h).  State that changed behind the render (reset, auto-reset, set_state, import,
// restore) needs no notice: the shadow is compared with the state itself.  A key that is not the expected one makes every line
// dirty — that is the first render, an invalidation and a change of the reverse mask, with no other code for any of them.
// One wave per env, one env per wave; envs go to XCDs in contiguous eighths as in k_observe.
#include <hip/hip_runtime.h>

#include "ctf_launch.h"
#include "ctf_obs_delta.h"
#include "ctf_obs_chunk.h"
#include "ctf_render_dev.h"

__host__ __device__ inline int delta_mask_bytes(int obs_bytes) { return ((obsd_lines(obs_bytes, CTF_OBS_LINE - 16) + 31) / 32 * 4 + 15) & ~15; }
__host__ __device__ inline int delta_list_bytes(int obs_bytes) { return (obsd_lines(obs_bytes, CTF_OBS_LINE - 16) * 2 + 15) & ~15; }
#define OBS_DELTA_UNROLL 4  // store instructions (of eight lines each) per pass, their bitmap halfwords read first

// Step 4's compaction, shared by the two kernels: lane q lists the set bits of mask dword q behind those of the dwords before it
// (popcount prefix); returns the list's length.  Ends with the wave's LDS traffic drained.
__device__ __forceinline__ int obs_delta_compact(const uint32_t* lmask, int ndw, uint16_t* llist, int lane) {
    uint32_t m = lane < ndw ? lmask[lane] : 0u;
    int total;
    if (OBS_ABLATE & 32) {  // profiling only, the price of the compaction (profiles/r17_delta_append.md): as many lines, the wrong ones
        uint32_t* cnt = (uint32_t*)llist;
        if (lane == 0) *cnt = 0u;
        if (m) atomicAdd(cnt, (uint32_t)__popc(m));
        __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
        __builtin_amdgcn_wave_barrier();
        total = __builtin_amdgcn_readfirstlane((int)*cnt);
        __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
        __builtin_amdgcn_wave_barrier();
        for (int q = lane; q < total; q += WAVE) llist[q] = (uint16_t)q;
    } else {
        int incl = __popc(m);
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const int up = __shfl_up(incl, d, WAVE);
            if (lane >= d) incl += up;
        }
        total = __shfl(incl, WAVE - 1, WAVE);
        for (int at = incl - __popc(m); m; m &= m - 1u) llist[at++] = (uint16_t)(32 * lane + __ffs((int)m) - 1);
    }
    __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
    __builtin_amdgcn_wave_barrier();
    return total;
}

// (Step 1's loads, the ObsDeltaShape fill and the closing shadow write-back stand in both kernels as they always did: as shared
// functions — by value, by reference or as one struct — each of them changed the instructions of k_observe_delta, which this
// file's move had to leave exactly as they were; profiles/r19_render_split.md.)

// ------------------------------------------------------------------------------------------------
// k_observe_delta_bitmap — the kernel of round 11: the env's whole one-hot block as a bitmap in LDS, as k_observe builds it
// ------------------------------------------------------------------------------------------------
//   1. all loads first: the env's record and grid, the shadow's grid and positions, the shadow's key;
//   2. the env's bitmap and its metadata rows exactly as k_observe makes them (obs_build_env: the rows are written whole);
//   3. the dirty lines of the env's span (ctf_obs_delta.h has the rule): XOR of the two grids names the changed cells, a moved
//      viewer its two bytes of plane 0;
//   4. the dirty lines' indices compacted into a list, then eight lines per store instruction: lanes 8k .. 8k+7 write the eight
//      16-byte chunks of the k-th line of the pass from the bitmap; chunks outside the env's own block belong to the neighbour's
//      wave and are skipped (blocks are whole chunks);
//   5. the shadow dwords that differ are written back, and the key where it was not the expected one.
// Per-wave LDS: [rec RS][mvals 96][meta staging][bitmap][line mask][line list u16].
// Kept selectable until k_observe_delta below has held its numbers on more than one box; three GPU suites compare the two.
__host__ __device__ inline int delta_bitmap_wave_bytes(int RS, int N, int M, int obs_bytes) {
    return RS + OBS_MV_BYTES + obs_meta_stage_bytes(N, M) + obs_bitmap_bytes(obs_bytes) + delta_mask_bytes(obs_bytes) + delta_list_bytes(obs_bytes);
}

template <int STORE_NT>
__global__ void __launch_bounds__(256) k_observe_delta_bitmap(DevCfg cfg, DevPtrs p, ObsShadow sh, uint8_t* __restrict__ obs,
                                                                     uint16_t* __restrict__ meta, uint32_t reverse_mask, uint32_t xcd_map) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int N = cfg.N, M = cfg.M, OB = cfg.obs_bytes, GW = cfg.GS / 4;
    const uint32_t b = blockIdx.x;
    const uint32_t lb = xcd_map ? (b & 7u) * (gridDim.x >> 3) + (b >> 3) : b;
    const int e = (int)lb * (int)(blockDim.x / WAVE) + wave;
    if (e >= cfg.n_envs) return;  // (the whole wave: nothing below synchronises across waves)
    uint8_t* wl = (uint8_t*)lds + wave * delta_bitmap_wave_bytes(cfg.RS, N, M, OB);
    uint8_t* srec = wl;
    uint16_t* mv = (uint16_t*)(wl + cfg.RS);
    uint16_t* mstage = (uint16_t*)(wl + cfg.RS + OBS_MV_BYTES);
    uint32_t* bits = (uint32_t*)(wl + cfg.RS + OBS_MV_BYTES + obs_meta_stage_bytes(N, M));
    uint32_t* lmask = (uint32_t*)((uint8_t*)bits + obs_bitmap_bytes(OB));
    uint16_t* llist = (uint16_t*)((uint8_t*)lmask + delta_mask_bytes(OB));

    // ---- 1. loads, all issued before anything waits, on clamped indices
    const uint32_t* gcur = (const uint32_t*)(p.grid + (size_t)e * cfg.GS);
    uint32_t* gsh = (uint32_t*)(sh.grid + (size_t)e * cfg.GS);
    const uint32_t recw = ((const uint32_t*)(p.rec + (size_t)e * cfg.RS))[min(lane, cfg.RS / 4 - 1)];
    uint32_t cur[4], old[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {  // G <= 32: at most 256 grid dwords (uniform conditions)
        cur[j] = (GW > WAVE * j) ? gcur[min(lane + WAVE * j, GW - 1)] : 0u;
        old[j] = (GW > WAVE * j) ? gsh[min(lane + WAVE * j, GW - 1)] : 0u;
    }
    uint16_t* psh = sh.pos + (size_t)e * CTF_MAX_AGENTS;
    const uint32_t old_pos = psh[min(lane, N - 1)];
    const uint32_t key = CTF_OBS_KEY(reverse_mask);
    const bool known = sh.key[e] == key;  // uniform

    // ---- 2. bitmap + metadata rows
    if (meta && lane == 0) { mv[40] = 0x3C00u; mv[41] = 0u; }
    const ObsSlots slots = obs_slots(cfg, reverse_mask);
    obs_build_env(cfg, p, e, recw, cur[0], srec, mv, mstage, p.meta_lut, bits, slots, reverse_mask, lane, true, meta);

    // ---- 3. the dirty lines of the env's span
    const size_t base = (size_t)e * (size_t)OB;
    const int lead = (int)(((uintptr_t)obs + base) & (uintptr_t)(CTF_OBS_LINE - 1));  // a multiple of 16
    const int nl = obsd_lines(OB, lead), ndw = (nl + 31) >> 5;                       // ndw <= 64 (obsd_applies)
    if (lane < ndw) {
        const int left = nl - 32 * lane;
        lmask[lane] = known ? 0u : (left >= 32 ? 0xFFFFFFFFu : (1u << left) - 1u);
    }
    __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
    __builtin_amdgcn_wave_barrier();
    const uint32_t cur_pos = *(const uint16_t*)(srec + cfg.off_pos + 2 * min(lane, N - 1));
    if (known) {
        ObsDeltaShape s;
        s.N = N; s.G = cfg.G; s.GG = cfg.GG; s.CGG = cfg.CGG; s.obs_bytes = OB; s.flip_axis = cfg.flip_axis;
        s.team_mask = cfg.team_mask; s.chan_lut[0] = cfg.chan_lut[0]; s.chan_lut[1] = cfg.chan_lut[1];
        auto mark = [&](int line) {
            if ((uint32_t)line < (uint32_t)nl) atomicOr(lmask + (line >> 5), 1u << (line & 31));
        };
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int w = lane + WAVE * j;
            const uint32_t x = cur[j] ^ old[j];
            if (GW > WAVE * j && w < GW && x) {
                for (int q = 0; q < 4; q++) {
                    const int cell = 4 * w + q;
                    if (((x >> (8 * q)) & 0xFFu) && cell < cfg.GG)
                        obsd_cell_changed(s, reverse_mask, lead, cell, (old[j] >> (8 * q)) & 0xFFu, (cur[j] >> (8 * q)) & 0xFFu, mark);
                }
            }
        }
        if (lane < N && cur_pos != old_pos) {
            const int oc = (int)(int8_t)(old_pos & 0xFFu) * cfg.G + (int)(int8_t)(old_pos >> 8);
            const int nc = (int)(int8_t)(cur_pos & 0xFFu) * cfg.G + (int)(int8_t)(cur_pos >> 8);
            obsd_viewer_moved(s, reverse_mask, lead, lane, oc, nc, mark);
        }
        __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
        __builtin_amdgcn_wave_barrier();
    }

    // ---- 4. compact ...
    const int total = obs_delta_compact(lmask, ndw, llist, lane);
    // ... and emit: lanes 8k .. 8k+7 hold the eight chunks of one line
    {
        uint8_t* out = obs + base;
        const uint16_t* hb = (const uint16_t*)bits;
        const int sub = lane >> 3, off_in_line = (lane & 7) * 16 - lead;
        for (int l0 = 0; l0 < total; l0 += 8 * OBS_DELTA_UNROLL) {
            uint32_t h[OBS_DELTA_UNROLL];
            int k[OBS_DELTA_UNROLL];
#pragma unroll
            for (int u = 0; u < OBS_DELTA_UNROLL; u++) {
                const int idx = l0 + 8 * u + sub;
                const int o = idx < total ? (int)llist[idx] * CTF_OBS_LINE + off_in_line : -1;  // byte of the env's block
                k[u] = (o >= 0 && o < OB) ? o >> 4 : -1;
                h[u] = k[u] >= 0 ? hb[k[u]] : 0u;
            }
#pragma unroll
            for (int u = 0; u < OBS_DELTA_UNROLL; u++) {
                if (k[u] >= 0) {
                    const u32x4_t v = {expand4(h[u], 0), expand4(h[u], 1), expand4(h[u], 2), expand4(h[u], 3)};
                    if (STORE_NT) __builtin_nontemporal_store(v, (u32x4_t*)(out + ((size_t)k[u] << 4)));
                    else *(u32x4_t*)(out + ((size_t)k[u] << 4)) = v;
                }
            }
        }
    }

    // ---- 5. the shadow follows what the buffer now holds
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int w = lane + WAVE * j;
        if (GW > WAVE * j && w < GW && (!known || cur[j] != old[j])) gsh[w] = cur[j];
    }
    if (lane < N && (!known || cur_pos != old_pos)) psh[lane] = (uint16_t)cur_pos;
    if (!known && lane == 0) sh.key[e] = key;
}

// ------------------------------------------------------------------------------------------------
// k_observe_delta — the same render without the block's bitmap
// ------------------------------------------------------------------------------------------------
//   1. all loads first, on clamped indices: the viewers' positions (and, META, the record), the grid, the shadow's grid, positions
//      and key and — key known — the shadow's images of the slots in use, 16 bytes per lane;
//   2. from the loaded registers into LDS, with no wait in between (a wave's LDS operations complete in order): at most four SLOT
//      IMAGES of CGG bits each (a view is seen through slot 2 * team + reversed; ctf_obs_chunk.h) — parked as loaded under a known
//      key, else zeroed and built from all cells with one OR per non-empty cell and slot in use —, the viewers' own (possibly
//      flipped) cells, the line mask's start (all ones under an unknown key or `all_dirty`) and, by ballot and lane count, the
//      list of cells whose tile differs from the shadow's;
//   3. key known: a lane per (changed cell, viewer) marks the pair's lines (obsd_pair_changed_at), a moved viewer its two bytes
//      of plane 0 (obsd_viewer_moved_rc); then a lane per (changed cell, slot) moves its bit in the slot's image
//      (obsc_update_slot) and stores the dwords it touched to the shadow;
//   4. the dirty lines' indices compacted into a list (obs_delta_compact), then eight lines per store instruction: lanes
//      8k .. 8k+7 write the eight 16-byte chunks of the k-th line of the pass, each from bit (offset % CGG) of its view's slot
//      image with the viewer's own cell ORed in (obsc_chunk_bits);
//   5. META: the metadata rows, whole, behind the stores (obs_build_env parks the record in LDS and makes them from it); then
//      the shadow follows: the grid dwords and position halfwords that differ and, under an unknown key, all of them, the images
//      of the slots in use, whole, and the key.
// REBUILD (CTF_OBS_DELTA_REBUILD=1): the images are built from all cells at every render, the shadow's neither read nor written.
// META = false: the caller has the rows from elsewhere (ctf_step_observe: k_step wrote them, ctf_meta.h) — no record load, no
// record parking and no obs_build_env in the kernel at all; `meta` is then not looked at.
// `all_dirty` (CTF_OBS_DELTA_ALL_DIRTY=1, tests and soaks): every line is rewritten although the key is known, the images still
// carried forward — every byte of the buffer then shows what the retained images hold.
// Per-wave LDS: [rec RS][mvals 96][meta staging][slot images 4 x][own cells u16[16]][changed cells u32[GS]][line mask][line list u16].
// How it came to this shape, what was measured and what was tried and dropped: DESIGN.md §3.1a and profiles/r1[1-7]_*.
__host__ __device__ inline int delta_wave_bytes(int RS, int N, int M, int CGG, int GS, int obs_bytes) {
    return RS + OBS_MV_BYTES + obs_meta_stage_bytes(N, M) + 16 * obsc_image_dwords(CGG) + 2 * CTF_MAX_AGENTS + 4 * GS + delta_mask_bytes(obs_bytes) +
           delta_list_bytes(obs_bytes);
}

#ifndef OBS_DELTA_META_FIRST
#define OBS_DELTA_META_FIRST 0  // 1 = profiling comparison only: the metadata rows made before the dirty lines are marked and stored
#endif

#define OBS_DELTA_IMG_REGS 2  // 16-byte units of the shadow's images a lane loads with the first loads (the arena needs one)

template <int STORE_NT, bool REBUILD, bool META>
__global__ void __launch_bounds__(256) k_observe_delta(DevCfg cfg, DevPtrs p, ObsShadow sh, uint8_t* __restrict__ obs,
                                                       uint16_t* __restrict__ meta, uint32_t reverse_mask, uint32_t xcd_map, uint32_t all_dirty) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int N = cfg.N, M = cfg.M, OB = cfg.obs_bytes, GW = cfg.GS / 4, IW = obsc_image_dwords(cfg.CGG), IU = IW / 4;
    const uint32_t b = blockIdx.x;
    const uint32_t lb = xcd_map ? (b & 7u) * (gridDim.x >> 3) + (b >> 3) : b;
    const int e = (int)lb * (int)(blockDim.x / WAVE) + wave;
    if (e >= cfg.n_envs) return;  // (the whole wave: nothing below synchronises across waves)
    uint8_t* wl = (uint8_t*)lds + wave * delta_wave_bytes(cfg.RS, N, M, cfg.CGG, cfg.GS, OB);
    uint8_t* srec = wl;
    uint16_t* mv = (uint16_t*)(wl + cfg.RS);
    uint16_t* mstage = (uint16_t*)(wl + cfg.RS + OBS_MV_BYTES);
    uint32_t* images = (uint32_t*)(wl + cfg.RS + OBS_MV_BYTES + obs_meta_stage_bytes(N, M));
    uint16_t* selfc = (uint16_t*)(images + 4 * IW);
    uint32_t* chg = (uint32_t*)(selfc + CTF_MAX_AGENTS);
    uint32_t* lmask = chg + cfg.GS;
    uint16_t* llist = (uint16_t*)((uint8_t*)lmask + delta_mask_bytes(OB));

    // ---- 1. loads, all issued before anything waits, on clamped indices
    const uint32_t* gcur = (const uint32_t*)(p.grid + (size_t)e * cfg.GS);
    uint32_t* gsh = (uint32_t*)(sh.grid + (size_t)e * cfg.GS);
    const uint8_t* rec = p.rec + (size_t)e * cfg.RS;
    uint32_t recw = 0u;
    if constexpr (META) recw = ((const uint32_t*)rec)[min(lane, cfg.RS / 4 - 1)];
    const uint32_t cur_pos = *(const uint16_t*)(rec + cfg.off_pos + 2 * min(lane, N - 1));
    uint32_t cur[4], old[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {  // G <= 32: at most 256 grid dwords (uniform conditions)
        cur[j] = (GW > WAVE * j) ? gcur[min(lane + WAVE * j, GW - 1)] : 0u;
        old[j] = (GW > WAVE * j) ? gsh[min(lane + WAVE * j, GW - 1)] : 0u;
    }
    uint16_t* psh = sh.pos + (size_t)e * CTF_MAX_AGENTS;
    const uint32_t old_pos = psh[min(lane, N - 1)];
    const uint32_t key = CTF_OBS_KEY(reverse_mask);
    const bool known = sh.key[e] == key;  // uniform

    ObsDeltaShape s;
    s.N = N; s.G = cfg.G; s.GG = cfg.GG; s.CGG = cfg.CGG; s.obs_bytes = OB; s.flip_axis = cfg.flip_axis;
    s.team_mask = cfg.team_mask; s.chan_lut[0] = cfg.chan_lut[0]; s.chan_lut[1] = cfg.chan_lut[1];
    const uint32_t used = obsc_slots_used(s, reverse_mask);
    const size_t base = (size_t)e * (size_t)OB;
    const int lead = (int)(((uintptr_t)obs + base) & (uintptr_t)(CTF_OBS_LINE - 1));  // a multiple of 16
    const int nl = obsd_lines(OB, lead), ndw = (nl + 31) >> 5;                       // ndw <= 64 (obsd_applies)
    // the shadow's images of the slots in use, 16 bytes per lane: unit q of [rank of the slot among those in use][IU] is unit
    // slot * IU + u of the env's [4][IU]
    uint32_t* ish = sh.images + (size_t)e * (size_t)(4 * IW);
    uint32_t slot_of_rank = 0u;  // nibble k = the k-th slot in use
    int n_iu = 0;
    for (int sl = 0; sl < 4; sl++)
        if (used & (1u << sl)) { slot_of_rank |= (uint32_t)sl << (4 * n_iu); n_iu++; }
    n_iu *= IU;
    auto image_unit = [&](int q) {
        const int k = (q >= IU) + (q >= 2 * IU) + (q >= 3 * IU);
        return q + OBSD_MUL((int)((slot_of_rank >> (4 * k)) & 3u) - k, IU);
    };
    u32x4_t img[OBS_DELTA_IMG_REGS];
    int img_at[OBS_DELTA_IMG_REGS];  // where the unit lies in the env's [4][IU], shadow and LDS alike: worked out once
    if (!REBUILD) {
#pragma unroll
        for (int j = 0; j < OBS_DELTA_IMG_REGS; j++)
            if (n_iu > WAVE * j) {  // (uniform condition)
                img_at[j] = image_unit(min(lane + WAVE * j, n_iu - 1));
                img[j] = ((const u32x4_t*)ish)[img_at[j]];
            }
    }
    const bool build = REBUILD || !known;  // uniform

    // ---- 2. everything the loaded registers give, into LDS: the slot images, the viewers' own cells, the mask's start, the
    // list of changed cells
    if (build) {
        const u32x4_t z = {0u, 0u, 0u, 0u};
        for (int q = lane; q < IW; q += WAVE) ((u32x4_t*)images)[q] = z;  // 4 images of IW dwords = IW x 16 bytes
    } else if (!REBUILD) {
#pragma unroll
        for (int j = 0; j < OBS_DELTA_IMG_REGS; j++)
            if (lane + WAVE * j < n_iu) ((u32x4_t*)images)[img_at[j]] = img[j];  // (not clamped for such a lane)
        for (int q = lane + WAVE * OBS_DELTA_IMG_REGS; q < n_iu; q += WAVE)  // larger shapes: the rest, loaded here
            ((u32x4_t*)images)[image_unit(q)] = ((const u32x4_t*)ish)[image_unit(q)];
    }
    if constexpr (META)
        if (meta && lane == 0) { mv[40] = 0x3C00u; mv[41] = 0u; }
    if (lane < ndw) {
        const int left = nl - 32 * lane;
        lmask[lane] = (known && !all_dirty) ? 0u : (left >= 32 ? 0xFFFFFFFFu : (1u << left) - 1u);
    }
    if (lane < N) selfc[lane] = (uint16_t)obsc_self_cell(s, reverse_mask, lane, (int)(int8_t)(cur_pos & 0xFFu), (int)(int8_t)(cur_pos >> 8));
    if (build) {  // from all cells
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int w = lane + WAVE * j;
            if (GW > WAVE * j) {  // uniform
                const bool mine = w < GW;
                int r = (int)fdiv((uint32_t)(mine ? w * 4 : 0), cfg.div_g), c = (mine ? w * 4 : 0) - OBSD_MUL(r, cfg.G);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int cell = 4 * w + q;
                    if (mine && cell < cfg.GG)
                        obsc_build_cell(s, used, cell, r, c, (cur[j] >> (8 * q)) & 0xFFu,
                                        [&](int slot, int bit) { atomicOr(images + OBSD_MUL(slot, IW) + (bit >> 5), 1u << (bit & 31)); });
                    if (++c == cfg.G) { c = 0; r++; }
                }
            }
        }
    }
    int n_chg = 0;  // uniform
    if (known) {    // the changed cells, gathered: cell | old tile << 16 | new tile << 24
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int w = lane + WAVE * j;
            const uint32_t x = cur[j] ^ old[j];
            if (GW > WAVE * j && __ballot(w < GW && x != 0u)) {  // uniform
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int cell = 4 * w + q;
                    const bool ch = w < GW && cell < cfg.GG && ((x >> (8 * q)) & 0xFFu) != 0u;
                    const uint64_t bal = __ballot(ch);
                    if (bal) {  // uniform
                        if (ch) chg[n_chg + obsd_rank(bal, lane)] = (uint32_t)cell | (((old[j] >> (8 * q)) & 0xFFu) << 16) | (((cur[j] >> (8 * q)) & 0xFFu) << 24);
                        n_chg += __popcll(bal);
                    }
                }
            }
        }
    }

    const ObsSlots no_slots = {{0, 0, 0, 0}};
    if constexpr (META && OBS_DELTA_META_FIRST)
        if (meta)
            obs_build_env(cfg, p, e, recw, 0u, srec, mv, mstage, p.meta_lut, nullptr, no_slots, reverse_mask, lane, false, meta);

    // ---- 3. the dirty lines of the env's span: one changed cell per lane, then the viewers that moved
    if (known) {
        __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
        __builtin_amdgcn_wave_barrier();
        auto mark = [&](int line) {
            if ((uint32_t)line < (uint32_t)nl) atomicOr(lmask + (line >> 5), 1u << (line & 31));
        };
        // a lane per (changed cell, viewer): viewers padded to a power of two, so a pair's cell and viewer are a shift and a mask
        const int vsh = N > 1 ? 32 - __clz(N - 1) : 0, n_pairs = n_chg << vsh;
        for (int at = 0; at < n_pairs; at += WAVE) {
            const int ci = (at + lane) >> vsh, i = (at + lane) & ((1 << vsh) - 1);
            if (ci < n_chg && i < N) {
                const uint32_t ent = chg[ci];
                const int cell = (int)(ent & 0xFFFFu), r = (int)fdiv((uint32_t)cell, cfg.div_g);
                obsd_pair_changed_at(s, lead, ((reverse_mask >> i) & 1u) ? obsc_flip_rc(s, cell, r, cell - OBSD_MUL(r, cfg.G)) : cell, i,
                                     (ent >> 16) & 0xFFu, ent >> 24, mark);
            }
        }
        if (lane < N && cur_pos != old_pos)  // from the row and column bytes of both positions: no division
            obsd_viewer_moved_rc(s, reverse_mask, lead, lane, (int)(int8_t)(old_pos & 0xFFu), (int)(int8_t)(old_pos >> 8), (int)(int8_t)(cur_pos & 0xFFu),
                                 (int)(int8_t)(cur_pos >> 8), mark);
        if (!REBUILD) {
            // the images follow the grid: a lane per (changed cell, slot) moves its bit, then stores the dwords it touched.  Two
            // passes may touch one dword: the later pass's store carries the later value and a wave's stores to one address land
            // in the order they were issued.
            for (int at = 0; at < 4 * n_chg; at += WAVE) {
                const int ci = (at + lane) >> 2, slot = (at + lane) & 3;
                int w_clear = -1, w_set = -1;
                if (ci < n_chg && (used & (1u << slot))) {
                    const uint32_t ent = chg[ci];
                    const int cell = (int)(ent & 0xFFFFu), r = (int)fdiv((uint32_t)cell, cfg.div_g);
                    obsc_update_slot(s, slot, cell, r, cell - OBSD_MUL(r, cfg.G), (ent >> 16) & 0xFFu, ent >> 24,
                                     [&](int sl, int bit) { w_clear = OBSD_MUL(sl, IW) + (bit >> 5); atomicAnd(images + w_clear, ~(1u << (bit & 31))); },
                                     [&](int sl, int bit) { w_set = OBSD_MUL(sl, IW) + (bit >> 5); atomicOr(images + w_set, 1u << (bit & 31)); });
                }
                __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
                __builtin_amdgcn_wave_barrier();
                if (w_clear >= 0) ish[w_clear] = images[w_clear];
                if (w_set >= 0) ish[w_set] = images[w_set];
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(LGKM_ONLY);
    __builtin_amdgcn_wave_barrier();

    // ---- 4. compact ...
    const int total = obs_delta_compact(lmask, ndw, llist, lane);
    // ... and emit: lanes 8k .. 8k+7 hold the eight chunks of one line; chunks outside the env's own block belong to the
    // neighbour's wave and are skipped (blocks are whole chunks)
    {
        uint8_t* out = obs + base;
        const int sub = lane >> 3, off_in_line = (lane & 7) * 16 - lead;
        for (int l0 = 0; l0 < total; l0 += 8 * OBS_DELTA_UNROLL) {
            uint32_t h[OBS_DELTA_UNROLL];
            int o[OBS_DELTA_UNROLL];
#pragma unroll
            for (int u = 0; u < OBS_DELTA_UNROLL; u++) {
                const int idx = l0 + 8 * u + sub;
                o[u] = idx < total ? (int)llist[idx] * CTF_OBS_LINE + off_in_line : -1;  // byte of the env's block
                if (o[u] >= OB) o[u] = -1;
                h[u] = 0u;
                if (o[u] >= 0) {
                    const int view = (int)fdiv((uint32_t)o[u], cfg.div_cgg);
                    h[u] = obsc_chunk_bits(s, reverse_mask, images, IW, selfc, view, o[u] - OBSD_MUL(view, cfg.CGG));
                }
            }
#pragma unroll
            for (int u = 0; u < OBS_DELTA_UNROLL; u++) {
                if (o[u] >= 0) {
                    const u32x4_t v = {obsc_expand4(h[u], 0), obsc_expand4(h[u], 1), obsc_expand4(h[u], 2), obsc_expand4(h[u], 3)};
                    if (STORE_NT) __builtin_nontemporal_store(v, (u32x4_t*)(out + o[u]));
                    else *(u32x4_t*)(out + o[u]) = v;
                }
            }
        }
    }

    // ---- 5. the metadata rows, whole (obs_build_env parks the record in LDS and makes them from it) ...
    if constexpr (META && !OBS_DELTA_META_FIRST)
        if (meta)
            obs_build_env(cfg, p, e, recw, 0u, srec, mv, mstage, p.meta_lut, nullptr, no_slots, reverse_mask, lane, false, meta);

    // ... and the shadow follows what the buffer now holds
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int w = lane + WAVE * j;
        if (GW > WAVE * j && w < GW && (!known || cur[j] != old[j])) gsh[w] = cur[j];
    }
    if (lane < N && (!known || cur_pos != old_pos)) psh[lane] = (uint16_t)cur_pos;
    if (!REBUILD && !known)  // the images built from all cells: the slots in use, whole
        for (int q = lane; q < n_iu; q += WAVE) ((u32x4_t*)ish)[image_unit(q)] = ((const u32x4_t*)images)[image_unit(q)];
    if (!known && lane == 0) sh.key[e] = key;
}
// Everything about the retained buffer is unknown again (ctf_obs_invalidate; behind every other launch that writes the buffer)
extern "C" __global__ void k_obs_key_clear(uint32_t* key, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) key[i] = 0u;
}

// ------------------------------------------------------------------------------------------------
// launchers (ctf_launch.h; called from ctf_abi.hip)
// ------------------------------------------------------------------------------------------------
// the one rule by which a render into a retained `obs` can be the delta render: whole 16-byte chunks at 16-byte aligned addresses
// and a span of lines the kernel's mask holds (ctf_obs_delta.h)
extern "C" int ctf_observe_delta_applies(const DevCfg& cfg, const uint8_t* obs) {
    return obs && ((uintptr_t)obs % 16) == 0 && obsd_applies(cfg.obs_bytes);
}
// k_observe_delta: one wave per env, up to 4 independent waves per block, a multiple of 8 blocks (XCD-contiguous envs);
// bitmap != 0: the round-11 kernel (CTF_OBS_DELTA_BITMAP=1)
extern "C" hipError_t ctf_launch_observe_delta(const DevCfg& cfg, const DevPtrs& p, const ObsShadow& shadow, const RenderArgs& r, int store_nt,
                                               int bitmap, uint32_t flags, hipStream_t st) {
    const int per_wave = bitmap ? delta_bitmap_wave_bytes(cfg.RS, cfg.N, cfg.M, cfg.obs_bytes)
                                : delta_wave_bytes(cfg.RS, cfg.N, cfg.M, cfg.CGG, cfg.GS, cfg.obs_bytes);
    const int wpb = obs_waves_per_block(per_wave);
    const size_t sh = (size_t)wpb * per_wave;
    const unsigned blocks = (unsigned)(((cfg.n_envs + wpb - 1) / wpb + 7) / 8 * 8);
    const uint32_t xcd_map = obs_xcd_knob();
    with_bool(store_nt != 0, [&](auto NT) {
        if (bitmap)
            hipLaunchKernelGGL(k_observe_delta_bitmap<NT.value>, dim3(blocks), dim3(wpb * WAVE), sh, st, cfg, p, shadow, r.obs, r.meta,
                               r.reverse_mask, xcd_map);
        else
            with_bool((flags & CTF_OBS_DELTA_F_REBUILD) != 0u, [&](auto RB) {
                with_bool(r.meta != nullptr, [&](auto META) {  // no rows asked for: the instantiation without any of their code
                    hipLaunchKernelGGL((k_observe_delta<NT.value, RB.value, META.value>), dim3(blocks), dim3(wpb * WAVE), sh, st, cfg, p, shadow, r.obs,
                                       r.meta, r.reverse_mask, xcd_map, (flags & CTF_OBS_DELTA_F_ALL_DIRTY) ? 1u : 0u);
                });
            });
    });
    return hipGetLastError();
}
extern "C" hipError_t ctf_launch_obs_key_clear(const ObsShadow& shadow, int n_envs, hipStream_t st) {
    hipLaunchKernelGGL(k_obs_key_clear, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0, st, shadow.key, n_envs);
    return hipGetLastError();
}
