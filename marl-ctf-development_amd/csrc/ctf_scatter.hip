// ctf_scatter.hip — k_reset_scattered: the rule of ctf_scatter.h on the device (ctf_reset_scattered): ctf_reset with the asked agents
// drawn onto open cells round their start cells.  A translation unit of its own: the step's and the renders' code objects stay as they are.
//
// One 64-lane wave per env, as k_reset.  Lane l owns cells 16 l .. 16 l + 15: one 16-byte load of the init grid, a 16-bit OPEN mask
// (cells of the grid proper: pad cells never count) and the two teams' OWN_SIDE masks, made once.  G = 32 fills all 64 lanes, G = 15
// leaves the last owning lane partial; the lanes past GS / 16 own nothing and only take part in the cross-lane steps.  Per asked agent:
// the radius mask from the coordinates of the lane's cells (row by row: sct_near16), candidates = OPEN & radius & side & ~taken (| the
// start cell's own bit), a popcount, an inclusive 64-lane prefix sum (__shfl_up, six steps), the draw (the agents' Philox words are
// made before the loop, lane i agent i's, and read by __shfl: they do not depend on the candidates), the owning lane by ballot, its
// (k - prefix)-th set bit broadcast by __shfl.  The chosen cell joins the owning lane's
// `taken` mask; both grid edits are applied to the lanes' 16 bytes in registers and the env's grid leaves as one 16-byte store per
// lane: no two lanes store to one address, no ordering question.  Lane i writes agent i's part of the record as reset_record lays it
// out, lane 0 the env's part; the counters are zeroed as k_reset zeroes them; the base maps, only when someone moved, leave as 16-byte
// stores of four u32 cells.  Plain C++ vector stores, no atomics, no LDS; index arithmetic into per-env blocks in size_t.
#include <hip/hip_runtime.h>

#include "ctf_launch.h"
#include "ctf_scatter.h"

#define SCT_WAVE 64
static_assert(CTF_MAX_CELLS / 16 <= SCT_WAVE && CTF_MAX_AGENTS <= SCT_WAVE, "a lane owns sixteen cells; lane i writes agent i");

typedef uint32_t sct_u32x4 __attribute__((ext_vector_type(4)));

// byte j (0..15) of the lane's sixteen := v
__device__ __forceinline__ void sct_set_byte(uint64_t& lo, uint64_t& hi, int j, uint32_t v) {
    const int sh = 8 * (j & 7);
    const uint64_t clr = ~(0xFFull << sh), put = (uint64_t)v << sh;
    if (j < 8) lo = (lo & clr) | put;
    else hi = (hi & clr) | put;
}

__global__ void __launch_bounds__(SCT_WAVE) k_reset_scattered(ScatterArgs A, const uint8_t* __restrict__ mask, uint32_t agent_mask, int32_t radius, uint32_t flags,
                                                               uint64_t seed, uint32_t round, uint32_t* episode, uint32_t env_offset) {
    const size_t e = blockIdx.x;
    const int lane = threadIdx.x;
    if (mask && !mask[e]) return;
    const uint32_t ep = episode ? episode[e] : 0u;
    const uint32_t r = sct_round(round, ep);

    // the lane's sixteen cells of the init grid
    const int base = 16 * lane;
    const bool owns = base < A.GS;
    uint64_t lo = 0, hi = 0;
    if (owns) {
        const sct_u32x4 v = *(const sct_u32x4*)(A.init_grid + base);
        lo = (uint64_t)v.x | (uint64_t)v.y << 32;
        hi = (uint64_t)v.z | (uint64_t)v.w << 32;
    }
    const int r0 = base / A.G, c0 = base - r0 * A.G, r1 = (base + 15) / A.G;
    const bool own_side = (flags & CTF_SCATTER_OWN_SIDE) != 0;
    uint32_t open = 0, side0 = 0xFFFFu, side1 = 0xFFFFu;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t tile = (uint32_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xFFu);
        open |= (base + j < A.GG && sct_open((int)tile) ? 1u : 0u) << j;
    }
    if (own_side) {  // (wave-uniform)
        side0 = side1 = 0;
        int rr = r0, cc = c0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            side0 |= (sct_own_side(A.flag_pack, 0, rr, cc) ? 1u : 0u) << j;
            side1 |= (sct_own_side(A.flag_pack, 1, rr, cc) ? 1u : 0u) << j;
            if (++cc == A.G) { cc = 0; rr++; }
        }
    }
    // the agents' Philox words, lane i agent i's: they depend on nothing the placement decides
    uint32_t my_word = 0;
    if (lane < A.N) my_word = sct_word(seed, env_offset + (uint32_t)e, r, (uint32_t)lane);

    uint32_t taken = 0;
    int my_cell = 0;  // lane i < N: agent i's cell
    bool moved = false;
    for (int i = 0; i < A.N; i++) {
        const int sr = A.start_pos[i][0], sc = A.start_pos[i][1];
        const int s = sr * A.G + sc;
        int cell = s;
        if ((agent_mask >> i) & 1u) {
            const uint32_t near = sct_near16(A.G, base, r0, r1, sr, sc, radius);
            const uint32_t side = ((A.team_mask >> i) & 1u) ? side1 : side0;
            uint32_t cand = open & near & side & ~taken;
            if ((s >> 4) == lane) cand |= 1u << (s & 15);
            const int cnt = __popc(cand);
            int incl = cnt;
#pragma unroll
            for (int d = 1; d < SCT_WAVE; d <<= 1) {
                const int up = __shfl_up(incl, d, SCT_WAVE);
                if (lane >= d) incl += up;
            }
            const uint32_t n = (uint32_t)__shfl(incl, SCT_WAVE - 1, SCT_WAVE);  // >= 1: the start cell
            const int k = (int)sct_pick((uint32_t)__shfl((int)my_word, i, SCT_WAVE), n);
            const int excl = incl - cnt;
            const bool owner = k >= excl && k < incl;  // exactly one lane
            int mine = 0;
            if (owner) {
                uint32_t m = cand;
                for (int t = k - excl; t > 0; t--) m &= m - 1;
                mine = base + __ffs((int)m) - 1;
            }
            const unsigned long long who = __ballot(owner);
            cell = __shfl(mine, __ffsll((long long)who) - 1, SCT_WAVE);
        }
        // cell < GG by construction: a candidate bit is set only for a cell of the grid proper or for s
        if ((cell >> 4) == lane) taken |= 1u << (cell & 15);
        moved = moved || cell != s;
        const uint32_t tile = A.init_grid[s];
        if ((s >> 4) == lane) sct_set_byte(lo, hi, s & 15, 0u);
        if ((cell >> 4) == lane) sct_set_byte(lo, hi, cell & 15, tile);
        if (lane == i) my_cell = cell;
    }

    if (owns) {
        sct_u32x4 v;
        v.x = (uint32_t)lo; v.y = (uint32_t)(lo >> 32); v.z = (uint32_t)hi; v.w = (uint32_t)(hi >> 32);
        *(sct_u32x4*)(A.grid + e * (size_t)A.GS + (size_t)base) = v;
    }
    uint8_t* rec = A.rec + e * (size_t)A.RS;
    if (lane < A.N) sct_record_agent(A, rec, lane, my_cell);
    if (lane == 0) {
        sct_record_misc(A, rec, moved);
        if (episode) episode[e] = ep + 1u;
    }
    if (A.log_metrics) {
        int32_t* m = A.metrics + e * (size_t)CTF_N_METRICS * (size_t)A.N;
        for (int w = lane; w < CTF_N_METRICS * A.N; w += SCT_WAVE) m[w] = 0;
        if (moved) {
            uint32_t* vis = A.vis + e * (size_t)A.N * (size_t)A.GS;
            for (int i = 0; i < A.N; i++) {
                const int ci = __shfl(my_cell, i, SCT_WAVE);
                for (int q = lane; q < A.GS / 4; q += SCT_WAVE) {
                    const int c = 4 * q;
                    sct_u32x4 v;
                    v.x = c == ci; v.y = c + 1 == ci; v.z = c + 2 == ci; v.w = c + 3 == ci;
                    *(sct_u32x4*)(vis + (size_t)i * (size_t)A.GS + (size_t)c) = v;
                }
            }
        }
    }
}

extern "C" hipError_t ctf_launch_reset_scattered(const ScatterArgs& A, const uint8_t* mask, uint32_t agent_mask, int32_t radius, uint32_t flags, uint64_t seed,
                                                 uint32_t round, uint32_t* episode, uint32_t env_offset, hipStream_t st) {
    if (A.n_envs < 1) return hipSuccess;
    hipLaunchKernelGGL(k_reset_scattered, dim3((unsigned)A.n_envs), dim3(SCT_WAVE), 0, st, A, mask, agent_mask, radius, flags, seed, round, episode, env_offset);
    return hipGetLastError();
}
