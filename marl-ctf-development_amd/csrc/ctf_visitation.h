// ctf_visitation.h — what the visitation harvest and export (ctf_harvest_visitation / ctf_export_visitation, ctf_visitation.hip)
// need of a handle, and the definition of the result.  Shared by the host code (ctf_abi.hip) and the kernels.
//
// THE MAP OF ONE ENV is what the host decode (sv_visitation, ctf_state_view.h) computes before its final `& 0xFF`.  For agent i:
//   base   CTF_F_BASE_ZERO set in the env's misc flags: zeros, plus 1 at start_pos[i];  otherwise vis[e][i][:] (u32)
//   log    + 1 at cell vislog[s & 511][e][i] for every step s in (folded, env_step_count], folded = misc[3] >> CTF_F_FOLDED_SHIFT
//          (at most 511 entries: k_step folds its own log before a slot is reused)
//   guard  an entry >= G * G is skipped (the wrapped cell of a CTF_ST_SPAWN_EDGE respawn)
// True counts: nothing wraps at 256.  N * G * G words per env, [N][G * G] (the base maps' row stride in HBM is GS >= G * G).
//
// ONE DEVICE CORE, TWO SINKS.  The core (vs_accumulate) adds the maps of a set of envs of one wave's run into an LDS histogram
// [agents of the tile][G * G]; the harvest flushes the histogram's non-zero cells into the caller's int64 table [n_groups][N][G * G]
// with 64-bit vector atomicAdds once per RUN of taken envs that share a group id (not per env), the export stores it to
// out[k][i][cell] with coalesced u32 stores.
//
// THE CELL TYPE is u32, and the histogram is dynamic LDS sized from the config at launch: tile_agents * G * G * 4 bytes, at most
// CTF_VIS_LDS_CAP = 32 KiB.  A config whose N * G * G words exceed the cap (N = 16, G = 32 is 64 KiB) is TILED OVER AGENTS: the
// kernel walks the same envs once per tile of tile_agents agents (G <= 32: a tile holds at least 8).  32 KiB rather than the 64
// KiB a workgroup may ask for without an attribute: five one-wave workgroups then share a CU's 160 KiB, and the kernel keeps
// nothing else in LDS.  A u32 cell cannot overflow between flushes: one env adds at most 256 + env_step_count to a cell (a
// handed-in base cell is a u8, ctf_set_state; every step adds one), and a run is cut — flushed early — before the sum of
// (256 + env_step_count) over its envs would pass 2^32 - 1.  The table's cells are int64.
//
// INDEX ARITHMETIC into vis and vislog is size_t throughout: at 262 144 envs of 16 agents the log has 2^31 elements.
#pragma once
#include <stdint.h>

#include "ctf_device.h"

#define CTF_VIS_LDS_CAP (32 * 1024)  // bytes of the LDS histogram of one wave

struct VisitArgs {
    const uint8_t* rec;      // u8 [E][RS]; the env's misc words (step, captures[2], flags) are at off_misc
    const uint32_t* vis;     // u32 [E][N][GS]
    const uint16_t* vislog;  // u16 [512][E][N]
    uint32_t* status;
    int32_t n_envs, N, GG, GS, RS, off_misc, game_steps;
    int32_t tile_agents;                    // agents whose maps one LDS histogram holds (N when everything fits)
    uint16_t start_cell[CTF_MAX_AGENTS];    // start_pos[i] as a cell index
};

static inline int32_t visitation_words(const DevCfg& d) { return d.N * d.GG; }

static inline VisitArgs visit_args(const DevCfg& d, const DevPtrs& p) {
    VisitArgs a;
    a.rec = p.rec;
    a.vis = p.vis;
    a.vislog = p.vislog;
    a.status = p.status;
    a.n_envs = d.n_envs;
    a.N = d.N;
    a.GG = d.GG;
    a.GS = d.GS;
    a.RS = d.RS;
    a.off_misc = d.off_misc;
    a.game_steps = d.game_steps;
    const int32_t fit = CTF_VIS_LDS_CAP / 4 / d.GG;  // >= 8
    a.tile_agents = d.N < fit ? d.N : fit;
    for (int i = 0; i < CTF_MAX_AGENTS; i++) a.start_cell[i] = i < d.N ? (uint16_t)(d.start_pos[i][0] * d.G + d.start_pos[i][1]) : 0;
    return a;
}

static inline size_t visit_lds_bytes(const VisitArgs& a) { return (size_t)a.tile_agents * a.GG * 4; }
