// ctf_harvest.h — what the episode harvest (ctf_harvest_episodes, ctf_harvest.hip) needs of a handle, and the layout of one row of
// the caller's table.  Shared by the host code (ctf_abi.hip) and the kernel.
//
// A row is H = CTF_HV_HEAD + 13 * N int64 words, one row per caller-defined group of envs:
//   [0] episodes   [1] team-0 wins   [2] draws   [3] team-1 wins      (the sign of team_flag_captures[0] - [1], utils.py:562-569)
//   [4] [5] summed team_flag_captures of team 0 / 1     [6] summed env_step_count     [7] reserved (never written)
//   [8 + m * N + i] summed agent-level counter m (CTF_M_* order) of agent i           (left alone when log_metrics == 0)
#pragma once
#include <stdint.h>

#include "ctf_device.h"

#define CTF_HV_HEAD 8    // words of a row before the counters
#define CTF_HV_SCALARS 7 // of which the kernel writes the first seven

struct HarvestArgs {
    const uint8_t* rec;      // u8 [E][RS]; the env's misc words (step, captures[2], flags) are at off_misc
    const int32_t* metrics;  // i32 [E][13][N], nullptr when log_metrics == 0
    uint32_t* status;
    int32_t n_envs, N, RS, off_misc, game_steps;
};

static inline HarvestArgs harvest_args(const DevCfg& d, const DevPtrs& p) {
    HarvestArgs a;
    a.rec = p.rec;
    a.metrics = d.log_metrics ? p.metrics : nullptr;
    a.status = p.status;
    a.n_envs = d.n_envs;
    a.N = d.N;
    a.RS = d.RS;
    a.off_misc = d.off_misc;
    a.game_steps = d.game_steps;
    return a;
}

static inline int32_t harvest_words(int32_t N) { return CTF_HV_HEAD + CTF_N_METRICS * N; }
