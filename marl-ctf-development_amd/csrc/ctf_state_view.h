// ctf_state_view.h — ONE env <-> its host view (ctf_state_view: ctf_get_state, ctf_set_state, ctf_host_step) through ctf_states.h:
// the view is the arrays of a batch of ONE record, and states_unpack / states_check / states_pack run on it as one "lane"
// (k, t, nt = 0, 0, 1): a view shows what ctf_export_states shows and takes what ctf_import_states takes, by construction.  Host
// only, plain C++; tests/hostsim/states_main.cpp runs it under sanitizers.
// grid, pos, hp, has_flag, inventory, perm, step_count and team_captures of the view ARE rows (dense from the member's first byte)
// and are aliased as bytes; an aligned row is stored as u32 words, into hp's doubles too: nothing here reads hp as a double after it.
// done (i32 in the view, u8 in a row), metrics and visitation (strided by CTF_MAX_*, dense [13][N] / [N][GG] in a row) are staged.
#pragma once
#include <string.h>
#include <vector>
#include "ctf_states.h"

static inline StateArrays sv_rows(ctf_state_view* v, uint8_t* done, int32_t* metrics, uint8_t* vis) {
    return StateArrays{{v->grid, (uint8_t*)v->pos, (uint8_t*)v->hp, v->has_flag, (uint8_t*)v->inventory, v->perm, (uint8_t*)&v->step_count,
                        (uint8_t*)v->team_captures, done, (uint8_t*)metrics, vis}};
}

// env (rec, grid, counters or NULL) -> *out, zeroed first; the visitation member is sv_visitation's.  misc := the record's four words.
static inline void sv_from_env(const StateShape& S, const uint8_t* rec, const uint8_t* grid, const int32_t* metrics, ctf_state_view* out, int32_t misc[4]) {
    memset(out, 0, sizeof(*out));
    uint8_t done = 0;
    std::vector<int32_t> m(metrics ? (size_t)CTF_N_METRICS * S.N : 0);
    states_unpack(S, rec, grid, (const uint8_t*)metrics, sv_rows(out, &done, metrics ? m.data() : nullptr, nullptr), 0, 0, 1);
    out->done = done;
    for (size_t w = 0; w < m.size(); w++) out->metrics[w / S.N][w % S.N] = m[w];
    memcpy(misc, rec + S.off_misc, 16);
}

// *in -> env (rec RS bytes, grid GS bytes; metrics i32 [13][N] and vis u32 [N][GS] exactly when the handle keeps them, else NULL:
// st_misc3 then sets CTF_F_BASE_ZERO).  false = the view breaks a rule of states_check; nothing has been written then.
static inline bool sv_to_env(const StateShape& S, const ctf_state_view* in, uint8_t* rec, uint8_t* grid, int32_t* metrics, uint32_t* vis) {
    uint8_t done = in->done != 0;
    std::vector<int32_t> m(metrics ? (size_t)CTF_N_METRICS * S.N : 0);
    for (size_t w = 0; w < m.size(); w++) m[w] = in->metrics[w / S.N][w % S.N];
    std::vector<uint8_t> v(vis ? (size_t)S.N * S.GG : 0);
    for (int i = 0; vis && i < S.N; i++) memcpy(v.data() + (size_t)i * S.GG, in->visitation[i], (size_t)S.GG);
    const StateArrays a = sv_rows(const_cast<ctf_state_view*>(in), &done, metrics ? m.data() : nullptr, vis ? v.data() : nullptr);
    if (!states_check(S, a, 0, 0, 1)) return false;
    states_pack(S, a, 0, rec, grid, metrics, vis, 0, 1);
    return true;
}

// The visitation log holds the entries of steps (folded, step_count]: sv_log_count of them (<= CTF_VIS_LOG - 1), entry r in sv_log_slot.
static inline int sv_log_count(const int32_t misc[4]) { return misc[0] > (misc[3] >> CTF_F_FOLDED_SHIFT) ? misc[0] - (misc[3] >> CTF_F_FOLDED_SHIFT) : 0; }
static inline int sv_log_slot(const int32_t misc[4], int r) { return ((misc[3] >> CTF_F_FOLDED_SHIFT) + 1 + r) & (CTF_VIS_LOG - 1); }

// out->visitation := the maps of one env (ctf_visitation.h), u8 wrap as in the reference.  v, u32 [N][GS]: its base maps on entry
// (CTF_F_BASE_ZERO: not read; zeros + 1 at the start cells, reset(): :473), the true counts on return.  ring[s * pitch + i]: agent i's cell of slot s.
static inline void sv_visitation(const StateShape& S, const int8_t start_pos[][2], const int32_t misc[4], uint32_t* v, const uint16_t* ring, size_t pitch, ctf_state_view* out) {
    if (misc[3] & CTF_F_BASE_ZERO) {
        memset(v, 0, (size_t)S.N * S.GS * 4);
        for (int i = 0; i < S.N; i++) v[(size_t)i * S.GS + start_pos[i][0] * S.G + start_pos[i][1]] = 1;
    }
    for (int r = 0, count = sv_log_count(misc); r < count; r++)
        for (int i = 0; i < S.N; i++) {
            const uint16_t cell = ring[(size_t)sv_log_slot(misc, r) * pitch + i];
            if (cell < (uint16_t)S.GG) v[(size_t)i * S.GS + cell]++;  // (>= G * G: the wrapped cell of a CTF_ST_SPAWN_EDGE respawn)
        }
    for (int i = 0; i < S.N; i++)
        for (int k = 0; k < S.GG; k++) out->visitation[i][k] = (uint8_t)(v[(size_t)i * S.GS + k] & 0xFFu);
}
