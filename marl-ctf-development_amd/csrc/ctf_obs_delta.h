// ctf_obs_delta.h — the dirty-line rule of the retained observation render (k_observe_delta, ctf_observe_delta.hip).
//
// An env's observation block u8 [N][C][G][G] is a pure function of its grid, every viewer's own position, the config and the
// reverse mask (gridworld_ctf.py:975-1009).  When a buffer still holds the render of an OLDER state of the env (the handle's
// shadow: the grid and position bytes that render was made from), the bytes that differ from the render of the current state
// are few and can be named without rendering either:
//   - a cell whose tile code went a -> b changes, in the view of every agent i, the byte of plane ch_i(a) and the byte of
//     plane ch_i(b) at flip_i(cell) (ch_i: the channel of a tile for a viewer of team(i), none for tiles without a plane;
//     flip_i: the cell's destination under reverse_grid when bit i of the reverse mask is set);
//   - a viewer that moved changes two bytes of its plane 0.
// The render rewrites whole 128-byte LINES of the flat buffer [E][N][C][G][G]; this header maps the changed bytes to lines.
// Env blocks are not line-aligned (the arena's 25 200 bytes are 196.875 lines), so a line is named by its index inside the env's
// own span: line l of env e covers the bytes [l * 128 - lead, (l + 1) * 128 - lead) of the env's block, where
// lead = (address of the block's first byte) % 128.  A line shared with a neighbouring env is dirty for each env separately and
// each env rewrites only its own bytes of it.
//
// Compiled for the device by ctf_observe_delta.hip and for the host by tests/obs_delta/ (checked against the oracle's consecutive
// renders without a GPU), in the manner of ctf_step_core.h.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OBSD_FN __host__ __device__ inline
#else
#define OBSD_FN static inline
#endif

// A product of two small numbers — cells, rows, planes, views, slots, offsets into an env's block: every operand here is below
// 2^18 (obsd_applies) — as ONE full-rate vector instruction on the device.  A 32-bit integer multiply (v_mul_lo_u32, and the
// v_mad_u64_u32 the compiler likes for a multiply-add) issues at a quarter of the rate, and the known-key path of k_observe_delta ran
// about 50 of them per wave (profiles/r17_delta_append.md); the 24-bit multiply gives the same product for operands of this size.
#if defined(__HIP_DEVICE_COMPILE__)
#define OBSD_MUL(a, b) __mul24((int)(a), (int)(b))
#else
#define OBSD_MUL(a, b) ((int)(a) * (int)(b))
#endif

#define CTF_OBS_LINE 128
#define CTF_OBS_LINE_SHIFT 7
#define CTF_OBS_DELTA_MAX_LINES 2048  // lines of one env's span the kernel's mask holds (64 lanes x 32 bits)

struct ObsDeltaShape {
    int32_t N, G, GG, CGG, obs_bytes;
    int32_t flip_axis;      // FLIP_AXIS: -1 = None (both axes), 0, 1, 2
    uint32_t team_mask;     // bit i = team(i)
    uint64_t chan_lut[2];   // [viewer team]: nibble v = channel of tile v after relabelling, 15 = no plane (DevCfg.chan_lut)
};

// lines of the span of an env whose block starts `lead` bytes into a line
OBSD_FN int obsd_lines(int obs_bytes, int lead) { return (lead + obs_bytes + CTF_OBS_LINE - 1) >> CTF_OBS_LINE_SHIFT; }

// whether the delta render applies to blocks of obs_bytes at all: whole 16-byte chunks, and a span the mask holds at any lead
OBSD_FN bool obsd_applies(int obs_bytes) {
    return obs_bytes > 0 && (obs_bytes % 16) == 0 && obsd_lines(obs_bytes, CTF_OBS_LINE - 16) <= CTF_OBS_DELTA_MAX_LINES;
}

// the render's own lookup (obs_build_env): nibble v of the 64-bit LUT
OBSD_FN uint32_t obsd_channel(const ObsDeltaShape& s, int team, uint32_t v) {
    const uint64_t lut = team ? s.chan_lut[1] : s.chan_lut[0];  // (a select: `team` may differ from lane to lane on the device)
    return (((v & 8u) ? (uint32_t)(lut >> 32) : (uint32_t)lut) >> (4u * (v & 7u))) & 15u;
}

// destination of `cell` under reverse_grid (gridworld_ctf.py:1003-1007; flip_cell of the renders)
OBSD_FN int obsd_flip(const ObsDeltaShape& s, int cell) {
    const int G = s.G, r = cell / G, c = cell - r * G;
    if (s.flip_axis == -1) return s.GG - 1 - cell;
    if (s.flip_axis == 0) return (G - 1 - r) * G + c;
    if (s.flip_axis == 1) return r * G + (G - 1 - c);
    return (G - 1 - c) * G + (G - 1 - r);
}

// `cell` went from tile a to tile b (a != b): mark(line) for every line that holds a byte this changes
template <class Mark>
OBSD_FN void obsd_cell_changed(const ObsDeltaShape& s, uint32_t reverse_mask, int lead, int cell, uint32_t a, uint32_t b, Mark mark) {
    const int fl = obsd_flip(s, cell);
    for (int t = 0; t < 2; t++) {
        const uint32_t ca = obsd_channel(s, t, a), cb = obsd_channel(s, t, b);
        if (ca == cb) continue;  // the same plane (or none) before and after: no byte of a team-t view changes
        for (int i = 0; i < s.N; i++) {
            if ((int)((s.team_mask >> i) & 1u) != t) continue;
            const int at = lead + i * s.CGG + (((reverse_mask >> i) & 1u) ? fl : cell);
            if (ca != 15u) mark((at + (int)ca * s.GG) >> CTF_OBS_LINE_SHIFT);
            if (cb != 15u) mark((at + (int)cb * s.GG) >> CTF_OBS_LINE_SHIFT);
        }
    }
}

// The same rule for one (changed cell, viewer) PAIR — what a lane of k_observe_delta does, the pairs of an env spread over the
// wave: viewer i's two bytes.  The union of the marks over i = 0 .. N-1 is obsd_cell_changed's.  `shown` is the cell as viewer
// i's view shows it (the kernel has the cell's row and column at hand and flips without a division).
template <class Mark>
OBSD_FN void obsd_pair_changed_at(const ObsDeltaShape& s, int lead, int shown, int i, uint32_t a, uint32_t b, Mark mark) {
    const int t = (int)((s.team_mask >> i) & 1u);
    const uint32_t ca = obsd_channel(s, t, a), cb = obsd_channel(s, t, b);
    if (ca == cb) return;
    const int at = lead + OBSD_MUL(i, s.CGG) + shown;
    if (ca != 15u) mark((at + OBSD_MUL(ca, s.GG)) >> CTF_OBS_LINE_SHIFT);
    if (cb != 15u) mark((at + OBSD_MUL(cb, s.GG)) >> CTF_OBS_LINE_SHIFT);
}
template <class Mark>
OBSD_FN void obsd_pair_changed(const ObsDeltaShape& s, uint32_t reverse_mask, int lead, int cell, int i, uint32_t a, uint32_t b, Mark mark) {
    obsd_pair_changed_at(s, lead, ((reverse_mask >> i) & 1u) ? obsd_flip(s, cell) : cell, i, a, b, mark);
}

// viewer i moved from old_cell to new_cell (old_cell != new_cell): the two bytes of its plane 0
template <class Mark>
OBSD_FN void obsd_viewer_moved(const ObsDeltaShape& s, uint32_t reverse_mask, int lead, int i, int old_cell, int new_cell, Mark mark) {
    const bool rev = (reverse_mask >> i) & 1u;
    const int at = lead + i * s.CGG;
    mark((at + (rev ? obsd_flip(s, old_cell) : old_cell)) >> CTF_OBS_LINE_SHIFT);
    mark((at + (rev ? obsd_flip(s, new_cell) : new_cell)) >> CTF_OBS_LINE_SHIFT);
}

// obsd_flip with the cell's row and column at hand: no division
OBSD_FN int obsd_flip_rc(const ObsDeltaShape& s, int cell, int r, int c) {
    const int G = s.G;
    if (s.flip_axis == -1) return s.GG - 1 - cell;
    if (s.flip_axis == 0) return OBSD_MUL(G - 1 - r, G) + c;
    if (s.flip_axis == 1) return OBSD_MUL(r, G) + (G - 1 - c);
    return OBSD_MUL(G - 1 - c, G) + (G - 1 - r);
}
// obsd_viewer_moved from the (row, column) of both cells, as the position bytes give them: the same two marks
template <class Mark>
OBSD_FN void obsd_viewer_moved_rc(const ObsDeltaShape& s, uint32_t reverse_mask, int lead, int i, int old_r, int old_c, int new_r, int new_c, Mark mark) {
    const bool rev = (reverse_mask >> i) & 1u;
    const int at = lead + OBSD_MUL(i, s.CGG), oc = OBSD_MUL(old_r, s.G) + old_c, nc = OBSD_MUL(new_r, s.G) + new_c;
    mark((at + (rev ? obsd_flip_rc(s, oc, old_r, old_c) : oc)) >> CTF_OBS_LINE_SHIFT);
    mark((at + (rev ? obsd_flip_rc(s, nc, new_r, new_c) : nc)) >> CTF_OBS_LINE_SHIFT);
}

// A wave's ballot made into an ascending list, 64 items per pass (k_observe_delta gathers the changed cells so): in pass p lane L
// stands for item 64p + L, `bal` holds bit L = the item is in, and such a lane writes its item at list[base + obsd_rank(bal, L)],
// base = the popcounts of the earlier passes' ballots.
OBSD_FN int obsd_rank(uint64_t bal, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;  // the executing lane: the hardware's count of the set bits below it
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
#else
    return __builtin_popcountll(bal & ((1ull << lane) - 1ull));
#endif
}

#if !defined(__HIPCC__)
// The whole rule for one env, one cell and one viewer after the other (what a wave of k_observe_delta does with its lanes):
// mask bit l = line l of the env's span is dirty.  pos: (row, col) bytes of every agent.  mask: (obsd_lines + 31) / 32 dwords.
OBSD_FN void obsd_env_dirty(const ObsDeltaShape& s, uint32_t reverse_mask, int lead, const uint8_t* grid_old, const int8_t* pos_old,
                            const uint8_t* grid_new, const int8_t* pos_new, uint32_t* mask) {
    const int nl = obsd_lines(s.obs_bytes, lead);
    for (int q = 0; q < (nl + 31) / 32; q++) mask[q] = 0u;
    auto mark = [&](int line) {
        if ((uint32_t)line < (uint32_t)nl) mask[line >> 5] |= 1u << (line & 31);
    };
    for (int cell = 0; cell < s.GG; cell++)
        if (grid_old[cell] != grid_new[cell]) obsd_cell_changed(s, reverse_mask, lead, cell, grid_old[cell], grid_new[cell], mark);
    for (int i = 0; i < s.N; i++) {
        const int oc = pos_old[2 * i] * s.G + pos_old[2 * i + 1], nc = pos_new[2 * i] * s.G + pos_new[2 * i + 1];
        if (oc != nc) obsd_viewer_moved(s, reverse_mask, lead, i, oc, nc, mark);
    }
}
#endif
