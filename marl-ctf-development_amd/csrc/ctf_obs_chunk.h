// ctf_obs_chunk.h — the chunk rule of the retained observation render (k_observe_delta, ctf_observe_delta.hip): the 16 bytes of chunk k
// of an env's observation block u8 [N][C][G][G], without a bitmap of the whole block in between.
//
// Byte o of the block belongs to view i = o / CGG, plane c = (o % CGG) / GG and destination cell d = o % GG.  It is 1 iff
//   - the tile shown at d has channel c for a viewer of team(i): the tile of cell d itself, or of flip(d) when bit i of the reverse
//     mask is set (reverse_grid; every flip is its own inverse), relabelled by chan_lut[team(i)] — the empty tile 0 and tiles whose
//     nibble is 15 have no plane; or
//   - c is 0 and d is the viewer's own (possibly flipped) cell (obs_build_env's "plane 0: the viewer's own position").
// A view is seen through one of four SLOTS, 2 * team + reversed, and apart from the viewer's own cell every view through a slot is
// the same CGG bytes.  So per env at most four slot IMAGES of CGG bits say it all (394 bytes each for the arena, against the
// N * CGG bits of a bitmap of the block): bit code * GG + d of image[slot] = the tile shown at d has channel `code`.  A wave
// builds them with one OR per non-empty cell and slot in use — not per viewing agent — and a lane then takes its chunk's 16 bits
// from bit r = o % CGG of its view's slot image with one funnel shift, ORs in the viewer's own cell and expands every bit to a
// byte.  A view's planes are contiguous in its image as they are in the block, so only a chunk that runs from one VIEW into the
// next (CGG is rarely a multiple of 16) is made of two segments, each from its own view's image.
// The images depend on the grid alone, so the handle's shadow keeps them between renders (ObsShadow.images, ctf_device.h) and a
// render moves one bit per changed cell and slot (obsc_update_slot) instead of building them again.
//
// Compiled for the device by ctf_observe_delta.hip and for the host by tests/obs_chunk/ (checked against the oracle's renders without a
// GPU), in the manner of ctf_obs_delta.h.  The host's obsc_chunk is the rule spelled out byte by byte; obsc_chunk_images goes through
// the very functions the kernel calls (obsc_build_cell, obsc_self_cell, obsc_chunk_bits, obsc_expand4).
#pragma once
#include <stdint.h>

#include "ctf_obs_delta.h"

#define OBSC_FN OBSD_FN
#define CTF_OBS_CODE_NONE 15u

// the slot a view looks through: 2 * team + reversed
OBSC_FN int obsc_slot(const ObsDeltaShape& s, uint32_t reverse_mask, int i) {
    return (int)(2u * ((s.team_mask >> i) & 1u) + ((reverse_mask >> i) & 1u));
}
// which slots some agent looks through (bit per slot)
OBSC_FN uint32_t obsc_slots_used(const ObsDeltaShape& s, uint32_t reverse_mask) {
    const uint32_t all = (1u << s.N) - 1u, t = s.team_mask & all, rv = reverse_mask & all;  // N <= 16
    return ((all & ~t & ~rv) ? 1u : 0u) | ((~t & rv) ? 2u : 0u) | ((t & ~rv) ? 4u : 0u) | ((t & rv) ? 8u : 0u);
}
// dwords of one slot's image: CGG bits, one dword more for the second half of the last funnel read, in whole 16-byte units
OBSC_FN int obsc_image_dwords(int CGG) { return (((CGG + 31) >> 5) + 1 + 3) & ~3; }

// obsd_flip with the cell's row and column at hand (ctf_obs_delta.h has the one definition)
OBSC_FN int obsc_flip_rc(const ObsDeltaShape& s, int cell, int r, int c) { return obsd_flip_rc(s, cell, r, c); }
// a viewer's own cell as its view shows it
OBSC_FN int obsc_self_cell(const ObsDeltaShape& s, uint32_t reverse_mask, int i, int r, int c) {
    const int cell = OBSD_MUL(r, s.G) + c;
    return ((reverse_mask >> i) & 1u) ? obsc_flip_rc(s, cell, r, c) : cell;
}

// The images' build for one cell (tile v at `cell` = row r, column c): set(slot, bit) once for every slot in `used` that shows
// the tile in a plane.  The images start out zero.
template <class Set>
OBSC_FN void obsc_build_cell(const ObsDeltaShape& s, uint32_t used, int cell, int r, int c, uint32_t v, Set set) {
    if (v == 0u) return;  // the empty tile has no plane (obs_build_env)
    const int fl = (used & 0xAu) ? obsc_flip_rc(s, cell, r, c) : cell;
    for (int t = 0; t < 2; t++) {
        if (!(used & (3u << (2 * t)))) continue;
        const uint32_t code = obsd_channel(s, t, v);
        if (code == CTF_OBS_CODE_NONE) continue;
        if (used & (1u << (2 * t))) set(2 * t, OBSD_MUL(code, s.GG) + cell);
        if (used & (2u << (2 * t))) set(2 * t + 1, OBSD_MUL(code, s.GG) + fl);
    }
}

// The images carried forward instead of rebuilt: `cell` (row r, column c) went from tile a to tile b.  In one slot's image the
// old tile's bit goes and the new tile's bit comes — clear(slot, bit), set(slot, bit); nothing for the empty tile, a tile without a
// plane, or two tiles the slot's team sees in the same plane.  Images that equalled obsc_env_images of the old grid equal those of
// the new grid once every changed cell has been through this (a cell owns its bit positions: no two cells touch the same bit).
template <class Clear, class Set>
OBSC_FN void obsc_update_slot(const ObsDeltaShape& s, int slot, int cell, int r, int c, uint32_t a, uint32_t b, Clear clear, Set set) {
    const uint32_t ca = a ? obsd_channel(s, slot >> 1, a) : CTF_OBS_CODE_NONE, cb = b ? obsd_channel(s, slot >> 1, b) : CTF_OBS_CODE_NONE;
    if (ca == cb) return;
    const int at = (slot & 1) ? obsc_flip_rc(s, cell, r, c) : cell;
    if (ca != CTF_OBS_CODE_NONE) clear(slot, OBSD_MUL(ca, s.GG) + at);
    if (cb != CTF_OBS_CODE_NONE) set(slot, OBSD_MUL(cb, s.GG) + at);
}
// ... in every slot in `used` (k_observe_delta gives every (changed cell, slot) its own lane)
template <class Clear, class Set>
OBSC_FN void obsc_update_cell(const ObsDeltaShape& s, uint32_t used, int cell, int r, int c, uint32_t a, uint32_t b, Clear clear, Set set) {
    for (int slot = 0; slot < 4; slot++)
        if (used & (1u << slot)) obsc_update_slot(s, slot, cell, r, c, a, b, clear, set);
}

// 16 bits of view i from its byte r on: its slot's image, and its own cell in plane 0.  Bits from CGG - r on are not the view's.
OBSC_FN uint32_t obsc_view_bits(const ObsDeltaShape& s, uint32_t reverse_mask, const uint32_t* images, int image_dwords, const uint16_t* self,
                                int i, int r) {
    const uint32_t* q = images + OBSD_MUL(obsc_slot(s, reverse_mask, i), image_dwords) + (r >> 5);
    uint32_t h = (uint32_t)(((((uint64_t)q[1]) << 32) | q[0]) >> (r & 31));
    const uint32_t d = (uint32_t)((int)self[i] - r);
    if (d < 16u) h |= 1u << d;
    return h;
}
// The chunk whose first byte is byte r of view i, one bit per byte.  The segment split: CGG - r bytes are this view's, the rest
// the next view's from its byte 0 on (and so on, should a view be shorter than a chunk); the caller's chunk ends inside the block.
OBSC_FN uint32_t obsc_chunk_bits(const ObsDeltaShape& s, uint32_t reverse_mask, const uint32_t* images, int image_dwords, const uint16_t* self,
                                 int i, int r) {
    uint32_t h = obsc_view_bits(s, reverse_mask, images, image_dwords, self, i, r);
    int at = s.CGG - r;
    if (at < 16) {
        h &= (1u << at) - 1u;
        for (; at < 16; at += s.CGG) {
            const int take = 16 - at < s.CGG ? 16 - at : s.CGG;
            h |= (obsc_view_bits(s, reverse_mask, images, image_dwords, self, ++i, 0) & ((1u << take) - 1u)) << at;
        }
    }
    return h & 0xFFFFu;
}
// bits 4j .. 4j + 3 of h as four bytes of 0 / 1: the four shifted copies of the nibble do not overlap, so no carries
OBSC_FN uint32_t obsc_expand4(uint32_t h, int j) { return (((h >> (4 * j)) & 15u) * 0x00204081u) & 0x01010101u; }

#if !defined(__HIPCC__)
// The rule, byte by byte.  grid: GG tile codes; pos: (row, col) bytes of every agent; k: chunk of the block (16k + 15 < obs_bytes).
OBSC_FN void obsc_chunk(const ObsDeltaShape& s, uint32_t reverse_mask, const uint8_t* grid, const int8_t* pos, int k, uint8_t out[16]) {
    for (int j = 0; j < 16; j++) {
        const int o = 16 * k + j;
        const int i = o / s.CGG, c = (o % s.CGG) / s.GG, d = o % s.GG;
        const bool rev = (reverse_mask >> i) & 1u;
        const int team = (int)((s.team_mask >> i) & 1u);
        const int own = pos[2 * i] * s.G + pos[2 * i + 1];
        const uint32_t v = grid[rev ? obsd_flip(s, d) : d];
        const uint32_t code = v ? obsd_channel(s, team, v) : CTF_OBS_CODE_NONE;
        out[j] = (uint8_t)((code == (uint32_t)c || (c == 0 && d == (rev ? obsd_flip(s, own) : own))) ? 1 : 0);
    }
}

// What a wave does, on the host: the images (4 * obsc_image_dwords(CGG) dwords) and own cells (N entries) of one env ...
OBSC_FN void obsc_env_images(const ObsDeltaShape& s, uint32_t reverse_mask, const uint8_t* grid, const int8_t* pos, uint32_t* images, uint16_t* self) {
    const int W = obsc_image_dwords(s.CGG);
    const uint32_t used = obsc_slots_used(s, reverse_mask);
    for (int q = 0; q < 4 * W; q++) images[q] = 0u;
    for (int cell = 0; cell < s.GG; cell++)
        obsc_build_cell(s, used, cell, cell / s.G, cell % s.G, grid[cell], [&](int slot, int bit) { images[slot * W + (bit >> 5)] |= 1u << (bit & 31); });
    for (int i = 0; i < s.N; i++) self[i] = (uint16_t)obsc_self_cell(s, reverse_mask, i, pos[2 * i], pos[2 * i + 1]);
}
// ... and one chunk from them
OBSC_FN void obsc_chunk_images(const ObsDeltaShape& s, uint32_t reverse_mask, const uint32_t* images, const uint16_t* self, int k, uint8_t out[16]) {
    const int o = 16 * k;
    const uint32_t h = obsc_chunk_bits(s, reverse_mask, images, obsc_image_dwords(s.CGG), self, o / s.CGG, o % s.CGG);
    for (int j = 0; j < 4; j++) {
        const uint32_t x = obsc_expand4(h, j);
        for (int b = 0; b < 4; b++) out[4 * j + b] = (uint8_t)(x >> (8 * b));
    }
}
#endif
