// ctf_states.h — env states as plain arrays (ctf_export_states / ctf_import_states, ctf_states.hip): the conversion between one
// env's device form (ctf_device.h: rec, grid, metric, vis) and row k of the caller's arrays (ctf_state_arrays), and the validity
// check of a row.  Plain inline functions over byte pointers, compiled for the host and the device: the kernels call them with a
// group of lanes per record, the host test (tests/hostsim/states_main.cpp) with one "lane" over heap buffers of the exact sizes.
//
// THE ROW of record k in array f is st_row_bytes(f) bytes at arr[f] + k * st_row_bytes(f): dense, no padding to GS.  Arrays are
// 16-byte aligned, rows are not (N = 3: a has_flag row is 3 bytes), so a row is moved as u32 words when its address and length
// allow it and as single bytes otherwise; every byte comes from st_out_byte (export) or st_rec_byte / st_grid_byte (import), so
// the two directions and the two widths cannot disagree.  Work items are taken t, t + nt, t + 2 nt, ...: consecutive lanes of a
// record's group touch consecutive words of a row.
//
// EXPORT shows what ctf_get_state shows (it runs these functions on one record, ctf_state_view.h): the record's fields as they lie (hp
// is eight bytes, copied), inventory widened from i16, step / captures = misc[0..2], done = misc[3] & CTF_F_DONE.
// IMPORT writes what ctf_set_state writes (likewise), byte for byte: the record with its unused bytes zero, the grid with GG..GS zero, the
// counters (zeros when none are given), and either the given u8 maps widened into the u32 base maps (pad cells zero) or
// CTF_F_BASE_ZERO; misc[3] = done | base-zero | step_count << CTF_F_FOLDED_SHIFT: the visitation log is empty.
// All offsets into caller arrays and env state are size_t.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ctf_device.h"

#if defined(__HIPCC__)
#define CTF_HD __host__ __device__ __forceinline__
#else
#define CTF_HD static inline
#endif

// the members of ctf_state_arrays, in the struct's order
enum { ST_GRID = 0, ST_POS, ST_HP, ST_FLAG, ST_INV, ST_PERM, ST_STEP, ST_CAPS, ST_DONE, ST_METRICS, ST_VIS, ST_FIELDS };

struct StateShape {
    int32_t n_envs, N, G, GG, GS, RS, off_pos, off_flag, off_perm, off_inv, off_misc, log_metrics;
};
// the caller's arrays (device pointers in the kernels)
struct StateArrays {
    uint8_t* arr[ST_FIELDS];
};
// the env state of a handle
struct StateDev {
    uint8_t* rec;       // u8 [E][RS]
    uint8_t* grid;      // u8 [E][GS]
    int32_t* metrics;   // i32 [E][13][N], or NULL (log_metrics == 0)
    uint32_t* vis;      // u32 [E][N][GS], or NULL
    uint32_t* status;
};

static inline StateShape state_shape(const DevCfg& d) {
    return StateShape{d.n_envs, d.N, d.G, d.GG, d.GS, d.RS, d.off_pos, d.off_flag, d.off_perm, d.off_inv, d.off_misc, d.log_metrics};
}
static inline StateDev state_dev(const DevCfg& d, const DevPtrs& p) {
    return StateDev{p.rec, p.grid, d.log_metrics ? p.metrics : nullptr, d.log_metrics ? p.vis : nullptr, p.status};
}

CTF_HD int st_row_bytes(const StateShape& S, int f) {
    switch (f) {
        case ST_GRID: return S.GG;
        case ST_POS: return 2 * S.N;
        case ST_HP: return 8 * S.N;
        case ST_FLAG: return S.N;
        case ST_INV: return 4 * S.N;
        case ST_PERM: return S.N;
        case ST_STEP: return 4;
        case ST_CAPS: return 8;
        case ST_DONE: return 1;
        case ST_METRICS: return 4 * CTF_N_METRICS * S.N;
        default: return S.N * S.GG;  // ST_VIS
    }
}

CTF_HD uint32_t st_load_u32(const uint8_t* p) {  // little-endian, any alignment
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// ---- export: device form -> row ---------------------------------------------------------------------------------------------------
// byte b of the row of field f (f < ST_VIS) of the env whose record / grid / counters these are
CTF_HD uint8_t st_out_byte(const StateShape& S, int f, const uint8_t* rec, const uint8_t* grid, const uint8_t* metrics, int b) {
    switch (f) {
        case ST_GRID: return grid[b];
        case ST_POS: return rec[S.off_pos + b];
        case ST_HP: return rec[b];
        case ST_FLAG: return rec[S.off_flag + b];
        case ST_INV: {  // i16 -> i32
            const uint8_t* q = rec + S.off_inv + 2 * (b >> 2);
            return (b & 2) ? (uint8_t)((q[1] & 0x80) ? 0xFF : 0) : q[b & 1];
        }
        case ST_PERM: return rec[S.off_perm + b];
        case ST_STEP: return rec[S.off_misc + b];
        case ST_CAPS: return rec[S.off_misc + 4 + b];
        case ST_DONE: return (uint8_t)(rec[S.off_misc + 12] & CTF_F_DONE);
        default: return metrics[b];  // ST_METRICS
    }
}

// row k of every non-NULL array of `out` := the env; work items t, t + nt, ...
CTF_HD void states_unpack(const StateShape& S, const uint8_t* rec, const uint8_t* grid, const uint8_t* metrics, const StateArrays& out,
                          size_t k, int t, int nt) {
    for (int f = 0; f < ST_VIS; f++) {
        if (!out.arr[f]) continue;
        const int rb = st_row_bytes(S, f);
        uint8_t* row = out.arr[f] + k * (size_t)rb;
        if ((((uintptr_t)row | (uintptr_t)rb) & 3) == 0) {
            for (int w = t; w < (rb >> 2); w += nt) {
                const int b = 4 * w;
                ((uint32_t*)row)[w] = (uint32_t)st_out_byte(S, f, rec, grid, metrics, b) | (uint32_t)st_out_byte(S, f, rec, grid, metrics, b + 1) << 8 |
                                      (uint32_t)st_out_byte(S, f, rec, grid, metrics, b + 2) << 16 |
                                      (uint32_t)st_out_byte(S, f, rec, grid, metrics, b + 3) << 24;
            }
        } else {
            for (int b = t; b < rb; b += nt) row[b] = st_out_byte(S, f, rec, grid, metrics, b);
        }
    }
}

// ---- import: row -> device form -----------------------------------------------------------------------------------------------------
CTF_HD const uint8_t* st_row(const StateShape& S, const StateArrays& in, int f, size_t k) { return in.arr[f] + k * (size_t)st_row_bytes(S, f); }

// what a record may hold, one predicate per rule: states_check applies them to a row, ctf_set_state names the first value that breaks one
CTF_HD bool st_ok_coord(const int8_t& v, const int32_t& G) { return v >= 0 && v < G; }  // a row or column inside the grid (by reference: k_import_states keeps its code)
CTF_HD bool st_ok_perm(int v, int N) { return v < N; }                     // an entry of the shuffled agent order
CTF_HD bool st_ok_inventory(int32_t v) { return v >= 0 && v <= 1000; }     // (the record keeps it as i16)
CTF_HD bool st_ok_tile(int v) { return v <= 13; }                          // a grid code
CTF_HD bool st_ok_step(int32_t v) { return v >= 0 && v < (1 << 28); }      // (misc[3] keeps step_count << CTF_F_FOLDED_SHIFT)

// the rules on row k (the items t, t + nt, ... of them): true = nothing wrong among these items
CTF_HD bool states_check(const StateShape& S, const StateArrays& in, size_t k, int t, int nt) {
    bool ok = true;
    const int8_t* pos = (const int8_t*)st_row(S, in, ST_POS, k);
    for (int j = t; j < 2 * S.N; j += nt) ok = ok && st_ok_coord(pos[j], S.G);
    const uint8_t* perm = st_row(S, in, ST_PERM, k);
    const uint8_t* inv = st_row(S, in, ST_INV, k);
    for (int i = t; i < S.N; i += nt) {
        const int32_t v = (int32_t)st_load_u32(inv + 4 * i);
        ok = ok && st_ok_perm(perm[i], S.N) && st_ok_inventory(v);
    }
    const uint8_t* grid = st_row(S, in, ST_GRID, k);
    for (int c = t; c < S.GG; c += nt) ok = ok && st_ok_tile(grid[c]);
    if (t == 0) {
        const int32_t step = (int32_t)st_load_u32(st_row(S, in, ST_STEP, k));
        ok = ok && st_ok_step(step);
    }
    return ok;
}

// misc[3] of the imported env: the given maps become the base maps, or the maps restart as after reset(); the log is empty
CTF_HD uint32_t st_misc3(const StateShape& S, const StateArrays& in, size_t k) {
    const uint32_t step = st_load_u32(st_row(S, in, ST_STEP, k));
    const bool maps = S.log_metrics && in.arr[ST_VIS];
    return (uint32_t)(st_row(S, in, ST_DONE, k)[0] ? CTF_F_DONE : 0) | (uint32_t)(maps ? 0 : CTF_F_BASE_ZERO) | step << CTF_F_FOLDED_SHIFT;
}

// byte b of the env's record
CTF_HD uint8_t st_rec_byte(const StateShape& S, const StateArrays& in, size_t k, int b) {
    const int N = S.N;
    if (b < S.off_pos) return st_row(S, in, ST_HP, k)[b];
    if (b < S.off_flag) return st_row(S, in, ST_POS, k)[b - S.off_pos];
    if (b < S.off_perm) return st_row(S, in, ST_FLAG, k)[b - S.off_flag];
    if (b < S.off_inv) return st_row(S, in, ST_PERM, k)[b - S.off_perm];
    if (b < S.off_inv + 2 * N) {  // i32 -> i16: the low two bytes
        const int j = b - S.off_inv;
        return st_row(S, in, ST_INV, k)[4 * (j >> 1) + (j & 1)];
    }
    const int m = b - S.off_misc;
    if (m < 0 || m >= 16) return 0;
    if (m < 4) return st_row(S, in, ST_STEP, k)[m];
    if (m < 12) return st_row(S, in, ST_CAPS, k)[m - 4];
    return (uint8_t)(st_misc3(S, in, k) >> (8 * (m - 12)));
}

CTF_HD uint8_t st_grid_byte(const StateShape& S, const StateArrays& in, size_t k, int c) { return c < S.GG ? st_row(S, in, ST_GRID, k)[c] : (uint8_t)0; }

CTF_HD uint32_t st_word(uint8_t b0, uint8_t b1, uint8_t b2, uint8_t b3) { return (uint32_t)b0 | (uint32_t)b1 << 8 | (uint32_t)b2 << 16 | (uint32_t)b3 << 24; }

// the env := row k.  rec / grid / metrics / vis are the ENV's blocks (16-byte aligned); metrics and vis may be NULL (log_metrics == 0)
CTF_HD void states_pack(const StateShape& S, const StateArrays& in, size_t k, uint8_t* rec, uint8_t* grid, int32_t* metrics, uint32_t* vis, int t,
                        int nt) {
    for (int w = t; w < (S.RS >> 2); w += nt) {
        const int b = 4 * w;
        ((uint32_t*)rec)[w] = st_word(st_rec_byte(S, in, k, b), st_rec_byte(S, in, k, b + 1), st_rec_byte(S, in, k, b + 2), st_rec_byte(S, in, k, b + 3));
    }
    for (int w = t; w < (S.GS >> 2); w += nt) {
        const int c = 4 * w;
        ((uint32_t*)grid)[w] = st_word(st_grid_byte(S, in, k, c), st_grid_byte(S, in, k, c + 1), st_grid_byte(S, in, k, c + 2), st_grid_byte(S, in, k, c + 3));
    }
    if (metrics) {
        const int words = CTF_N_METRICS * S.N;
        const uint8_t* m = in.arr[ST_METRICS] ? st_row(S, in, ST_METRICS, k) : nullptr;
        for (int w = t; w < words; w += nt) metrics[w] = m ? (int32_t)st_load_u32(m + 4 * w) : 0;
    }
    if (vis && in.arr[ST_VIS]) {
        const uint8_t* v = st_row(S, in, ST_VIS, k);
        for (int i = 0; i < S.N; i++)
            for (int c = t; c < S.GS; c += nt) vis[(size_t)i * S.GS + c] = c < S.GG ? (uint32_t)v[(size_t)i * S.GG + c] : 0u;
    }
}
