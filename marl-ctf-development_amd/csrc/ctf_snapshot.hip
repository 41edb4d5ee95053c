// ctf_snapshot.hip — gather / scatter of whole env records (ctf_save_states / ctf_load_states, ctf_snapshot.h has the record).
//
// Two kinds of blocks in one launch:
//   body blocks    block k < n moves record k's header and body segments (rec, grid, both streams' rings, digests, the rng words,
//                  counters, visitation base maps): the env's bytes of every segment are contiguous in HBM, so the block walks
//                  the segments in turn with 16-byte accesses, 4 KB per pass of its 256 threads, two passes in flight at a time;
//   vislog blocks  the visitation log is u16 [512][E][N]: one env's column is 512 rows of 2N bytes, E * 2N bytes apart.  Lane l of
//                  a wave takes record 64 g + l, so that for an identity (or any run of consecutive) index list the 64 lanes read
//                  and write 64 adjacent rows of a slot — one coalesced 64 x 2N-byte access — and the wave walks SNAP_LOG_SLOTS
//                  slots of that column, four rows in flight per lane.
// Loads check every record they write from: the magic, the layout version and the fingerprint in its header, and the destination
// index (0 <= idx < E).  A record that fails writes nothing and raises CTF_ST_BAD_SNAPSHOT (its body block's thread 0, with a
// vector atomic OR as every other status bit); the vislog lanes of that record skip it.  Saves from an index outside [0, E)
// write a record whose header is zero (a load rejects it) and raise the same bit.  Plain C++ loads and stores throughout.
#include <hip/hip_runtime.h>

#include "ctf_snapshot.h"
#include "ctf_launch.h"

#define SNAP_THREADS 256
#define SNAP_LOG_SLOTS 32                           // vislog slots one wave moves for its 64 records
#define SNAP_LOG_CHUNKS (CTF_VIS_LOG / SNAP_LOG_SLOTS)  // waves per group of 64 records
#define SNAP_WAVE 64

__device__ __forceinline__ bool snap_header_ok(const SnapLayout& L, const uint8_t* rec) {
    const uint4 h = *(const uint4*)rec;
    return h.x == CTF_SNAP_MAGIC && h.y == CTF_SNAP_VERSION && h.z == (uint32_t)L.fingerprint && h.w == (uint32_t)(L.fingerprint >> 32);
}

// 16-byte unit q of segment s of env e: in HBM <-> in the record
template <bool LOAD>
__device__ __forceinline__ uint4 snap_fetch(const SnapLayout& L, const SnapSeg& s, int e, int q, const uint8_t* rec) {
    if (LOAD) return *(const uint4*)(rec + s.off + 16 * q);
    if (s.kind == CTF_SNAP_VEC) return *(const uint4*)(s.base + (size_t)e * s.bytes + 16 * q);
    if (s.kind == CTF_SNAP_RNG)
        return make_uint4(L.rngpos[2 * e], L.rngpos[2 * e + 1],
                          (uint32_t)L.rngready[2 * e] | (uint32_t)L.rngready[2 * e + 1] << 8 | (uint32_t)L.rngage[2 * e] << 16 |
                              (uint32_t)L.rngage[2 * e + 1] << 24,
                          0u);
    const uint32_t* w = (const uint32_t*)(s.base + (size_t)e * s.bytes) + 4 * q;
    const int left = (s.bytes >> 2) - 4 * q;  // words of the segment from this unit on (the record's padding reads as zero)
    return make_uint4(w[0], left > 1 ? w[1] : 0u, left > 2 ? w[2] : 0u, left > 3 ? w[3] : 0u);
}

template <bool LOAD>
__device__ __forceinline__ void snap_put(const SnapLayout& L, const SnapSeg& s, int e, int q, uint8_t* rec, uint4 v) {
    if (!LOAD) {
        *(uint4*)(rec + s.off + 16 * q) = v;
    } else if (s.kind == CTF_SNAP_VEC) {
        *(uint4*)(s.base + (size_t)e * s.bytes + 16 * q) = v;
    } else if (s.kind == CTF_SNAP_RNG) {
        L.rngpos[2 * e] = v.x;
        L.rngpos[2 * e + 1] = v.y;
        L.rngready[2 * e] = (uint8_t)v.z;
        L.rngready[2 * e + 1] = (uint8_t)(v.z >> 8);
        L.rngage[2 * e] = (uint8_t)(v.z >> 16);
        L.rngage[2 * e + 1] = (uint8_t)(v.z >> 24);
    } else {
        uint32_t* w = (uint32_t*)(s.base + (size_t)e * s.bytes) + 4 * q;
        const int left = (s.bytes >> 2) - 4 * q;
        w[0] = v.x;
        if (left > 1) w[1] = v.y;
        if (left > 2) w[2] = v.z;
        if (left > 3) w[3] = v.w;
    }
}

template <bool LOAD>
__device__ __forceinline__ void snap_body(const SnapLayout& L, const int32_t* idx, uint8_t* recs, int k) {
    const int t = threadIdx.x;
    const int e = idx ? idx[k] : k;
    uint8_t* rec = recs + (size_t)k * L.bytes;
    const bool in_range = e >= 0 && e < L.n_envs;
    if (LOAD ? !(in_range && snap_header_ok(L, rec)) : !in_range) {
        if (!LOAD && t < CTF_SNAP_HEADER / 16) ((uint4*)rec)[t] = make_uint4(0u, 0u, 0u, 0u);
        if (t == 0) atomicOr(L.status, CTF_ST_BAD_SNAPSHOT);
        return;
    }
    if (!LOAD && t < CTF_SNAP_HEADER / 16) {
        uint4 h = make_uint4(0u, 0u, 0u, 0u);
        if (t == 0) h = make_uint4(CTF_SNAP_MAGIC, CTF_SNAP_VERSION, (uint32_t)L.fingerprint, (uint32_t)(L.fingerprint >> 32));
        if (t == 1) h.x = (uint32_t)L.bytes, h.y = (uint32_t)L.N;
        ((uint4*)rec)[t] = h;
    }
    for (int j = 0; j < L.n_segs; j++) {  // uniform
        const SnapSeg s = L.seg[j];
        const int units = (s.bytes + 15) >> 4;
        for (int q = t; q < units; q += 2 * SNAP_THREADS) {
            const bool two = q + SNAP_THREADS < units;
            const uint4 a = snap_fetch<LOAD>(L, s, e, q, rec);
            uint4 b = a;
            if (two) b = snap_fetch<LOAD>(L, s, e, q + SNAP_THREADS, rec);
            snap_put<LOAD>(L, s, e, q, rec, a);
            if (two) snap_put<LOAD>(L, s, e, q + SNAP_THREADS, rec, b);
        }
    }
    if (!LOAD) {  // the record's tail after the last segment (up to the 256-byte multiple) is zero
        const int end = L.off_vislog ? L.off_vislog + CTF_VIS_LOG * L.N * 2 : CTF_SNAP_HEADER + 16 * L.body_units;
        for (int o = end + 16 * t; o < L.bytes; o += 16 * SNAP_THREADS) *(uint4*)(rec + o) = make_uint4(0u, 0u, 0u, 0u);
    }
}

// rows of the vislog column, CNT 16-byte vectors per row (2N = 16 or 32 bytes): four rows in flight per lane
template <bool LOAD, int CNT>
__device__ __forceinline__ void snap_log_vec(const SnapLayout& L, int e, uint8_t* rec, int s0) {
    const size_t pitch = (size_t)L.n_envs * CNT;  // vectors between two slots of one env
    uint4* hbm = (uint4*)L.vislog + (size_t)s0 * pitch + (size_t)e * CNT;
    uint4* rows = (uint4*)(rec + L.off_vislog) + (size_t)s0 * CNT;
    uint4* src = LOAD ? rows : hbm;
    uint4* dst = LOAD ? hbm : rows;
    const size_t sp = LOAD ? CNT : pitch, dp = LOAD ? pitch : CNT;  // vectors between two slots on either side
    for (int s = 0; s < SNAP_LOG_SLOTS; s += 4) {
        const uint4* in = src + (size_t)s * sp;
        uint4* out = dst + (size_t)s * dp;
        const uint4 a0 = in[0], a1 = in[sp], a2 = in[2 * sp], a3 = in[3 * sp];
        uint4 b0, b1, b2, b3;
        if (CNT == 2) b0 = in[1], b1 = in[sp + 1], b2 = in[2 * sp + 1], b3 = in[3 * sp + 1];
        out[0] = a0, out[dp] = a1, out[2 * dp] = a2, out[3 * dp] = a3;
        if (CNT == 2) out[1] = b0, out[dp + 1] = b1, out[2 * dp + 1] = b2, out[3 * dp + 1] = b3;
    }
}

// any other N: rows of 2N bytes as elements of T, the widest the row's alignment allows
template <bool LOAD, typename T>
__device__ __forceinline__ void snap_log_rows(const SnapLayout& L, int e, uint8_t* rec, int s0) {
    const int cnt = L.N * 2 / (int)sizeof(T);
    const size_t pitch = (size_t)L.n_envs * cnt;
    T* hbm = (T*)L.vislog + (size_t)s0 * pitch + (size_t)e * cnt;
    T* rows = (T*)(rec + L.off_vislog) + (size_t)s0 * cnt;
#pragma unroll 4
    for (int s = 0; s < SNAP_LOG_SLOTS; s++)
        for (int c = 0; c < cnt; c++) {
            if (LOAD) hbm[(size_t)s * pitch + c] = rows[s * cnt + c];
            else rows[s * cnt + c] = hbm[(size_t)s * pitch + c];
        }
}

template <bool LOAD>
__device__ __forceinline__ void snap_log(const SnapLayout& L, const int32_t* idx, uint8_t* recs, int n, int w) {
    const int g = w / SNAP_LOG_CHUNKS, chunk = w - g * SNAP_LOG_CHUNKS;
    const int k = g * SNAP_WAVE + (threadIdx.x & (SNAP_WAVE - 1));
    if (k >= n) return;
    const int e = idx ? idx[k] : k;
    uint8_t* rec = recs + (size_t)k * L.bytes;
    if (e < 0 || e >= L.n_envs) return;  // (the body block raises the bit)
    if (LOAD && !snap_header_ok(L, rec)) return;
    const int s0 = chunk * SNAP_LOG_SLOTS;
    const int rb = L.N * 2;  // row bytes: the alignment of a row in HBM and in the record
    if (rb == 16) snap_log_vec<LOAD, 1>(L, e, rec, s0);
    else if (rb == 32) snap_log_vec<LOAD, 2>(L, e, rec, s0);
    else if (rb % 8 == 0) snap_log_rows<LOAD, uint2>(L, e, rec, s0);
    else if (rb % 4 == 0) snap_log_rows<LOAD, uint32_t>(L, e, rec, s0);
    else snap_log_rows<LOAD, uint16_t>(L, e, rec, s0);
}

// blocks [0, n): body of record `block`; blocks [n, ...): four vislog waves each
template <bool LOAD>
__device__ __forceinline__ void snap_kernel(const SnapLayout& L, const int32_t* idx, uint8_t* recs, int n) {
    if ((int)blockIdx.x < n) {
        snap_body<LOAD>(L, idx, recs, blockIdx.x);
        return;
    }
    const int w = ((int)blockIdx.x - n) * (SNAP_THREADS / SNAP_WAVE) + (int)(threadIdx.x / SNAP_WAVE);
    if (w < (n + SNAP_WAVE - 1) / SNAP_WAVE * SNAP_LOG_CHUNKS) snap_log<LOAD>(L, idx, recs, n, w);
}

extern "C" __global__ void __launch_bounds__(SNAP_THREADS) k_save_states(SnapLayout L, const int32_t* idx, uint8_t* recs, int n) {
    snap_kernel<false>(L, idx, recs, n);
}

extern "C" __global__ void __launch_bounds__(SNAP_THREADS) k_load_states(SnapLayout L, const int32_t* idx, const uint8_t* recs, int n) {
    snap_kernel<true>(L, idx, (uint8_t*)recs, n);
}

static dim3 snap_grid(const SnapLayout& L, int n) {
    const int log_waves = L.off_vislog ? (n + SNAP_WAVE - 1) / SNAP_WAVE * SNAP_LOG_CHUNKS : 0;
    return dim3((unsigned)(n + (log_waves + SNAP_THREADS / SNAP_WAVE - 1) / (SNAP_THREADS / SNAP_WAVE)));
}

extern "C" hipError_t ctf_launch_save_states(const SnapLayout& L, const int32_t* idx, int n, uint8_t* dst, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_save_states, snap_grid(L, n), dim3(SNAP_THREADS), 0, st, L, idx, dst, n);
    return hipGetLastError();
}

extern "C" hipError_t ctf_launch_load_states(const SnapLayout& L, const uint8_t* src, const int32_t* idx, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_load_states, snap_grid(L, n), dim3(SNAP_THREADS), 0, st, L, idx, src, n);
    return hipGetLastError();
}
