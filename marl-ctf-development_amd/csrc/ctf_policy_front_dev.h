// ctf_policy_front_dev.h — the conv front of the policy network (agent_network.py:13-14,30-36), ONE definition of every piece the three
// forward kernels (k_policy_features, k_policy_features_team: ctf_policy.hip; k_policy_features_fact: ctf_policy_fact.hip) and the two
// backward kernels (k_policy_front_dgrad<.., true>, k_policy_front_wgrad) share.  Device only.  The forward kernels call the same
// code, so every output is the same sum in the same order in all three: they agree bit for bit.  (Two pieces have a second text,
// kept because the compiler schedules that kernel differently through the helper: k_policy_features' conv2 tile pair, which
// stores tile by tile, and k_policy_features_fact's prologue.  tests/test_gpu_policy_native.py and test_gpu_policy_fact.py pin the
// bit-for-bit agreement of the three.)
//
// The front's layout — one wave per sample (or per env), everything between the code bytes and the activation row stays on the CU:
//   h0  LDS bf16 [2 halves][G*G cells][8 ch]  the one-hot input, written straight from the codes (channel halves in separate
//           arrays: a lane's 16-byte operand reads then fall on consecutive addresses across lanes — no bank conflicts)
//   conv1 = 16x16x32 MFMAs: D[out ch][position] over K = (2 taps) x (16 in ch); A = weights, register-resident for the
//           whole launch; B = ds_read_b128 of h0 rows (a lane's 8 consecutive channels of one cell)
//   h1  LDS bf16 [2 halves][G1*G1 positions][8 ch]  tanh(conv1), written 8 bytes per lane from the accumulator layout
//   conv2 = 32x32x16 MFMAs: D[out ch][position], one MFMA per tap (K = 16 in ch), B = ds_read_b128 of h1 rows
//   out HBM bf16 [sample][Kp]            tanh(conv2) as 8-byte stores in the order the accumulators hold it:
//           column ((c/4) * PP + p) * 4 + c%4 for out channel c, position p (PP = positions rounded up to whole
//           32-position tiles, so that every store instruction covers whole 128-byte lines) — the fc1 weight's columns
//           are permuted to this order once on the host (policy_native.py), so no transpose happens anywhere; then the M
//           metadata values (f16 -> bf16) and padding up to Kp (a multiple of 64: rows are whole lines).
// tanh(x) = 1 - 2 / (2^(x * 2 log2 e) + 1): the factor 2 log2 e is folded into the conv weights and biases on the host,
// so a pair of activations costs 2 v_exp_f32, v_pk_add_f32, 2 v_rcp_f32, v_pk_fma_f32, v_cvt_pk_bf16_f32.
//
// The hand-placed prefetches and their counted waits (ctf_policy_dev.h) are NOT here: they stay in their kernels, in their iteration.
#pragma once
#include "ctf_policy_dev.h"

// four accumulator values (consecutive out channels of one position) -> their tanh as two packed bf16 pairs
__device__ __forceinline__ u32x2_t pol_tanh4(float z0, float z1, float z2, float z3) { return (u32x2_t){tanh2_pack(z0, z1), tanh2_pack(z2, z3)}; }
__device__ __forceinline__ u32x2_t pol_tanh4(const f32x4_t& acc) { return pol_tanh4(acc[0], acc[1], acc[2], acc[3]); }
__device__ __forceinline__ u32x2_t pol_tanh4(const f32x16_t& acc, int q) { return pol_tanh4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]); }

// One lane's dword of the metadata behind the conv features: the f16 pair `mw` as a bf16 pair (lane < M / 2); `one_column`: then ONE
// column of 1.0 (column 32 PP + M: a caller may keep fc1's bias in that column of its weight — the training path does, so that the bias
// gradient falls out of the weight-gradient GEMM; the inference weights hold zero there); zero padding behind it
__device__ __forceinline__ uint32_t pol_meta_word(uint32_t mw, int lane, int M, bool one_column) {
    if (lane < (M >> 1)) {
        const float lo = (float)__builtin_bit_cast(_Float16, (uint16_t)(mw & 0xFFFFu));
        const float hi = (float)__builtin_bit_cast(_Float16, (uint16_t)(mw >> 16));
        return pack_bf16(lo, hi);
    }
    return one_column && lane == (M >> 1) ? 0x3F80u : 0u;
}

// ---- launch-lifetime registers of a forward kernel: both convolutions' weights in MFMA A-operand order, the biases, the lane geometry
struct PolFront {
    u32x4_t w1[5], w2[9];
    f32x4_t bias1;
    f32x16_t bias2;
    int off1[5];           // conv1 B operand of K-step s: byte offset from the output position's own cell in h0
    int n1, g1;            // conv1: lane = (position n1 = lane & 15, k-group g1 = lane >> 4): taps 2 s + (g1 >> 1), channels 8 (g1 & 1) ..
    int y1_0, x1_0;        // position 16 t + n1 walks the G1 x G1 output row-major, from here ..
    int dy1, dx1;          // .. per tile it advances 16 = dy1 rows + dx1 columns
    uint8_t* h1w;          // conv1 output: this lane's 4 channels 4 g1 .. 4 g1 + 3 of position n1, as 8 bytes of half g1 >> 1
    int n2, hh;            // conv2: lane = (position n2 = lane & 31, channel half hh = lane >> 5)
};
// TG: the grid side, or 0 for a.G (k_policy_features<0>); h1: this wave's h1 image
template <int TG>
__device__ __forceinline__ void pol_front_prologue(PolFront& f, const PolicyArgs& a, uint8_t* h1) {
    const int G = TG ? TG : a.G, G1 = G - 2, lane = threadIdx.x & (WAVE - 1);
    const int H0A = G * G * 16, H1A = pol_h1_bytes(G) / 2;  // bytes of one channel-half array of h0 / h1
#pragma unroll
    for (int s = 0; s < 5; s++) f.w1[s] = a.w1frag[s * WAVE + lane];
#pragma unroll
    for (int t = 0; t < 9; t++) f.w2[t] = a.w2frag[t * WAVE + lane];
#pragma unroll
    for (int r = 0; r < 4; r++) f.bias1[r] = a.b1[(lane >> 4) * 4 + r];
#pragma unroll
    for (int r = 0; r < 16; r++) f.bias2[r] = a.b2[(r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)];
    f.n1 = lane & 15;
    f.g1 = lane >> 4;
#pragma unroll
    for (int s = 0; s < 5; s++) {
        const int tap = min(2 * s + (f.g1 >> 1), 8);  // "tap 9" has zero weights: any valid address
        f.off1[s] = ((tap / 3) * G + (tap % 3)) * 16 + (f.g1 & 1) * H0A;
    }
    f.y1_0 = (int)(((uint32_t)f.n1 * a.inv_g1) >> 16);
    f.x1_0 = f.n1 - f.y1_0 * G1;
    f.dy1 = 16 / G1;
    f.dx1 = 16 - f.dy1 * G1;
    f.h1w = h1 + (f.g1 >> 1) * H1A + f.n1 * 16 + (f.g1 & 1) * 8;
    f.n2 = lane & 31;
    f.hh = lane >> 5;
}

// ---- conv1: one 16-position tile whose lanes' own cells lie at `base` (in h0) -> the accumulators, bias included
__device__ __forceinline__ f32x4_t pol_conv1_tile(const PolFront& f, const uint8_t* base) {
    f32x4_t acc = f.bias1;
#pragma unroll
    for (int q = 0; q < 5; q++) {
        const u32x4_t b = *(const u32x4_t*)(base + f.off1[q]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(f.w1[q]), as_bf16x8(b), acc, 0, 0, 0);
    }
    return acc;
}
// conv1 + tanh of the whole image -> h1, T1 tiles ((G1 * G1 + 15) >> 4; 0: nothing).  (Positions >= P1 of the last tile read past h0
// into h1 — inside this wave's LDS — and land in h1 rows >= P1, which nothing reads.)
__device__ __forceinline__ void pol_conv1_pass(const PolFront& f, const uint8_t* h0, int G, int T1) {
    const int G1 = G - 2;
    int x1 = f.x1_0, cell1 = f.y1_0 * G + f.x1_0;
    // two tiles per pass: two independent accumulation chains keep the MFMA pipe and the LDS busy within one wave
    int t = 0;
#pragma unroll 1
    for (; t + 1 < T1; t += 2) {
        const uint8_t* base_a = h0 + ((POL_ABLATE & 8) ? 0 : cell1 * 16);
        x1 += f.dx1;
        cell1 += f.dy1 * G + f.dx1;
        if (x1 >= G1) { x1 -= G1; cell1 += G - G1; }
        const uint8_t* base_b = h0 + ((POL_ABLATE & 8) ? 64 : cell1 * 16);
        x1 += f.dx1;
        cell1 += f.dy1 * G + f.dx1;
        if (x1 >= G1) { x1 -= G1; cell1 += G - G1; }
        f32x4_t acc_a = f.bias1, acc_b = f.bias1;
#pragma unroll
        for (int q = 0; q < 5; q++) {
            const u32x4_t ba = *(const u32x4_t*)(base_a + f.off1[q]);
            const u32x4_t bb = *(const u32x4_t*)(base_b + f.off1[q]);
            acc_a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(f.w1[q]), as_bf16x8(ba), acc_a, 0, 0, 0);
            acc_b = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(f.w1[q]), as_bf16x8(bb), acc_b, 0, 0, 0);
        }
        *(u32x2_t*)(f.h1w + 16 * t * 16) = pol_tanh4(acc_a);  // rows up to 16 * T1 exist
        *(u32x2_t*)(f.h1w + 16 * (t + 1) * 16) = pol_tanh4(acc_b);
    }
    if (t < T1)  // odd tile count: the last one alone
        *(u32x2_t*)(f.h1w + 16 * t * 16) = pol_tanh4(pol_conv1_tile(f, h0 + ((POL_ABLATE & 8) ? 0 : cell1 * 16)));
}

// ---- conv2: one 32-position tile whose lanes' top-left inputs lie at `base` (in h1, this lane's channel half; rows of G1 cells)
__device__ __forceinline__ f32x16_t pol_conv2_tile(const PolFront& f, const uint8_t* base, int G1) {
    f32x16_t acc = f.bias2;
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const u32x4_t b = *(const u32x4_t*)(base + ((tap / 3) * G1 + (tap % 3)) * 16);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(f.w2[tap]), as_bf16x8(b), acc, 0, 0, 0);
    }
    return acc;
}
// conv2 + tanh of the tiles t, t + 1 (positions pa = 32 t + n2 and pb = pa + 32; past the image's end: the last position again), two
// accumulation chains side by side.  store(q, oa, ob) takes the out channels 8 q + 4 hh .. + 3 of pa and of pb — where they go is all
// the two shared-view kernels differ in (k_policy_features: see there).
template <typename Store>
__device__ __forceinline__ void pol_conv2_pair(const PolFront& f, const uint8_t* h1, int H1A, int G, uint32_t inv_g2, int t, Store store) {
    const int G1 = G - 2, G2 = G - 4, P2 = G2 * G2;
    const int pa = 32 * t + f.n2, pb = pa + 32;
    const int pca = min(pa, P2 - 1), pcb = min(pb, P2 - 1);
    const int ya = (int)(((uint32_t)pca * inv_g2) >> 16), yb = (int)(((uint32_t)pcb * inv_g2) >> 16);
    const uint8_t* base_a = h1 + ((POL_ABLATE & 8) ? 0 : (ya * G1 + (pca - ya * G2)) * 16 + f.hh * H1A);
    const uint8_t* base_b = h1 + ((POL_ABLATE & 8) ? 64 : (yb * G1 + (pcb - yb * G2)) * 16 + f.hh * H1A);
    f32x16_t acc_a = f.bias2, acc_b = f.bias2;
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const int off = ((tap / 3) * G1 + (tap % 3)) * 16;
        const u32x4_t ba = *(const u32x4_t*)(base_a + off);
        const u32x4_t bb = *(const u32x4_t*)(base_b + off);
        acc_a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(f.w2[tap]), as_bf16x8(ba), acc_a, 0, 0, 0);
        acc_b = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(f.w2[tap]), as_bf16x8(bb), acc_b, 0, 0, 0);
    }
    if ((POL_ABLATE & 1) ? (acc_a[0] == 12345.0f && acc_b[5] == 1.0f) : true) {
#pragma unroll
        for (int q = 0; q < 4; q++) store(q, pol_tanh4(acc_a, q), pol_tanh4(acc_b, q));
    }
}

// ---- the backward's position contraction (conv2's weight gradient in k_policy_front_dgrad<.., true>, either one in k_policy_front_wgrad)
typedef short i16x4_t __attribute__((ext_vector_type(4)));
// two transposed 4-position blocks (4 positions apart) -> one 8-position MFMA operand of this lane's channel
__device__ __forceinline__ u32x4_t wgrad_tr_operand(const uint8_t* lds_addr, int second_block_bytes) {
    typedef __attribute__((address_space(3))) i16x4_t* lds_v4;
    const i16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(lds_addr));
    const i16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(lds_addr + second_block_bytes));
    const u32x2_t l2 = __builtin_bit_cast(u32x2_t, lo), h2 = __builtin_bit_cast(u32x2_t, hi);
    return (u32x4_t){l2[0], l2[1], h2[0], h2[1]};
}
// dW[o][i][tap] += sum over positions of grad[o][y][x] * img[i][y + dy][x + dx], NH halves of 16 out channels.  K-step ks = gradient
// rows 2 ks, 2 ks + 1 of 16 columns; tap (dy, dx) reads the activation rows + dy from column + dx on.  The operands come through the
// transposing read, whose lanes may point anywhere (all 64 lanes must be active).  ga / gb: this lane's addresses for K-step 0, tap
// (0, 0) in the gradient / the activation image; g_half: bytes from one 16-channel half of the out channels to the next; g_row / b_row:
// bytes of an image row, g_pos / b_pos: of a position.
template <int NH>
__device__ __forceinline__ void pol_wgrad_contract(f32x4_t (&acc)[9][NH], int KS, const uint8_t* ga, int g_half, int g_row, int g_pos,
                                                   const uint8_t* gb, int b_row, int b_pos) {
#pragma unroll 1
    for (int ks = 0; ks < KS; ks++) {
        u32x4_t av[NH];
#pragma unroll
        for (int h = 0; h < NH; h++) av[h] = wgrad_tr_operand(ga + h * g_half + ks * 2 * g_row, 4 * g_pos);
#pragma unroll
        for (int t = 0; t < 9; t++) {
            const u32x4_t bv = wgrad_tr_operand(gb + (ks * 2 + t / 3) * b_row + (t % 3) * b_pos, 4 * b_pos);
#pragma unroll
            for (int h = 0; h < NH; h++) acc[t][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(av[h]), as_bf16x8(bv), acc[t][h], 0, 0, 0);
        }
    }
}
// The block's per-wave tap accumulators -> one sum (through `red`, the block's LDS: float [wave][9 taps][CO][16], free by now) -> the
// gradient dw [CO][16][9] by atomicAdd, or (deterministic mode: `part` not NULL) block b's own slice part + b * part_stride.  D tile: a lane holds rows
// m = 4 (lane >> 4) + r of column n = lane & 15.
template <int NH>
__device__ __forceinline__ void pol_wgrad_reduce(const f32x4_t (&acc)[9][NH], float* red, int wave, int wpb, int lane, float* dw, float* part,
                                                 size_t part_stride) {
    constexpr int CO = 16 * NH;
    const int mn = lane & 15, kg = lane >> 4;
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; t++)
#pragma unroll
        for (int h = 0; h < NH; h++)
#pragma unroll
            for (int r = 0; r < 4; r++) red[((wave * 9 + t) * CO + 16 * h + 4 * kg + r) * 16 + mn] = acc[t][h][r];
    __syncthreads();
    for (int e = threadIdx.x; e < 9 * CO * 16; e += blockDim.x) {
        float v = 0.0f;
        for (int w = 0; w < wpb; w++) v += red[w * 9 * CO * 16 + e];
        const int t = e / (CO * 16), oi = e - t * (CO * 16);
        if (part) part[(size_t)blockIdx.x * part_stride + (size_t)oi * 9 + t] = v;
        else atomicAdd(dw + (size_t)oi * 9 + t, v);  // [out][in][tap]
    }
}
