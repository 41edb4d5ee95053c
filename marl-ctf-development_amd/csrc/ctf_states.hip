// ctf_states.hip — env states as plain arrays on the device (ctf_export_states / ctf_import_states; ctf_states.h has the
// conversion, the check and the layout of a row).
//
// Both kernels are data movement: ST_LPR = 16 lanes per record, a 256-thread block takes 16 consecutive records.  The 16 lanes of
// a record walk each block of its env (rec, grid, metric, vis) and each row of the caller's arrays word by word, lane t taking
// words t, t + 16, ...: a wave's four records touch four runs of 64 contiguous bytes per access, and for consecutive indices the
// rows of the four records are adjacent in every array.  An array that is NULL costs one uniform test.
// Export: an index outside [0, E) writes nothing for that record and raises CTF_ST_BAD_GROUP (ctf_export_visitation's rule).
// Import: the lanes of a record first check their share of the row (ctf_set_state's rules, states_check), the verdicts are
// combined with one ballot per wave, and only a record that passed whole is written; one that failed, or whose index is outside
// [0, E), writes nothing and raises CTF_ST_BAD_STATE.  Every index is range-checked before it forms an address; lanes past n
// neither load nor store.  Plain C++ loads and stores; the status bits are raised with a vector atomic OR.
#include <hip/hip_runtime.h>

#include "ctf_launch.h"
#include "ctf_states.h"

#define ST_THREADS 256
#define ST_LPR 16                       // lanes per record
#define ST_RPB (ST_THREADS / ST_LPR)    // records per block

extern "C" __global__ void __launch_bounds__(ST_THREADS) k_export_states(StateShape S, StateDev D, const int32_t* idx, int n, StateArrays out) {
    const int t = (int)threadIdx.x & (ST_LPR - 1);
    const size_t k = (size_t)blockIdx.x * ST_RPB + threadIdx.x / ST_LPR;
    if (k >= (size_t)n) return;
    const int e = idx ? idx[k] : (int)k;
    if (e < 0 || e >= S.n_envs) {
        if (t == 0) atomicOr(D.status, CTF_ST_BAD_GROUP);
        return;
    }
    const uint8_t* met = D.metrics ? (const uint8_t*)(D.metrics + (size_t)e * CTF_N_METRICS * S.N) : nullptr;
    states_unpack(S, D.rec + (size_t)e * S.RS, D.grid + (size_t)e * S.GS, met, out, k, t, ST_LPR);
}

extern "C" __global__ void __launch_bounds__(ST_THREADS) k_import_states(StateShape S, StateDev D, StateArrays in, const int32_t* idx, int n) {
    const int t = (int)threadIdx.x & (ST_LPR - 1);
    const size_t k = (size_t)blockIdx.x * ST_RPB + threadIdx.x / ST_LPR;
    const bool live = k < (size_t)n;
    int e = -1;
    bool ok = true;
    if (live) {
        e = idx ? idx[k] : (int)k;
        ok = e >= 0 && e < S.n_envs && states_check(S, in, k, t, ST_LPR);
    }
    // the verdict of a record = the AND over its 16 lanes (every lane of the wave takes part in the ballot)
    const unsigned long long bad = __ballot(!ok);
    const int lane = (int)(threadIdx.x & 63);
    const bool good = ((bad >> (lane & ~(ST_LPR - 1))) & ((1ull << ST_LPR) - 1)) == 0;
    if (!live) return;
    if (!good) {
        if (t == 0) atomicOr(D.status, CTF_ST_BAD_STATE);
        return;
    }
    states_pack(S, in, k, D.rec + (size_t)e * S.RS, D.grid + (size_t)e * S.GS, D.metrics ? D.metrics + (size_t)e * CTF_N_METRICS * S.N : nullptr,
                D.vis ? D.vis + (size_t)e * S.N * S.GS : nullptr, t, ST_LPR);
}

extern "C" hipError_t ctf_launch_export_states(const StateShape& S, const StateDev& D, const int32_t* idx, int n, const StateArrays& out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_export_states, dim3((unsigned)((n + ST_RPB - 1) / ST_RPB)), dim3(ST_THREADS), 0, st, S, D, idx, n, out);
    return hipGetLastError();
}

extern "C" hipError_t ctf_launch_import_states(const StateShape& S, const StateDev& D, const StateArrays& in, const int32_t* idx, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_import_states, dim3((unsigned)((n + ST_RPB - 1) / ST_RPB)), dim3(ST_THREADS), 0, st, S, D, in, idx, n);
    return hipGetLastError();
}
static_assert(64 % ST_LPR == 0 && ST_THREADS % 64 == 0, "a record's lanes lie in one wave");
