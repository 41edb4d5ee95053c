// effects_main.cpp — the rule of csrc/ctf_effects.h on the host: a stand-alone program (tests/test_effects_cpu.py builds it with
// -fsanitize=address,undefined) that reads env states and prints what eff_env_effects and eff_env_sample compute for them.
// Input (text, argv[1]): the number of cases, then per case
//   N G team_mask type_pack flag_pack spawn_pack home_flag_capture vault_cost vault_min agent_mask seed step env
//   followed by G*G grid codes, 2N position bytes, N has_flag bytes, N inventories, N hp values (hexadecimal floats: every bit of
//   the f64).
// Output: one line per case: N masks, 9N flag bytes, N sampled actions; an agent outside agent_mask shows the sentinels 9999 / 99 /
// 77 the program put there.
// Buffers are heap blocks of the exact sizes the functions may touch: the grid G*G bytes, the record
// f64 hp[N] | i8 pos[N][2] | u8 has_flag[N] | u8 perm[N] | i16 inv[N] as the library lays it out, the outputs N, 9N and N entries.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ctf_effects.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    int cases = 0;
    if (fscanf(in, "%d", &cases) != 1) return 2;
    for (int k = 0; k < cases; k++) {
        EffectArgs A;
        memset(&A, 0, sizeof(A));
        uint32_t agent_mask, step, env;
        uint64_t seed;
        if (fscanf(in, "%d %d %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %d %la %la %" SCNu32 " %" SCNu64 " %" SCNu32 " %" SCNu32, &A.N, &A.G,
                   &A.team_mask, &A.type_pack, &A.flag_pack, &A.spawn_pack, &A.home_flag_capture, &A.vault_cost, &A.vault_min, &agent_mask, &seed, &step,
                   &env) != 13)
            return 3;
        if (A.N < 1 || A.N > CTF_MAX_AGENTS || A.G < 1 || A.G > CTF_MAX_GRID) return 3;
        const int GG = A.G * A.G, N = A.N;
        A.GS = GG;
        A.off_hp = 0;
        A.off_pos = 8 * N;
        A.off_flag = 10 * N;
        A.off_inv = 12 * N;
        A.RS = 14 * N;
        A.n_envs = 1;
        uint8_t* grid = (uint8_t*)malloc((size_t)A.GS);
        uint8_t* rec = (uint8_t*)calloc((size_t)A.RS, 1);
        uint16_t* mask = (uint16_t*)malloc(sizeof(uint16_t) * (size_t)N);
        uint8_t* eff = (uint8_t*)malloc((size_t)N * CTF_N_ACTIONS);
        int8_t* act = (int8_t*)malloc((size_t)N);
        for (int c = 0; c < GG; c++) {
            int v;
            if (fscanf(in, "%d", &v) != 1) return 3;
            grid[c] = (uint8_t)v;
        }
        for (int j = 0; j < 3 * N; j++) {  // positions, then has_flag: adjacent in the record
            int v;
            if (fscanf(in, "%d", &v) != 1) return 3;
            rec[A.off_pos + j] = (uint8_t)(int8_t)v;
        }
        for (int j = 0; j < N; j++) {
            int v;
            if (fscanf(in, "%d", &v) != 1) return 3;
            const int16_t w = (int16_t)v;
            memcpy(rec + A.off_inv + 2 * j, &w, 2);
        }
        for (int j = 0; j < N; j++) {
            double hp;
            if (fscanf(in, "%la", &hp) != 1) return 3;
            memcpy(rec + A.off_hp + 8 * j, &hp, 8);
        }
        for (int i = 0; i < N; i++) mask[i] = 9999;
        memset(eff, 99, (size_t)N * CTF_N_ACTIONS);
        memset(act, 77, (size_t)N);
        eff_env_effects(A, grid, rec, agent_mask, mask, eff);
        eff_env_sample(A, grid, rec, agent_mask, seed, step, env, act);
        // either output alone gives the same
        uint16_t* mask2 = (uint16_t*)malloc(sizeof(uint16_t) * (size_t)N);
        uint8_t* eff2 = (uint8_t*)malloc((size_t)N * CTF_N_ACTIONS);
        memcpy(mask2, mask, sizeof(uint16_t) * (size_t)N);
        memcpy(eff2, eff, (size_t)N * CTF_N_ACTIONS);
        eff_env_effects(A, grid, rec, agent_mask, mask2, nullptr);
        eff_env_effects(A, grid, rec, agent_mask, nullptr, eff2);
        if (memcmp(mask2, mask, sizeof(uint16_t) * (size_t)N) || memcmp(eff2, eff, (size_t)N * CTF_N_ACTIONS)) return 4;
        for (int i = 0; i < N; i++) printf("%d ", (int)mask[i]);
        for (int i = 0; i < N * CTF_N_ACTIONS; i++) printf("%d ", (int)eff[i]);
        for (int i = 0; i < N; i++) printf("%d%c", (int)act[i], i + 1 < N ? ' ' : '\n');
        free(grid);
        free(rec);
        free(mask);
        free(eff);
        free(act);
        free(mask2);
        free(eff2);
    }
    fclose(in);
    printf("done %d\n", cases);
    return 0;
}
