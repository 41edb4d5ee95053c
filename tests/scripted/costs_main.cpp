// costs_main.cpp — the costs of csrc/ctf_scripted.h on the host: a stand-alone program (tests/test_scripted_costs_cpu.py builds it with
// -fsanitize=address,undefined) that reads env states and prints the costs scr_env_costs computes for them and, behind them, the
// actions scr_env_abilities computes for the same state and arguments without exploration (what the costs must be consistent with).
// Input (text, argv[1]): the number of cases, then per case
//   N G team_mask flag_pack type_pack vault_cost vault_min agent_mask role_pack ability_mask
//   followed by G*G grid codes, 2N position bytes, N has_flag bytes, N hp values (hexadecimal floats: every bit of the f64).
// Output: one line per case, N costs then N actions; an agent outside agent_mask shows the sentinels 9999 / 99 the program put there.
// Buffers are heap blocks of the exact sizes the functions may touch, as in abilities_main.cpp: the grid GS = G*G rounded up to 16
// bytes, the record f64 hp[N] | i8 pos[N][2] | u8 has_flag[N], the outputs N entries each.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ctf_scripted.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    int cases = 0;
    if (fscanf(in, "%d", &cases) != 1) return 2;
    for (int k = 0; k < cases; k++) {
        ScriptArgs A;
        ScriptAbil B;
        memset(&A, 0, sizeof(A));
        memset(&B, 0, sizeof(B));
        uint32_t agent_mask, ability_mask;
        uint64_t role_pack;
        if (fscanf(in, "%d %d %" SCNu32 " %" SCNu32 " %" SCNu32 " %la %la %" SCNu32 " %" SCNu64 " %" SCNu32, &A.N, &A.G, &A.team_mask, &A.flag_pack,
                   &B.type_pack, &B.vault_cost, &B.vault_min, &agent_mask, &role_pack, &ability_mask) != 10)
            return 3;
        if (A.N < 1 || A.N > CTF_MAX_AGENTS || A.G < 1 || A.G > CTF_MAX_GRID) return 3;
        const int GG = A.G * A.G;
        A.GS = (GG + 15) / 16 * 16;
        B.off_hp = 0;
        A.off_pos = 8 * A.N;
        A.off_flag = A.off_pos + 2 * A.N;
        A.RS = A.off_flag + A.N;
        A.n_envs = 1;
        uint8_t* grid = (uint8_t*)calloc((size_t)A.GS, 1);
        uint8_t* rec = (uint8_t*)calloc((size_t)A.RS, 1);
        int16_t* cost = (int16_t*)malloc(sizeof(int16_t) * (size_t)A.N);
        int8_t* act = (int8_t*)malloc((size_t)A.N);
        for (int c = 0; c < GG; c++) {
            int v;
            if (fscanf(in, "%d", &v) != 1) return 3;
            grid[c] = (uint8_t)v;
        }
        for (int j = 0; j < 3 * A.N; j++) {
            int v;
            if (fscanf(in, "%d", &v) != 1) return 3;
            rec[A.off_pos + j] = (uint8_t)(int8_t)v;
        }
        for (int j = 0; j < A.N; j++) {
            double hp;
            if (fscanf(in, "%la", &hp) != 1) return 3;
            memcpy(rec + B.off_hp + 8 * j, &hp, 8);
        }
        for (int i = 0; i < A.N; i++) cost[i] = 9999;
        memset(act, 99, (size_t)A.N);
        scr_env_costs(A, B, grid, rec, agent_mask, role_pack, ability_mask, cost);
        scr_env_abilities(A, B, grid, rec, agent_mask, role_pack, ability_mask, 0u, 0u, 0u, 0u, act);
        for (int i = 0; i < A.N; i++) printf("%d ", (int)cost[i]);
        for (int i = 0; i < A.N; i++) printf("%d%c", (int)act[i], i + 1 < A.N ? ' ' : '\n');
        free(grid);
        free(rec);
        free(cost);
        free(act);
    }
    fclose(in);
    printf("done %d\n", cases);
    return 0;
}
