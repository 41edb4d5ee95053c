// scatter_main.cpp — the rule of csrc/ctf_scatter.h on the host: a stand-alone program (tests/test_scatter_cpu.py builds it with
// -fsanitize=address,undefined) that runs sct_env_reset on one env per case and prints what the env then holds.
// Input (text, argv[1]): the number of cases, then per case
//   N G team_mask type_pack flag_pack log_metrics agent_mask radius flags seed env r
//   followed by four type hp values (hexadecimal floats), 2N start position bytes and G*G init grid codes.
// Output: one line per case: N cells | G*G grid codes | 2N position bytes | N has_flag | N inventories | N perm bytes | N hp (f64 bits)
// | step, captures 0 and 1, misc[3] | the sum of the counters | per agent the sum of its base map and the index of its largest word.
// Buffers are heap blocks of the exact sizes the function may touch — the grid GS bytes, the record RS bytes in the library's layout,
// 13 N counters, N * GS map words — filled with sentinels first: the record with 0xAB (`perm` must keep it), the counters with 5, the
// maps with 7 (an env nobody moved in keeps them: sum 7 GS).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ctf_scatter.h"

static int round_up(int x, int a) { return (x + a - 1) / a * a; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    int cases = 0;
    if (fscanf(in, "%d", &cases) != 1) return 2;
    for (int k = 0; k < cases; k++) {
        ScatterArgs A;
        memset(&A, 0, sizeof(A));
        uint32_t agent_mask, flags, env, r;
        int32_t radius;
        uint64_t seed;
        if (fscanf(in, "%d %d %" SCNu32 " %" SCNu32 " %" SCNu32 " %d %" SCNu32 " %d %" SCNu32 " %" SCNu64 " %" SCNu32 " %" SCNu32, &A.N, &A.G, &A.team_mask,
                   &A.type_pack, &A.flag_pack, &A.log_metrics, &agent_mask, &radius, &flags, &seed, &env, &r) != 12)
            return 3;
        if (A.N < 1 || A.N > CTF_MAX_AGENTS || A.G < 1 || A.G > CTF_MAX_GRID) return 3;
        const int N = A.N;
        A.GG = A.G * A.G;
        A.GS = round_up(A.GG, 16);
        A.off_pos = 8 * N;
        A.off_flag = 10 * N;
        const int off_perm = 11 * N;
        A.off_inv = 12 * N;
        A.off_misc = round_up(14 * N, 4);
        A.RS = round_up(A.off_misc + 16, 16);
        A.n_envs = 1;
        for (int t = 0; t < 4; t++) {
            double hp;
            if (fscanf(in, "%la", &hp) != 1) return 3;
            memcpy(&A.type_hp_bits[t], &hp, 8);
        }
        for (int j = 0; j < 2 * N; j++) {
            int v;
            if (fscanf(in, "%d", &v) != 1) return 3;
            A.start_pos[j / 2][j % 2] = (int8_t)v;
        }
        uint8_t* init = (uint8_t*)calloc((size_t)A.GS, 1);
        for (int c = 0; c < A.GG; c++) {
            int v;
            if (fscanf(in, "%d", &v) != 1) return 3;
            init[c] = (uint8_t)v;
        }
        A.init_grid = init;
        uint8_t* grid = (uint8_t*)malloc((size_t)A.GS);
        uint8_t* rec = (uint8_t*)malloc((size_t)A.RS);
        int32_t* metrics = (int32_t*)malloc(sizeof(int32_t) * (size_t)CTF_N_METRICS * (size_t)N);
        uint32_t* vis = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)N * (size_t)A.GS);
        int* cells = (int*)malloc(sizeof(int) * (size_t)N);
        memset(grid, 0xCD, (size_t)A.GS);
        memset(rec, 0xAB, (size_t)A.RS);
        for (int w = 0; w < CTF_N_METRICS * N; w++) metrics[w] = 5;
        for (int w = 0; w < N * A.GS; w++) vis[w] = 7u;
        // the kernel's form of the radius test, sixteen cells at a time, is sct_near on every cell of the grid — and nothing past it
        for (int i = 0; i < N; i++)
            for (int base = 0; base < CTF_MAX_CELLS; base += 16) {
                const uint32_t bits = sct_near16(A.G, base, base / A.G, (base + 15) / A.G, A.start_pos[i][0], A.start_pos[i][1], radius);
                for (int j = 0; j < 16; j++) {
                    const int c = base + j;
                    const bool want = c < A.GG && sct_near(c / A.G, c % A.G, A.start_pos[i][0], A.start_pos[i][1], radius);
                    if (((bits >> j) & 1u) != (want ? 1u : 0u) || (bits >> 16)) return 5;
                }
            }
        sct_env_reset(A, grid, rec, metrics, vis, agent_mask, radius, flags, seed, env, r, cells);
        for (int i = 0; i < N; i++) printf("%d ", cells[i]);
        for (int c = 0; c < A.GG; c++) printf("%d ", (int)grid[c]);
        for (int c = A.GG; c < A.GS; c++)
            if (grid[c] != 0) return 4;  // pad cells are the init grid's: zero
        for (int j = 0; j < 2 * N; j++) printf("%d ", (int)(int8_t)rec[A.off_pos + j]);
        for (int i = 0; i < N; i++) printf("%d ", (int)rec[A.off_flag + i]);
        for (int i = 0; i < N; i++) {
            int16_t v;
            memcpy(&v, rec + A.off_inv + 2 * i, 2);
            printf("%d ", (int)v);
        }
        for (int i = 0; i < N; i++) printf("%d ", (int)rec[off_perm + i]);
        for (int i = 0; i < N; i++) {
            uint64_t b;
            memcpy(&b, rec + 8 * i, 8);
            printf("%" PRIu64 " ", b);
        }
        for (int m = 0; m < 4; m++) {
            int32_t v;
            memcpy(&v, rec + A.off_misc + 4 * m, 4);
            printf("%d ", (int)v);
        }
        long long msum = 0;
        for (int w = 0; w < CTF_N_METRICS * N; w++) msum += metrics[w];
        printf("%lld", msum);
        for (int i = 0; i < N; i++) {
            unsigned long long sum = 0;
            int best = 0;
            for (int c = 0; c < A.GS; c++) {
                sum += vis[(size_t)i * A.GS + c];
                if (vis[(size_t)i * A.GS + c] > vis[(size_t)i * A.GS + best]) best = c;
            }
            printf(" %llu %d", sum, best);
        }
        printf("\n");
        free(init);
        free(grid);
        free(rec);
        free(metrics);
        free(vis);
        free(cells);
    }
    fclose(in);
    printf("done %d\n", cases);
    return 0;
}
