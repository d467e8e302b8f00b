/* Stand-alone address / undefined-behaviour sanitizer run of the oracle's environment lookup (tests/test_env_sampler_cpu.py builds and
 * runs it):  env_sampler_sanitize_main <file of directions: int32 n, then n * 3 binary32>
 * Every cube is a heap block of exactly its own size, so a tap read outside the cube is a heap-buffer-overflow report and a non-zero
 * exit.  Sizes 3 and 255, both formats, every direction of the file (the test's finite sets and its NaN / inf / zero / subnormal ones). */
#include "../oracle/pt_oracle.c"
#include <stdio.h>

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    int n = 0;
    if (!f || fread(&n, 4, 1, f) != 1 || n <= 0) return 2;
    float *dirs = malloc((size_t)n * 12), *out = malloc((size_t)n * 12);
    if (fread(dirs, 12, (size_t)n, f) != (size_t)n) return 2;
    fclose(f);
    const int sizes[2] = { 3, 255 };
    for (int k = 0; k < 2; k++)
        for (int format = 0; format < 2; format++) {
            const int S = sizes[k];
            const size_t texels = (size_t)6 * S * S;
            void *cube = malloc(texels * (format ? 4 : 16));
            for (size_t i = 0; i < texels * 4; i++) {
                if (format) ((uint8_t *)cube)[i] = (uint8_t)(17 + i % 200);
                else ((float *)cube)[i] = 0.5f + (float)(i % 37);
            }
            pto_sample_env_n(cube, S, format, dirs, n, out);
            for (int i = 0; i < 3 * n; i++)
                if (!(out[i] >= 0.0f && out[i] <= 37.5f)) { printf("size %d format %d direction %d: %g\n", S, format, i / 3, out[i]); return 1; }
            int *idx = malloc((size_t)24 * S * 3 * sizeof(int));
            pto_env_wrapped_index(S, idx);
            free(idx);
            free(cube);
        }
    free(dirs); free(out);
    printf("ok %d directions\n", n);
    return 0;
}
