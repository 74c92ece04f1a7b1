/* Build container: what does a refused call of gclm_perspective_fields and of gclm_field_errors cost on the host?  Each call
 * is refused late (a misaligned d_lat, a misaligned latitude map) and no HIP call is made; the addresses are fake.  Before
 * the entries moved onto csrc/gclm_args.h, gclm_perspective_fields tested the alignment of both outputs BEFORE any range
 * arithmetic, so its misaligned d_lat skipped that arithmetic; the third case, a d_lat that overlaps the gravity, is the one
 * that was refused at that entry's last check, after every other one had run.  Run by `scripts/abi_refusals.py REV --cost`:
 *   cc -O2 scripts/probes/refusal_cost.c -o refusal_cost -ldl && ./refusal_cost LIB_AT_REV LIB_OF_THE_TREE [calls=1000000] [reps=5]
 * Prints one JSON object: ns per call, `reps` repetitions per library, the two libraries alternating. */
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
#include <unistd.h>

typedef int (*persp_fn)(int, const float*, const float*, int, int, int, int, float*, float*, void*);
typedef int (*errs_fn)(int, const float*, const float*, int, int, int, const float*, const float*, const float*, const float*, int,
                       const float*, void*, size_t, float*, float*, float*, void*);

#define AT(i) ((float*)(uintptr_t)(0x10000000ull * ((i) + 1)))

static const float thr[4] = {1.f, 3.f, 5.f, 10.f};
static int persp(void* f) { return ((persp_fn)f)(1, AT(0), AT(1), 2, 48, 64, 1, AT(2), (float*)((char*)AT(3) + 2), NULL); }
static int persp_last(void* f) { return ((persp_fn)f)(1, AT(0), AT(1), 2, 48, 64, 1, AT(2), (float*)((char*)AT(1) + 20), NULL); }
static int errs(void* f) {
    return ((errs_fn)f)(1, AT(0), AT(1), 2, 48, 64, AT(2), AT(3), AT(4), AT(5), 4, thr, AT(6), (size_t)1 << 24, AT(7), AT(8),
                        (float*)((char*)AT(9) + 2), NULL);
}

static double ns_per_call(int (*call)(void*), void* f, long calls) {
    struct timespec t0, t1;
    long refused = 0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (long i = 0; i < calls; ++i) refused += call(f) == -3;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    if (refused != calls) { fprintf(stderr, "a call was not refused\n"); exit(2); }
    return ((t1.tv_sec - t0.tv_sec) * 1e9 + (t1.tv_nsec - t0.tv_nsec)) / calls;
}

int main(int argc, char** argv) {
    if (argc < 3) return 1;
    if (access("/dev/kfd", F_OK) == 0) { fprintf(stderr, "a HIP device is visible: the addresses here are fake\n"); return 3; }
    const long calls = argc > 3 ? atol(argv[3]) : 1000000;
    const int reps = argc > 4 ? atoi(argv[4]) : 5;
    const char* names[3] = {"gclm_perspective_fields", "gclm_field_errors", "gclm_perspective_fields"};
    const char* cases[3] = {"", "", " (d_lat overlaps the gravity)"};
    int (*drivers[3])(void*) = {persp, errs, persp_last};
    void* libs[2];
    for (int l = 0; l < 2; ++l)
        if (!(libs[l] = dlopen(argv[1 + l], RTLD_NOW | RTLD_LOCAL))) { fprintf(stderr, "%s\n", dlerror()); return 1; }
    printf("{\"calls\": %ld", calls);
    for (int e = 0; e < 3; ++e) {
        double ns[2][64];
        void* f[2] = {dlsym(libs[0], names[e]), dlsym(libs[1], names[e])};
        if (!f[0] || !f[1] || reps > 64) return 1;
        ns_per_call(drivers[e], f[0], calls / 10);          /* warm both */
        ns_per_call(drivers[e], f[1], calls / 10);
        for (int r = 0; r < reps; ++r)
            for (int l = 0; l < 2; ++l) ns[l][r] = ns_per_call(drivers[e], f[l], calls);
        printf(", \"%s%s\": {", names[e], cases[e]);
        for (int l = 0; l < 2; ++l) {
            printf("%s\"%s\": [", l ? ", " : "", l ? "tree" : "rev");
            for (int r = 0; r < reps; ++r) printf("%s%.2f", r ? ", " : "", ns[l][r]);
            printf("]");
        }
        printf("}");
    }
    printf("}\n");
    return 0;
}
