/* Plain-C consumer of the trainer's entries in include/s2s_hip.h (the sibling of cabi_check.c): every s2s_trainer_* symbol
 * resolves, s2s_adam fills from C, and the refusals that need no GPU answer with their messages.
 * usage: cabi_check_train /path/to/libs2s_hip.so */
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>
#include "s2s_hip.h"

typedef size_t (*blob_floats_fn)(const s2s_config*);
typedef int (*create_fn)(const s2s_config*, const void*, size_t, int, s2s_trainer**);
typedef void (*destroy_fn)(s2s_trainer*);
typedef const char* (*last_error_fn)(const s2s_trainer*);
typedef int (*set_memory_fn)(s2s_trainer*, size_t);
typedef int64_t (*micro_batch_fn)(const s2s_trainer*, int32_t);
typedef int (*weights_fn)(s2s_trainer*, void*, float*);
typedef int (*gradients_fn)(s2s_trainer*, void*, const uint8_t*, const int32_t*, const float*, const float*, int32_t, float*, float*);
typedef int (*step_fn)(s2s_trainer*, void*, const uint8_t*, const int32_t*, const float*, const float*, int32_t, const s2s_adam*, float*);

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);             \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    void* lib = dlopen(argv[1], RTLD_NOW);
    if (!lib) { fprintf(stderr, "%s\n", dlerror()); return 2; }
    const char* names[] = {"s2s_trainer_create", "s2s_trainer_destroy", "s2s_trainer_last_error", "s2s_trainer_set_memory",
                           "s2s_trainer_micro_batch", "s2s_trainer_weights", "s2s_trainer_gradients", "s2s_trainer_step"};
    for (size_t i = 0; i < sizeof names / sizeof *names; ++i)
        if (!dlsym(lib, names[i])) { fprintf(stderr, "missing %s\n", names[i]); return 1; }
    blob_floats_fn blob_floats = (blob_floats_fn)dlsym(lib, "s2s_blob_floats");
    create_fn create = (create_fn)dlsym(lib, "s2s_trainer_create");
    destroy_fn destroy = (destroy_fn)dlsym(lib, "s2s_trainer_destroy");
    last_error_fn last_error = (last_error_fn)dlsym(lib, "s2s_trainer_last_error");
    set_memory_fn set_memory = (set_memory_fn)dlsym(lib, "s2s_trainer_set_memory");
    micro_batch_fn micro_batch = (micro_batch_fn)dlsym(lib, "s2s_trainer_micro_batch");
    weights_fn weights = (weights_fn)dlsym(lib, "s2s_trainer_weights");
    gradients_fn gradients = (gradients_fn)dlsym(lib, "s2s_trainer_gradients");
    step_fn step = (step_fn)dlsym(lib, "s2s_trainer_step");
    CHECK(blob_floats);

    s2s_adam hyper = {5e-4, 0.9, 0.999, 1e-7, 0.01, 1.0, 1, 1};
    CHECK(hyper.lr == 5e-4 && hyper.beta2 == 0.999 && hyper.clip == 1.0 && hyper.decoupled == 1 && hyper.step == 1);
    CHECK(sizeof(s2s_adam) == 6 * sizeof(double) + 2 * sizeof(int32_t));
    CHECK(S2S_TRAINER_DEFAULT_MEMORY == ((size_t)2 << 30));

    s2s_config cfg = {6, 5, 37, 48, 96, 3, 1, 1, 1, 165.0f, S2S_MODE_GENERIC_GEOMETRY, 1};
    const size_t n = blob_floats(&cfg);
    CHECK(n > 0);
    static float blob[1 << 17];
    CHECK(n <= sizeof blob / sizeof *blob);
    s2s_trainer* t = (s2s_trainer*)1;

    CHECK(create(&cfg, blob, n * sizeof(float), 0, NULL) == S2S_ERR_ARG && strstr(last_error(NULL), "out is NULL"));
    CHECK(create(NULL, blob, n * sizeof(float), 0, &t) == S2S_ERR_ARG && t == NULL && strstr(last_error(NULL), "NULL argument"));
    t = (s2s_trainer*)1;
    CHECK(create(&cfg, NULL, n * sizeof(float), 0, &t) == S2S_ERR_ARG && t == NULL && strstr(last_error(NULL), "NULL argument"));
    s2s_config other = cfg;
    other.compute_mode = S2S_MODE_GENERIC;
    other.max_dna_len = S2S_T_ENC;
    other.max_signal_len = S2S_T_DEC;
    CHECK(create(&other, blob, n * sizeof(float), 0, &t) == S2S_ERR_ARG && t == NULL && strstr(last_error(NULL), "S2S_MODE_GENERIC_GEOMETRY only"));
    other = cfg;
    other.dmodel = 20;                                        /* not a multiple of 16 */
    CHECK(create(&other, blob, n * sizeof(float), 0, &t) == S2S_ERR_ARG && t == NULL && strstr(last_error(NULL), "dmodel"));
    CHECK(create(&cfg, blob, n * sizeof(float) - 4, 0, &t) == S2S_ERR_BLOB && t == NULL && strstr(last_error(NULL), "weight blob is"));

    destroy(NULL);
    CHECK(set_memory(NULL, 1u << 20) == S2S_ERR_ARG);
    CHECK(micro_batch(NULL, 8) == S2S_ERR_ARG);
    CHECK(weights(NULL, NULL, blob) == S2S_ERR_ARG);
    CHECK(gradients(NULL, NULL, NULL, NULL, NULL, NULL, 1, NULL, NULL) == S2S_ERR_ARG);
    CHECK(step(NULL, NULL, NULL, NULL, NULL, NULL, 1, &hyper, NULL) == S2S_ERR_ARG);
    printf("CABI_TRAIN_OK %zu\n", n);
    return 0;
}
