/* babe_restore: blind bandwidth extension of one clip batch from C - no Python, no torch in the process.
 *
 *     babe_restore model.babe in.f32 out.f32 [--seed N] [--T n] [--batch B] [--params out_params.f32] [--precision f32|bf16|bf16x3]
 *                  [--attention f32|bf16] [--fir NUMTAPS FC WIDTH | --declip C]
 *
 * model.babe: written by `python -m babe_amd.export`.  in.f32: B * L float32 samples at the model's rate (L and the rate are the
 * model's: babe_model_info), B clips one after the other.  out.f32: the B * L restored samples.  --params: the estimated filter
 * of each clip, B * 2 * K float32 (K cut-off frequencies in Hz, then K slopes in dB).  --T: sampling steps (default: the file's
 * tester.T); --seed: the noise is the library's counter-based generator under this seed (default 0), so the output is a function
 * of (model, input, seed, T, precision).  --precision: the conv arithmetic the loader packs the file's fp32 weights for (default
 * f32; bf16 is the fast one).  --attention: the core a model with time-attention layers runs them on (without it such a file is
 * refused).  --fir: the input was degraded by a KNOWN low-pass FIR - scipy.signal.firwin(NUMTAPS, FC, width=WIDTH,
 * window="kaiser", fs=the model's rate), designed here by babe_firwin_kaiser - and is restored against it, no filter is fitted;
 * --declip: the input was clipped at +-C and is restored against the clip.  With either, --params writes the initial filter back.
 * Links against libbabe_hip.so and the HIP runtime (babe_amd/build.py::build_example).
 * Exit status: 0, or 1 with the failing step and babe_last_error() on stderr. */
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "babe_hip.h"

#define FAIL(...) do { fprintf(stderr, "babe_restore: " __VA_ARGS__); fprintf(stderr, "\n"); goto done; } while (0)
#define LIB(call, what) do { if ((call) != 0) FAIL("%s: %s", what, babe_last_error()); } while (0)
#define HIP(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) FAIL("%s: %s", what, hipGetErrorString(e_)); } while (0)

static int precision_of(const char* s) {
    return !strcmp(s, "f32") ? BABE_PRECISION_F32 : !strcmp(s, "bf16") ? BABE_PRECISION_BF16 : !strcmp(s, "bf16x3") ? BABE_PRECISION_BF16X3 : -1;
}

static int attention_of(const char* s) { return !strcmp(s, "f32") ? BABE_ATTENTION_F32 : !strcmp(s, "bf16") ? BABE_ATTENTION_BF16 : -1; }

static double setting(const void* model, const char* key, double fallback) {
    double v;
    return babe_model_setting(model, key, &v) == 0 ? v : fallback;
}

/* the known low-pass FIR into the descriptor: taps designed in double, rounded to float32 once, copied to the device (*taps_dev is
 * the caller's to free).  0, or -1 with the message printed. */
static int observe_fir(babe_eval_desc* e, int numtaps, double fc, double width, double fs, float** taps_dev) {
    int rc = -1;
    double* h = (double*)malloc((size_t)(numtaps > 0 ? numtaps : 1) * sizeof *h);
    float* hf = (float*)malloc((size_t)(numtaps > 0 ? numtaps : 1) * sizeof *hf);
    if (!h || !hf) fprintf(stderr, "babe_restore: out of memory\n");
    else if (babe_firwin_kaiser(numtaps, fc, width, fs, 0, h) != 0) fprintf(stderr, "babe_restore: --fir: %s\n", babe_last_error());
    else {
        for (int i = 0; i < numtaps; ++i) hf[i] = (float)h[i];
        if (hipMalloc((void**)taps_dev, (size_t)numtaps * sizeof(float)) != hipSuccess ||
            hipMemcpy(*taps_dev, hf, (size_t)numtaps * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            fprintf(stderr, "babe_restore: --fir: the taps could not be copied to the device\n");
        else {
            e->obs_kind = BABE_OBS_FIR, e->taps = *taps_dev, e->ntaps = numtaps, e->blind = 0;
            rc = 0;
        }
    }
    free(h), free(hf);
    return rc;
}

int main(int argc, char** argv) {
    int status = 1, B = 1, T = 0, precision = BABE_PRECISION_F32, attention = BABE_ATTENTION_REFUSE, fir_n = 0;
    double fir_fc = 0, fir_width = 0, declip = -1;
    long seed = 0;
    const char* params_path = NULL;
    void *model = NULL, *state = NULL, *ws = NULL;
    float *y = NULL, *x = NULL, *params = NULL, *host = NULL, *host_params = NULL, *taps = NULL;
    babe_sample_step* steps = NULL;
    FILE* fh = NULL;
    if (argc < 4) {
        fprintf(stderr, "usage: babe_restore model.babe in.f32 out.f32 [--seed N] [--T n] [--batch B] [--params out_params.f32] "
                        "[--precision f32|bf16|bf16x3] [--attention f32|bf16] [--fir NUMTAPS FC WIDTH | --declip C]\n");
        return 2;
    }
    for (int i = 4; i < argc; ++i) {
        if (i + 1 >= argc) FAIL("option %s needs a value", argv[i]);
        if (!strcmp(argv[i], "--seed")) seed = atol(argv[++i]);
        else if (!strcmp(argv[i], "--T")) T = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--batch")) B = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--params")) params_path = argv[++i];
        else if (!strcmp(argv[i], "--precision")) {
            if ((precision = precision_of(argv[++i])) < 0) FAIL("--precision is one of f32, bf16, bf16x3");
        }
        else if (!strcmp(argv[i], "--attention")) {
            if ((attention = attention_of(argv[++i])) < 0) FAIL("--attention is one of f32, bf16");
        }
        else if (!strcmp(argv[i], "--fir")) {
            if (i + 3 >= argc) FAIL("--fir needs NUMTAPS FC WIDTH");
            fir_n = atoi(argv[i + 1]), fir_fc = atof(argv[i + 2]), fir_width = atof(argv[i + 3]), i += 3;
            if (fir_n < 1) FAIL("--fir: NUMTAPS must be at least 1");
        }
        else if (!strcmp(argv[i], "--declip")) {
            if ((declip = atof(argv[++i])) < 0) FAIL("--declip: C must not be negative");
        }
        else FAIL("unknown option %s", argv[i]);
    }
    if (B < 1) FAIL("--batch must be at least 1");
    if (fir_n && declip >= 0) FAIL("--fir and --declip exclude each other");
    const int known = fir_n || declip >= 0;

    /* [core] the listing of INTEGRATION.md section 2 */
    /* 1. the network: weights, packed images, CQT plan, STFT tables - one handle, one device arena */
    const babe_model_options options = {precision, attention, {0}};      /* attention: REFUSE unless --attention chose a core */
    model = babe_model_load_opt(argv[1], &options, NULL);
    if (!model) FAIL("babe_model_load_opt: %s", babe_last_error());
    babe_model_summary info;
    LIB(babe_model_info(model, &info), "babe_model_info");
    const long L = info.L;

    /* 2. one evaluation's bookkeeping (one per concurrent stream), 3. the descriptor with the file's sampler defaults */
    state = babe_unet_state_create();
    if (!state) FAIL("babe_unet_state_create failed");
    babe_sample_desc d;
    memset(&d, 0, sizeof d);
    LIB(babe_model_eval_desc(model, state, &d.eval), "babe_model_eval_desc");
    const int K = d.eval.K;                       /* (a host overrides d.eval.xi, d.eval.fit, ... here) */
    /* a known degradation instead of the blind filter fit: the observation model goes into the descriptor */
    if (fir_n && observe_fir(&d.eval, fir_n, fir_fc, fir_width, info.fs, &taps) != 0) goto done;
    if (declip >= 0) d.eval.obs_kind = BABE_OBS_CLIP, d.eval.clip_value = (float)declip, d.eval.blind = 0;

    /* 4. the schedule: one row per step, from the file's tester.diff_params */
    if (T == 0) T = (int)setting(model, "tester.T", 35);
    if (T < 2) FAIL("--T must be at least 2");
    steps = (babe_sample_step*)calloc((size_t)T, sizeof *steps);
    if (!steps) FAIL("out of memory");
    double start_sigma = setting(model, "tester.posterior_sampling.start_sigma", -1.0);      /* "None" in the file: a cold start */
    LIB(babe_edm_steps(steps, &d.t0, T, (int)setting(model, "tester.order", 2), setting(model, "tester.diff_params.sigma_min", 1e-4),
                       setting(model, "tester.diff_params.sigma_max", 1.0), setting(model, "tester.diff_params.ro", 8.0),
                       setting(model, "tester.diff_params.sigma_data", 0.063), setting(model, "tester.diff_params.Schurn", 10.0),
                       setting(model, "tester.diff_params.Stmin", 0.0), setting(model, "tester.diff_params.Stmax", 50.0),
                       known ? setting(model, "tester.diff_params.Snoise", 1.0) : 1.0 /* the blind loop injects with Snoise = 1 */, start_sigma),
        "babe_edm_steps");
    d.T = T, d.steps = steps, d.warm_start = start_sigma > 0;

    /* 5. the workspace is the caller's, 6. like every other buffer */
    const long ws_bytes = babe_sample_workspace_bytes(&d, B);
    if (ws_bytes < 0) FAIL("babe_sample_workspace_bytes: %s", babe_last_error());
    HIP(hipMalloc(&ws, (size_t)ws_bytes), "hipMalloc(workspace)");
    HIP(hipMalloc((void**)&y, (size_t)B * L * sizeof(float)), "hipMalloc(y)");
    HIP(hipMalloc((void**)&x, (size_t)B * L * sizeof(float)), "hipMalloc(x)");
    HIP(hipMalloc((void**)&params, (size_t)B * 2 * K * sizeof(float)), "hipMalloc(params)");
    host = (float*)malloc((size_t)B * L * sizeof(float));
    host_params = (float*)malloc((size_t)B * 2 * K * sizeof(float));
    if (!host || !host_params) FAIL("out of memory");
    fh = fopen(argv[2], "rb");
    if (!fh) FAIL("cannot open %s", argv[2]);
    if (fread(host, sizeof(float), (size_t)B * L, fh) != (size_t)B * L) FAIL("%s: fewer than %d x %ld float32 samples", argv[2], B, L);
    fclose(fh), fh = NULL;
    HIP(hipMemcpy(y, host, (size_t)B * L * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(y)");
    for (int b = 0; b < B; ++b)                  /* the initial filter of every clip: tester.blind_bwe.initial_conditions */
        for (int k = 0; k < K; ++k) {
            char key[64];
            snprintf(key, sizeof key, "tester.blind_bwe.initial_conditions.fc.%d", k);
            host_params[(b * 2 + 0) * K + k] = (float)setting(model, key, 0);
            snprintf(key, sizeof key, "tester.blind_bwe.initial_conditions.A.%d", k);
            host_params[(b * 2 + 1) * K + k] = (float)setting(model, key, 0);
        }
    HIP(hipMemcpy(params, host_params, (size_t)B * 2 * K * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(params)");

    /* 7. the whole run: T steps of score evaluations, noise from the library's generator under `seed` */
    LIB(babe_sample_bwe(&d, y, params, x, NULL, seed, 0, NULL, NULL, ws, ws_bytes, B, NULL), "babe_sample_bwe");
    HIP(hipDeviceSynchronize(), "hipDeviceSynchronize");
    HIP(hipMemcpy(host, x, (size_t)B * L * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(x)");
    HIP(hipMemcpy(host_params, params, (size_t)B * 2 * K * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(params)");
    /* [/core] */

    fh = fopen(argv[3], "wb");
    if (!fh || fwrite(host, sizeof(float), (size_t)B * L, fh) != (size_t)B * L) FAIL("cannot write %s", argv[3]);
    fclose(fh), fh = NULL;
    if (params_path) {
        fh = fopen(params_path, "wb");
        if (!fh || fwrite(host_params, sizeof(float), (size_t)B * 2 * K, fh) != (size_t)B * 2 * K) FAIL("cannot write %s", params_path);
        fclose(fh), fh = NULL;
    }
    status = 0;
done:
    if (fh) fclose(fh);
    free(host), free(host_params), free(steps);
    if (ws) (void)hipFree(ws);
    if (y) (void)hipFree(y);
    if (x) (void)hipFree(x);
    if (params) (void)hipFree(params);
    if (taps) (void)hipFree(taps);
    if (state) babe_unet_state_destroy(state);
    if (model) babe_model_destroy(model);          /* last: the descriptor points into its arena */
    return status;
}
