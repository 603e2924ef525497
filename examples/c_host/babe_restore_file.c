/* babe_restore_file: blind bandwidth extension of a recording FILE at any sample rate from C, with the denoiser pre-pass - no
 * Python, no torch in the process.
 *
 *     babe_restore_file model.babe in.f32 RATE out.f32 [--denoiser denoiser.babe] [--seed N] [--T n] [--blind-segments N]
 *                       [--ix-start s] [--precision f32|bf16|bf16x3]
 *                       [--attention f32|bf16]
 *
 * model.babe: written by `python -m babe_amd.export`; denoiser.babe: by `python -m babe_amd.export_denoiser`.  in.f32: the
 * recording, float32 samples of any length at RATE Hz.  out.f32: the restored recording at the MODEL's rate.  The file is
 * converted to the denoiser's rate, denoised, converted to the model's rate (without --denoiser: converted to the model's rate),
 * then restored as babe_restore_recording does it.  The low-pass filter of the recording is estimated blind on
 * --blind-segments segments (default 1: the one that starts --ix-start seconds into the file, default 0; more: evenly spread
 * over the file), then the file is restored segment by segment, every segment out-painted from the end of the previous one.
 * The estimated filter is printed: K cut-off frequencies in Hz, then K slopes in dB.  --T: sampling steps (default: the file's
 * tester.T); --seed: the noise is the library's counter-based generator under this seed (default 0), so the output is a
 * function of (model, input, seed, T, blind segments).  --attention: the core a model with time-attention layers runs them
 * on (without it such a file is refused).  Links against libbabe_hip.so and the HIP runtime
 * (babe_amd/build.py::build_example).  Exit status: 0, or 1 with the failing step and babe_last_error() on stderr. */
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "babe_hip.h"

#define FAIL(...) do { fprintf(stderr, "babe_restore_file: " __VA_ARGS__); fprintf(stderr, "\n"); goto done; } while (0)
#define LIB(call, what) do { if ((call) != 0) FAIL("%s: %s", what, babe_last_error()); } while (0)
#define HIP(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) FAIL("%s: %s", what, hipGetErrorString(e_)); } while (0)

#define DC_SIZE 50          /* predict_bwe_AR smooths the edge of its mask over 50 samples */
#define DISCARD_END 200     /* samples at the end of a restored segment that are not kept */

static int precision_of(const char* s) {
    return !strcmp(s, "f32") ? BABE_PRECISION_F32 : !strcmp(s, "bf16") ? BABE_PRECISION_BF16 : !strcmp(s, "bf16x3") ? BABE_PRECISION_BF16X3 : -1;
}

static int attention_of(const char* s) { return !strcmp(s, "f32") ? BABE_ATTENTION_F32 : !strcmp(s, "bf16") ? BABE_ATTENTION_BF16 : -1; }

static double setting(const void* model, const char* key, double fallback) {
    double v;
    return babe_model_setting(model, key, &v) == 0 ? v : fallback;
}

int main(int argc, char** argv) {
    int status = 1, T = 0, n_blind = 1, precision = BABE_PRECISION_F32, attention = BABE_ATTENTION_REFUSE;
    long seed = 0, Lfile = 0, Lrec = 0, fs_file = 0;
    double ix_start = 0.0;
    const char* denoiser_path = NULL;
    void *model = NULL, *denoiser = NULL, *state = NULL, *ws = NULL;
    float *rec = NULL, *out = NULL, *filter = NULL, *init = NULL, *window = NULL, *host = NULL, *host_kernel = NULL;
    float* dev_kernel[2] = {NULL, NULL};
    int *dev_krange[2] = {NULL, NULL}, *host_krange = NULL;
    babe_sample_step* steps = NULL;
    FILE* fh = NULL;
    if (argc < 5) {
        fprintf(stderr, "usage: babe_restore_file model.babe in.f32 RATE out.f32 [--denoiser denoiser.babe] [--seed N] [--T n] "
                        "[--blind-segments N] [--ix-start s] [--precision f32|bf16|bf16x3] [--attention f32|bf16]\n");
        return 2;
    }
    fs_file = atol(argv[3]);
    if (fs_file < 1) FAIL("RATE must be a positive number of samples per second");
    for (int i = 5; i < argc; ++i) {
        if (i + 1 >= argc) FAIL("option %s needs a value", argv[i]);
        if (!strcmp(argv[i], "--seed")) seed = atol(argv[++i]);
        else if (!strcmp(argv[i], "--denoiser")) denoiser_path = argv[++i];
        else if (!strcmp(argv[i], "--T")) T = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--blind-segments")) n_blind = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--ix-start")) ix_start = atof(argv[++i]);
        else if (!strcmp(argv[i], "--precision")) {
            if ((precision = precision_of(argv[++i])) < 0) FAIL("--precision is one of f32, bf16, bf16x3");
        }
        else if (!strcmp(argv[i], "--attention")) {
            if ((attention = attention_of(argv[++i])) < 0) FAIL("--attention is one of f32, bf16");
        }
        else FAIL("unknown option %s", argv[i]);
    }
    if (n_blind < 1 || n_blind > 16) FAIL("--blind-segments must be 1..16");

    /* the recording */
    fh = fopen(argv[2], "rb");
    if (!fh) FAIL("cannot open %s", argv[2]);
    if (fseek(fh, 0, SEEK_END) != 0 || (Lfile = ftell(fh) / (long)sizeof(float)) < 2) FAIL("%s: fewer than 2 float32 samples", argv[2]);
    rewind(fh);
    host = (float*)malloc((size_t)Lfile * sizeof(float));
    if (!host) FAIL("out of memory");
    if (fread(host, sizeof(float), (size_t)Lfile, fh) != (size_t)Lfile) FAIL("cannot read %s", argv[2]);
    fclose(fh), fh = NULL;

    /* [core] the listing of INTEGRATION.md, "A recording file at any rate, with the denoiser" */
    /* 1. the network, the denoiser and one evaluation's bookkeeping */
    const babe_model_options options = {precision, attention, {0}};      /* attention: REFUSE unless --attention chose a core */
    model = babe_model_load_opt(argv[1], &options, NULL);
    if (!model) FAIL("babe_model_load_opt: %s", babe_last_error());
    if (denoiser_path && !(denoiser = babe_denoiser_load(denoiser_path, NULL))) FAIL("babe_denoiser_load: %s", babe_last_error());
    state = babe_unet_state_create();
    if (!state) FAIL("babe_unet_state_create failed");
    babe_file_desc fd;
    memset(&fd, 0, sizeof fd);
    babe_recording_desc* const d = &fd.rec;         /* the recording part: as in babe_restore_recording.c */
    LIB(babe_model_eval_desc(model, state, &d->eval), "babe_model_eval_desc");
    const int K = d->eval.K;
    const long segL = d->eval.L;

    /* 1b. the rate plan, and one sinc table per conversion that runs: built on the host, the caller's on the device */
    babe_denoiser_summary dn;
    memset(&dn, 0, sizeof dn);
    if (denoiser) LIB(babe_denoiser_info(denoiser, &dn), "babe_denoiser_info");
    const long fs_model = (long)d->eval.fs;
    const int convs = babe_restore_file_plan(Lfile, fs_file, dn.sample_rate, fs_model, fd.lengths);
    if (convs < 0) FAIL("babe_restore_file_plan: %s", babe_last_error());
    const long from[2] = {fs_file, dn.sample_rate}, to[2] = {denoiser ? dn.sample_rate : fs_model, fs_model};
    for (int k = 0; k < 2; ++k) {
        if (!(convs >> k & 1)) continue;
        babe_sinc_table* t = &fd.conv[k];
        const long n = babe_resample_sinc_table_size(from[k], to[k], &t->width, &t->orig, &t->new_);
        if (n < 0) FAIL("babe_resample_sinc_table_size: %s", babe_last_error());
        host_kernel = (float*)realloc(host_kernel, (size_t)n * sizeof(float));
        host_krange = (int*)realloc(host_krange, (size_t)2 * t->new_ * sizeof(int));
        if (!host_kernel || !host_krange) FAIL("out of memory");
        LIB(babe_resample_sinc_table(from[k], to[k], host_kernel, host_krange), "babe_resample_sinc_table");
        HIP(hipMalloc((void**)&dev_kernel[k], (size_t)n * sizeof(float)), "hipMalloc(kernel)");
        HIP(hipMalloc((void**)&dev_krange[k], (size_t)2 * t->new_ * sizeof(int)), "hipMalloc(krange)");
        HIP(hipMemcpy(dev_kernel[k], host_kernel, (size_t)n * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(kernel)");
        HIP(hipMemcpy(dev_krange[k], host_krange, (size_t)2 * t->new_ * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy(krange)");
        t->kernel = dev_kernel[k], t->krange = dev_krange[k];
    }
    fd.denoiser = denoiser;
    Lrec = fd.lengths[2];                         /* samples at the model's rate: what the blind segments refer to */

    /* 2. two step tables over one schedule: the blind loop injects with Snoise = 1, the known-filter loops with the tester's */
    if (T == 0) T = (int)setting(model, "tester.T", 35);
    if (T < 2) FAIL("--T must be at least 2");
    steps = (babe_sample_step*)calloc((size_t)2 * T, sizeof *steps);
    if (!steps) FAIL("out of memory");
    const double start_sigma = setting(model, "tester.posterior_sampling.start_sigma", -1.0);
    const double snoise[2] = {1.0, setting(model, "tester.diff_params.Snoise", 1.0)};
    for (int k = 0; k < 2; ++k)
        LIB(babe_edm_steps(steps + k * T, &d->t0, T, (int)setting(model, "tester.order", 2), setting(model, "tester.diff_params.sigma_min", 1e-4),
                           setting(model, "tester.diff_params.sigma_max", 1.0), setting(model, "tester.diff_params.ro", 8.0),
                           setting(model, "tester.diff_params.sigma_data", 0.063), setting(model, "tester.diff_params.Schurn", 10.0),
                           setting(model, "tester.diff_params.Stmin", 0.0), setting(model, "tester.diff_params.Stmax", 50.0), snoise[k],
                           start_sigma),
            "babe_edm_steps");
    d->T = T, d->steps_blind = steps, d->steps_known = steps + T, d->warm_start = start_sigma > 0;

    /* 3. the policy is the host's: where the blind segments start, how loud the model hears the file, how far segments overlap */
    d->n_blind = Lrec > segL ? n_blind : 1;
    for (int j = 0; j < d->n_blind; ++j)
        d->blind_starts[j] = Lrec <= segL ? 0 : d->n_blind == 1 ? (long)(ix_start * d->eval.fs) : (long)((double)j * (Lrec - segL) / (d->n_blind - 1));
    d->target_std = (float)setting(model, "tester.complete_recording.std", 0.1);
    d->overlap = (long)(0.25 * d->eval.fs), d->discard_end = DISCARD_END;
    d->inpaint_dc = (int)setting(model, "tester.complete_recording.inpaint_DC", 1), d->dc_size = DC_SIZE;
    d->std_dev = NULL;                             /* the call measures the file */

    /* 4. tables come from the caller: the initial filter and the periodic Hann window the mask's edge is smoothed with */
    float host_init[2 * 8], host_window[2 * DC_SIZE];
    for (int k = 0; k < K; ++k) {
        char key[64];
        snprintf(key, sizeof key, "tester.blind_bwe.initial_conditions.fc.%d", k);
        host_init[k] = (float)setting(model, key, 0);
        snprintf(key, sizeof key, "tester.blind_bwe.initial_conditions.A.%d", k);
        host_init[K + k] = (float)setting(model, key, 0);
    }
    for (int k = 0; k < 2 * DC_SIZE; ++k) host_window[k] = (float)(0.5 - 0.5 * cos(2.0 * 3.14159265358979323846 * k / (2 * DC_SIZE)));
    HIP(hipMalloc((void**)&init, sizeof host_init), "hipMalloc(init)");
    HIP(hipMalloc((void**)&window, sizeof host_window), "hipMalloc(window)");
    HIP(hipMemcpy(init, host_init, sizeof host_init, hipMemcpyHostToDevice), "hipMemcpy(init)");
    HIP(hipMemcpy(window, host_window, sizeof host_window, hipMemcpyHostToDevice), "hipMemcpy(window)");
    d->init_params = init, d->dc_window = window;

    /* 5. the workspace holds the converted signals too; 6. the file and the result are the caller's buffers */
    const long ws_bytes = babe_restore_file_workspace_bytes(&fd);
    if (ws_bytes < 0) FAIL("babe_restore_file_workspace_bytes: %s", babe_last_error());
    HIP(hipMalloc(&ws, (size_t)ws_bytes), "hipMalloc(workspace)");
    HIP(hipMalloc((void**)&rec, (size_t)Lfile * sizeof(float)), "hipMalloc(rec)");
    HIP(hipMalloc((void**)&out, (size_t)Lrec * sizeof(float)), "hipMalloc(out)");
    HIP(hipMalloc((void**)&filter, (size_t)2 * K * sizeof(float)), "hipMalloc(filter)");
    HIP(hipMemcpy(rec, host, (size_t)Lfile * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(rec)");

    /* 7. the whole file: conversions, denoiser, blind estimate, the autoregressive walk, enqueued by one call */
    LIB(babe_restore_file(&fd, rec, Lfile, out, filter, NULL, NULL, seed, 0, ws, ws_bytes, NULL), "babe_restore_file");
    HIP(hipDeviceSynchronize(), "hipDeviceSynchronize");
    if (Lrec > Lfile && !(host = (float*)realloc(host, (size_t)Lrec * sizeof(float)))) FAIL("out of memory");
    HIP(hipMemcpy(host, out, (size_t)Lrec * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(out)");
    HIP(hipMemcpy(host_init, filter, (size_t)2 * K * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(filter)");
    /* [/core] */

    printf("fc_Hz");
    for (int k = 0; k < K; ++k) printf(" %.9g", host_init[k]);
    printf("\nA_dB");
    for (int k = 0; k < K; ++k) printf(" %.9g", host_init[K + k]);
    printf("\n");
    fh = fopen(argv[4], "wb");
    if (!fh || fwrite(host, sizeof(float), (size_t)Lrec, fh) != (size_t)Lrec) FAIL("cannot write %s", argv[4]);
    fclose(fh), fh = NULL;
    status = 0;
done:
    if (fh) fclose(fh);
    free(host), free(steps), free(host_kernel), free(host_krange);
    for (int k = 0; k < 2; ++k) {
        if (dev_kernel[k]) (void)hipFree(dev_kernel[k]);
        if (dev_krange[k]) (void)hipFree(dev_krange[k]);
    }
    if (ws) (void)hipFree(ws);
    if (rec) (void)hipFree(rec);
    if (out) (void)hipFree(out);
    if (filter) (void)hipFree(filter);
    if (init) (void)hipFree(init);
    if (window) (void)hipFree(window);
    if (state) babe_unet_state_destroy(state);
    if (denoiser) babe_denoiser_destroy(denoiser);
    if (model) babe_model_destroy(model);          /* last: the descriptor points into its arena */
    return status;
}
