// A WHOLE RECORDING from plan handles - the flow long_file.restore_recording_complete (without denoiser and rate conversion) and
// restore_file_AR sequence from Python (babe_amd/testing/long_file.py; BlindTester.test_real_blind_bwe_complete,
// testing/blind_bwe_tester.py:710-867), as ONE C-ABI call for a non-Python host:
//   normalise the file to target_std -> blind filter estimate on n_blind segments in one coupled batch (babe_sample_bwe, blind = 1,
//   shared = 1) -> first segment with that filter -> every following segment out-painted from the tail of the previous result
//   (the observation model of predict_bwe_AR: babe_sample_bwe with eval.mask / eval.dc_mask) -> undo the normalisation.
// Scope: the STFT filter the flow estimates itself (eval.obs_kind = BABE_OBS_STFT, no classic replacement step); the known
// degradations babe_score_eval sequences besides are refused here, before the first device call.
// The file is never copied: every segment is cut from it and normalised on the way (element-wise, so the same bits as normalising
// the file first), and the restored pieces are written straight into `out`, which is scaled back in place at the end.  The scale
// factors stay on the device.  The quirks of the Python flow are kept: a last segment longer than segL is truncated, and the last
// segment's known head is the tail of the last PREDICTION, not of what was kept of it (:842).
// Nothing allocates, nothing synchronises, nothing is copied from or to the host; all of it is enqueued on the caller's stream.
#include <cmath>
#include "common.h"
#include "eval_geom.h"
#include "workspace.h"

namespace {

constexpr int STD_BLK = 64;            // slices of a row, one workgroup each: part[b] = STD_BLK sums, then STD_BLK sums of squares

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// part[b][blk] = sum of (x - x[0]), part[b][STD_BLK + blk] = sum of (x - x[0])^2 over slice blk of row b, in double.  The slices
// are whole float4 after the row's first 16-byte boundary (workgroup 0 also takes the scalars before it and after the last whole
// float4); every thread walks its slice front to back and the workgroup sum has one order (block_sum).
__global__ __launch_bounds__(256) void row_std_partial_kernel(const float* __restrict__ x, long x_bs, long n, double* __restrict__ part) {
    __shared__ double sh[4];
    const int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const float* row = x + (long)b * x_bs;
    const double shift = (double)row[0];
    long head = (4 - (long)((reinterpret_cast<uintptr_t>(row) >> 2) & 3)) & 3;
    if (head > n) head = n;
    const long nv = (n - head) / 4, per = (nv + STD_BLK - 1) / STD_BLK;
    const long v0 = (long)blk * per, v1 = v0 + per < nv ? v0 + per : nv;
    const float4* rv = reinterpret_cast<const float4*>(row + head);
    double s = 0.0, ss = 0.0;
    auto acc = [&](float f) {
        const double v = (double)f - shift;
        s += v;
        ss += v * v;
    };
    for (long q = v0 + tid; q < v1; q += 256) {
        const float4 f = rv[q];
        acc(f.x), acc(f.y), acc(f.z), acc(f.w);
    }
    if (blk == 0) {
        if (tid < head) acc(row[tid]);
        const long i = head + 4 * nv + tid;
        if (tid < 4 && i < n) acc(row[i]);
    }
    s = block_sum<4>(s, sh);
    __syncthreads();
    ss = block_sum<4>(ss, sh);
    if (tid == 0) {
        part[(long)b * 2 * STD_BLK + blk] = s;
        part[(long)b * 2 * STD_BLK + STD_BLK + blk] = ss;
    }
}

// out[b] = sqrt((SS - S^2 / n) / (n - 1)) rounded once to float: one wave per row, the slice sums added in wave_sum's order
__global__ __launch_bounds__(64) void row_std_final_kernel(const double* __restrict__ part, long n, float* __restrict__ out) {
    const int b = blockIdx.x;
    const double S = wave_sum(part[(long)b * 2 * STD_BLK + threadIdx.x]);
    const double SS = wave_sum(part[(long)b * 2 * STD_BLK + STD_BLK + threadIdx.x]);
    if (threadIdx.x == 0) {
        const double var = (SS - S * S / (double)n) / (double)(n - 1);
        out[b] = (float)sqrt(var > 0.0 ? var : 0.0);
    }
}

// dst[i] = i < n ? src[i] : 0 for i in [0, len)
__global__ __launch_bounds__(256) void cut_kernel(const float* __restrict__ src, long n, float* __restrict__ dst, long len) {
    const long step = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (aligned16(src) && aligned16(dst)) {
        const long lv = len / 4;
        for (long q = t0; q < lv; q += step) {
            const long i = 4 * q;
            float4 f;
            if (i + 3 < n) f = reinterpret_cast<const float4*>(src)[q];
            else f = make_float4(i < n ? src[i] : 0.f, i + 1 < n ? src[i + 1] : 0.f, i + 2 < n ? src[i + 2] : 0.f, 0.f);
            reinterpret_cast<float4*>(dst)[q] = f;
        }
        for (long i = 4 * lv + t0; i < len; i += step) dst[i] = i < n ? src[i] : 0.f;
    } else {
        for (long i = t0; i < len; i += step) dst[i] = i < n ? src[i] : 0.f;
    }
}

// mode 0: out = (a x) / s[0] (two roundings, the normalisation);  mode 1: out = x (s[0] a) (a = the rounded 1 / target_std)
__device__ __forceinline__ float scale1(float x, float a, float s, float f, int mode) { return mode == 0 ? (a * x) / s : x * f; }
// (out may be x: element i is read before it is written, by the same thread)
__global__ __launch_bounds__(256) void scale_dev_kernel(float* out, const float* x, long n, float a, const float* __restrict__ s_dev,
                                                        int mode) {
    const float s = s_dev[0], f = s * a;
    const long step = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long done = 0;
    if (aligned16(out) && aligned16(x)) {
        const long nv = n / 4;
        for (long q = t0; q < nv; q += step) {
            const float4 v = reinterpret_cast<const float4*>(x)[q];
            reinterpret_cast<float4*>(out)[q] = make_float4(scale1(v.x, a, s, f, mode), scale1(v.y, a, s, f, mode), scale1(v.z, a, s, f, mode),
                                                            scale1(v.w, a, s, f, mode));
        }
        done = 4 * nv;
    }
    for (long i = done + t0; i < n; i += step) out[i] = scale1(x[i], a, s, f, mode);
}

// the mask pair of an edge at sample e: mask = i < e; smooth = 1 before e - size, window[size + (i - (e - size))] - the falling
// half of the 2 size table - on [e - size, e), 0 from e on (prepare_smooth_mask on that mask, blind_bwe_sampler.py:232-257);
// smooth may be NULL: the hard mask alone
__device__ __forceinline__ float smooth_at(long i, long e, int size, const float* __restrict__ window) {
    return i < e - size ? 1.f : (i < e ? window[size + (i - (e - size))] : 0.f);
}
__global__ __launch_bounds__(256) void edge_masks_kernel(float* __restrict__ mask, float* __restrict__ smooth, long L, long e, int size,
                                                         const float* __restrict__ window) {
    const long step = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long done = 0;
    if (aligned16(mask) && aligned16(smooth)) {
        const long lv = L / 4;
        for (long q = t0; q < lv; q += step) {
            const long i = 4 * q;
            reinterpret_cast<float4*>(mask)[q] = make_float4(i < e ? 1.f : 0.f, i + 1 < e ? 1.f : 0.f, i + 2 < e ? 1.f : 0.f, i + 3 < e ? 1.f : 0.f);
            if (smooth)
                reinterpret_cast<float4*>(smooth)[q] = make_float4(smooth_at(i, e, size, window), smooth_at(i + 1, e, size, window),
                                                                   smooth_at(i + 2, e, size, window), smooth_at(i + 3, e, size, window));
        }
        done = 4 * lv;
    }
    for (long i = done + t0; i < L; i += step) {
        mask[i] = i < e ? 1.f : 0.f;
        if (smooth) smooth[i] = smooth_at(i, e, size, window);
    }
}

int grid_for(long n) {
    const int g = cdiv(n, 1024);
    return g < 1 ? 1 : (g > 2048 ? 2048 : g);
}

// ---- the walk of restore_file_AR: segment j starts at j * hop, hop = segL - overlap - discard_end; the last segment is the first
// whose start is not below L - segL - discard_end.  A file of at most segL samples is one (zero-padded) segment.
long seg_count(long L, long segL, long overlap, long discard_end) {
    if (L <= segL) return 1;
    const long hop = segL - overlap - discard_end;
    long j = 1;
    while (j * hop < L - segL - discard_end) ++j;
    return j + 1;
}
// samples of segment j that exist in the file (the last one truncated to segL where the walk leaves it longer)
long seg_valid(long j, long count, long L, long segL, long hop) {
    if (count == 1) return L;
    if (j < count - 1) return segL;
    const long n = L - j * hop;
    return n > segL ? segL : n;
}

bool walk_ok(long Lrec, long segL, long overlap, long discard_end) {
    return Lrec >= 1 && segL >= 1 && discard_end >= 0 && overlap >= 1 && overlap < segL - discard_end;
}

// every buffer of one call.  The two kinds of run (the blind batch, one known-filter segment) come one after the other and
// share one block of the larger size.
struct RecWork {
    void* run;
    float *std, *yb, *blind_pred, *filter, *seg, *yobs, *mask, *smooth, *y_masked, *dc_y, *pred;
    double* part;
};
void carve(Carver& c, const babe_recording_desc* d, long run_bytes, RecWork& w) {
    const size_t L = (size_t)d->eval.L;
    w.run = c.take<char>((size_t)run_bytes);
    w.part = c.take<double>(2 * STD_BLK);
    w.std = c.take<float>(1);
    w.yb = c.take<float>((size_t)d->n_blind * L), w.blind_pred = c.take<float>((size_t)d->n_blind * L);
    w.filter = c.take<float>(2 * (size_t)d->eval.K);
    for (float** p : {&w.seg, &w.yobs, &w.mask, &w.smooth, &w.y_masked, &w.dc_y, &w.pred}) *p = c.take<float>(L);
}

// the descriptor's own fields, checked before anything else (host only; who: the entry point's name)
int desc_check(const babe_recording_desc* d, const char* who) {
    BABE_CHECK_ARG(d, "%s: NULL descriptor", who);
    BABE_CHECK_ARG(d->steps_blind && d->steps_known, "%s: NULL steps_blind or steps_known", who);
    BABE_CHECK_ARG(d->init_params, "%s: NULL init_params", who);
    BABE_CHECK_ARG(d->n_blind >= 1 && d->n_blind <= 16, "%s: n_blind = %d outside 1..16", who, d->n_blind);
    BABE_CHECK_ARG(d->T >= 1, "%s: T = %d steps", who, d->T);
    BABE_CHECK_ARG(d->eval.K >= 1 && d->eval.K <= 8, "%s: eval.K = %d", who, d->eval.K);
    BABE_CHECK_ARG(d->target_std > 0.f && std::isfinite(d->target_std), "%s: target_std = %g", who, d->target_std);
    BABE_CHECK_ARG(d->discard_end >= 0, "%s: discard_end = %ld", who, d->discard_end);
    BABE_CHECK_ARG(d->inpaint_dc == 0 || (d->dc_size >= 1 && d->dc_window), "%s: inpaint_dc with dc_size = %d or a NULL dc_window", who,
                   d->dc_size);
    BABE_CHECK_ARG(d->overlap >= 1 && d->overlap > d->dc_size, "%s: overlap = %ld must exceed dc_size = %d", who, d->overlap, d->dc_size);
    BABE_CHECK_ARG(d->overlap < d->eval.L - d->discard_end, "%s: overlap = %ld must be below L - discard_end = %ld", who, d->overlap,
                   d->eval.L - d->discard_end);
    BABE_CHECK_ARG(!d->eval.mask && !d->eval.dc_mask && !d->eval.dc_y, "%s: eval.mask / dc_mask / dc_y are the call's to set", who);
    BABE_CHECK_ARG(d->eval.obs_kind == BABE_OBS_STFT && !d->eval.dc_classic, "%s: eval.obs_kind = %d, dc_classic = %d: a recording is "
                   "restored against the STFT filter it estimates (BABE_OBS_STFT, no classic replacement step)", who, d->eval.obs_kind,
                   d->eval.dc_classic);
    return BABE_OK;
}

// the two runs' descriptors and the larger of their workspace sizes (-1: a size query failed, its message stands)
long run_descs(const babe_recording_desc* d, babe_sample_desc& blind, babe_sample_desc& known) {
    blind.eval = d->eval, blind.T = d->T, blind.steps = d->steps_blind, blind.t0 = d->t0, blind.warm_start = d->warm_start;
    blind.skip_zero_inject = 0;
    blind.eval.blind = 1, blind.eval.shared = 1;
    known = blind;
    known.steps = d->steps_known;
    known.eval.blind = 0, known.eval.shared = d->eval.shared;
    const long a = babe_sample_workspace_bytes(&blind, d->n_blind), b = babe_sample_workspace_bytes(&known, 1);
    return (a < 0 || b < 0) ? -1 : (a > b ? a : b);
}

}  // namespace

extern "C" int babe_row_std(const float* x, long x_bs, int B, long n, float* out, double* part, void* stream) {
    BABE_CHECK_ARG(x && out && part && B >= 1 && B <= 65535, "row_std: bad arguments");
    BABE_CHECK_ARG(n >= 2, "row_std: n = %ld (the unbiased estimate needs two samples)", n);
    hipLaunchKernelGGL(row_std_partial_kernel, dim3(STD_BLK, B), dim3(256), 0, (hipStream_t)stream, x, x_bs, n, part);
    BABE_LAUNCH_CHECK();
    hipLaunchKernelGGL(row_std_final_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, part, n, out);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" int babe_segment_cut(const float* src, long n, float* dst, long len, void* stream) {
    BABE_CHECK_ARG(src && dst && n >= 0 && len >= 1 && n <= len, "segment_cut: n = %ld, len = %ld", n, len);
    hipLaunchKernelGGL(cut_kernel, dim3(grid_for(len)), dim3(256), 0, (hipStream_t)stream, src, n, dst, len);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" int babe_scale_dev(float* out, const float* x, long n, float a, const float* s_dev, int mode, void* stream) {
    BABE_CHECK_ARG(out && x && s_dev && n >= 1 && (mode == 0 || mode == 1), "scale_dev: bad arguments");
    hipLaunchKernelGGL(scale_dev_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, out, x, n, a, s_dev, mode);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" int babe_edge_masks(float* mask, float* smooth, long L, long e, int size, const float* window, void* stream) {
    BABE_CHECK_ARG(mask && L >= 1 && (!smooth || (window && size >= 1)), "edge_masks: bad arguments");
    if (!smooth) size = 0;
    BABE_CHECK_ARG(e >= size && e <= L, "edge_masks: edge e = %ld outside [size = %d, L = %ld]", e, size, L);
    hipLaunchKernelGGL(edge_masks_kernel, dim3(grid_for(L)), dim3(256), 0, (hipStream_t)stream, mask, smooth, L, e, size, window);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" long babe_recording_plan(long Lrec, long segL, long overlap, long discard_end, long* starts, long* n_valid, long max_segments) {
    if (!walk_ok(Lrec, segL, overlap, discard_end) || max_segments < 0) {
        babe_set_error("recording_plan: Lrec = %ld, segL = %ld, overlap = %ld, discard_end = %ld (1 <= overlap < segL - discard_end)", Lrec,
                       segL, overlap, discard_end);
        return -1;
    }
    const long count = seg_count(Lrec, segL, overlap, discard_end), hop = segL - overlap - discard_end;
    for (long j = 0; j < count && j < max_segments; ++j) {
        if (starts) starts[j] = j * hop;
        if (n_valid) n_valid[j] = seg_valid(j, count, Lrec, segL, hop);
    }
    return count;
}

extern "C" long babe_recording_workspace_bytes(const babe_recording_desc* d) {
    if (desc_check(d, "recording_workspace_bytes") != BABE_OK) return -1;
    babe_sample_desc blind, known;
    const long run = run_descs(d, blind, known);
    if (run < 0) return -1;
    Carver dry{nullptr, 0, 256};
    RecWork w;
    carve(dry, d, run, w);
    return (long)dry.used;
}

extern "C" int babe_restore_recording(const babe_recording_desc* d, const float* rec, long Lrec, float* out, float* filter_out,
                                      float* blind_pred, long seed, long clip0, void* ws, long ws_bytes, void* stream) {
    // ---- host-side validation, all of it before the first device call
    BABE_TRY(desc_check(d, "restore_recording"));
    BABE_CHECK_ARG(rec && out && ws, "restore_recording: NULL rec, out or ws");
    BABE_CHECK_ARG(Lrec >= 2, "restore_recording: Lrec = %ld", Lrec);
    const long segL = d->eval.L, overlap = d->overlap, hop = segL - overlap - d->discard_end;
    for (int j = 0; j < d->n_blind; ++j)
        BABE_CHECK_ARG(d->blind_starts[j] >= 0 && d->blind_starts[j] <= (Lrec > segL ? Lrec - segL : 0),
                       "restore_recording: blind_starts[%d] = %ld past Lrec - segL = %ld", j, d->blind_starts[j], Lrec - segL);
    const long count = seg_count(Lrec, segL, overlap, d->discard_end);
    BABE_CHECK_ARG(clip0 >= 0 && clip0 + d->n_blind + count <= 0x100000000L, "restore_recording: clip0 = %ld outside the counter word", clip0);
    babe_sample_desc blind, known;
    const long run = run_descs(d, blind, known);
    if (run < 0) return BABE_ERR_ARG;
    BABE_TRY(eval_desc_check(&blind.eval, "restore_recording"));          // (what the runs would refuse, refused here: nothing is
    BABE_TRY(sample_steps_check(d->steps_blind, d->T, d->t0, "restore_recording: steps_blind"));     // enqueued before them)
    BABE_TRY(sample_steps_check(d->steps_known, d->T, d->t0, "restore_recording: steps_known"));
    Carver c{static_cast<char*>(ws), ws_bytes > 0 ? (size_t)ws_bytes : 0, 256};
    RecWork w;
    carve(c, d, run, w);
    BABE_CHECK_ARG(c.ok, "restore_recording: workspace of %ld bytes, need %ld", ws_bytes, (long)c.used);
    hipStream_t st = (hipStream_t)stream;
#define RT(call)                                                                                   \
    do {                                                                                           \
        const hipError_t e__ = (call);                                                             \
        if (e__ != hipSuccess) {                                                                   \
            babe_set_error("%s:%d %s: %s", __FILE__, __LINE__, #call, hipGetErrorString(e__));     \
            return BABE_ERR_HIP;                                                                   \
        }                                                                                          \
    } while (0)
    const int K = d->eval.K, nb = d->n_blind;
    float* const filter = filter_out ? filter_out : w.filter;
    float* const bpred = blind_pred ? blind_pred : w.blind_pred;
    const float inv_target = 1.f / d->target_std;
    // ---- the file's standard deviation (the caller's, or computed here); (target_std x) / s is applied to every cut
    const float* s_dev = d->std_dev;
    if (!s_dev) {
        BABE_TRY(babe_row_std(rec, Lrec, 1, Lrec, w.std, w.part, stream));
        s_dev = w.std;
    }
    auto cut_norm = [&](long ix, long n, float* dst) -> int {
        BABE_TRY(babe_segment_cut(rec + ix, n, dst, segL, stream));
        return babe_scale_dev(dst, dst, segL, d->target_std, s_dev, 0, stream);
    };
    // ---- blind step: the filter of the whole recording, fitted on n_blind segments as one coupled batch
    for (int j = 0; j < nb; ++j) {
        const long ix = d->blind_starts[j];
        BABE_TRY(cut_norm(ix, Lrec - ix < segL ? Lrec - ix : segL, w.yb + (long)j * segL));
    }
    RT(hipMemcpyAsync(filter, d->init_params, sizeof(float) * 2 * K, hipMemcpyDeviceToDevice, st));
    BABE_TRY(babe_sample_bwe(&blind, w.yb, filter, bpred, nullptr, seed, clip0, nullptr, nullptr, w.run, run, nb, stream));
    // ---- the walk: first segment against the plain filter, the others out-painted from the previous result
    RT(hipMemsetAsync(out, 0, sizeof(float) * (size_t)Lrec, st));
    if (count > 1) BABE_TRY(babe_edge_masks(w.mask, d->inpaint_dc ? w.smooth : nullptr, segL, overlap, d->dc_size, d->dc_window, stream));
    long n_end = 0;
    for (long j = 0; j < count; ++j) {
        const long ix = j * hop, n = seg_valid(j, count, Lrec, segL, hop);
        const bool last = count > 1 && j == count - 1;
        BABE_TRY(cut_norm(ix, n, w.seg));
        const float* y = w.seg;
        known.eval.mask = nullptr, known.eval.dc_mask = nullptr, known.eval.dc_y = nullptr;
        if (j > 0) {
            // the known head: the last `overlap` samples kept of the previous result, or of the whole prediction for the last segment
            // (n > overlap: the walk's last segment always reaches past its head, so clearing mask and head past n changes nothing)
            const long from = last ? segL - overlap : segL - overlap - d->discard_end;
            BABE_TRY(babe_segment_cut(w.pred + from, overlap, w.y_masked, segL, stream));
            BABE_TRY(babe_mask_blend(w.yobs, w.mask, 0, w.y_masked, w.seg, 1, segL, stream));
            y = w.yobs;
            known.eval.mask = w.mask, known.eval.mask_bs = 0;
            if (d->inpaint_dc) {
                BABE_TRY(babe_mask_blend(w.dc_y, w.smooth, 0, w.y_masked, nullptr, 1, segL, stream));
                known.eval.dc_mask = w.smooth, known.eval.dc_y = w.dc_y;
            }
        }
        BABE_TRY(babe_sample_bwe(&known, y, filter, w.pred, nullptr, seed, clip0 + nb + j, nullptr, nullptr, w.run, run, 1, stream));
        const long keep = (count == 1 || last) ? n : segL - d->discard_end;
        BABE_TRY(babe_segment_cut(w.pred, keep, out + ix, keep, stream));
        n_end = ix + keep;
    }
    // ---- undo the normalisation, in place, on what was written (the rest of out is zero)
    BABE_TRY(babe_scale_dev(out, out, n_end, inv_target, s_dev, 1, stream));
#undef RT
    return BABE_OK;
}
