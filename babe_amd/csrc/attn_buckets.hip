// The relative-position bucket table of the time attention: on the host (babe_attn_buckets), and written ON THE DEVICE, for the
// library-side UNet sequencer (csrc/unet_engine.hip): the table's length 2T-1 is known at call time only, and that sequencer
// allocates nothing, copies nothing from the host and never synchronises.  The bucket of a key-minus-query offset d is
// non-decreasing in |d| and constant from max_distance on, so `half - 1` thresholds (half = num_buckets / 2) and the sign
// describe the whole function; they are derived on the host from babe_attn_buckets itself, once per plan, and reach the kernel
// by value.  No logarithm is evaluated on the device.
#include "common.h"
#include "../../include/babe_hip.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace {

__global__ __launch_bounds__(256) void attn_bucket_table_kernel(babe_attn_bucket_thr thr, int T, int* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * T - 1) return;
    const int rel = i - (T - 1);                       // key position - query position
    const int n = rel < 0 ? -rel : rel;
    int v = 0;
    for (int k = 0; k < thr.half - 1; ++k) v += thr.thr[k] <= n ? 1 : 0;
    out[i] = (rel >= 0 ? thr.half : 0) + v;
}

}  // namespace

extern "C" int babe_attn_buckets(int* out, int T, int num_buckets, int max_distance) {
    BABE_CHECK_ARG(out && T > 0 && num_buckets >= 4 && max_distance > num_buckets / 4, "attn_buckets: bad arguments");
    // T5 bidirectional buckets exactly as the reference evaluates them in float32 (torch: n.float() / max_exact, log,
    // division by the Python scalar log(max_distance / max_exact) as multiplication by its float reciprocal, then .long())
    const int nb = num_buckets / 2, max_exact = nb / 2;
    const float inv = 1.f / (float)std::log((double)max_distance / (double)max_exact);
    for (int i = 0; i < 2 * T - 1; ++i) {
        const int rel = i - (T - 1);          // key position - query position
        const int n = rel < 0 ? -rel : rel;
        int v;
        if (n < max_exact) {
            v = n;
        } else {
            const float lf = logf((float)n / (float)max_exact);
            long large = max_exact + (long)(lf * inv * (float)(nb - max_exact));
            if (large > nb - 1) large = nb - 1;
            v = (int)large;
        }
        out[i] = (rel >= 0 ? nb : 0) + v;
    }
    return BABE_OK;
}

extern "C" int babe_attn_bucket_thresholds(babe_attn_bucket_thr* out, int num_buckets, int max_distance) {
    BABE_CHECK_ARG(out, "attn_bucket_thresholds: null output");
    BABE_CHECK_ARG(num_buckets >= 4 && num_buckets <= 64 && num_buckets % 2 == 0,
                   "attn_bucket_thresholds: num_buckets = %d unsupported (even, 4..64)", num_buckets);
    BABE_CHECK_ARG(max_distance > num_buckets / 4 && max_distance <= 65536,
                   "attn_bucket_thresholds: max_distance = %d unsupported (%d..65536 for %d buckets)", max_distance, num_buckets / 4 + 1,
                   num_buckets);
    const int half = num_buckets / 2, Tt = max_distance + 1;        // offsets 0 .. max_distance: the upper half of a table of Tt steps
    std::vector<int> tab((size_t)2 * Tt - 1);
    BABE_TRY(babe_attn_buckets(tab.data(), Tt, num_buckets, max_distance));
    const int* up = tab.data() + (Tt - 1);                           // up[n] = half + bucket of |d| = n
    memset(out, 0, sizeof *out);
    out->half = half, out->max_distance = max_distance;
    for (int n = 0; n <= max_distance; ++n) {
        const int v = up[n] - half, w = n ? tab[Tt - 1 - n] : 0;     // ... and the lower half carries the same value without the offset
        BABE_CHECK_ARG(v >= 0 && v < half && v == w && (n == 0 ? v == 0 : v >= up[n - 1] - half),
                       "attn_bucket_thresholds: the buckets of num_buckets = %d, max_distance = %d are not monotone in the distance",
                       num_buckets, max_distance);
    }
    BABE_CHECK_ARG(up[max_distance] - half == half - 1,
                   "attn_bucket_thresholds: max_distance = %d does not reach the last of %d buckets", max_distance, num_buckets);
    for (int k = 1; k < half; ++k) {
        int n = 0;
        while (up[n] - half < k) ++n;                                // (ends: the last bucket is reached at max_distance)
        out->thr[k - 1] = n;
    }
    return BABE_OK;
}

extern "C" int babe_attn_bucket_table(const babe_attn_bucket_thr* thr, int T, int* out, void* stream) {
    BABE_CHECK_ARG(thr && out, "attn_bucket_table: null pointer");
    BABE_CHECK_ARG(T > 0 && T < (1 << 30), "attn_bucket_table: bad length T=%d", T);
    BABE_CHECK_ARG(thr->half >= 2 && thr->half <= 32, "attn_bucket_table: bad thresholds (half = %d)", thr->half);
    hipLaunchKernelGGL(attn_bucket_table_kernel, dim3(cdiv(2L * T - 1, 256)), dim3(256), 0, (hipStream_t)stream, *thr, T, out);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}
