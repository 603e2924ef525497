// What the fp32 and the bf16 time-attention kernels (attention.hip, attention_bf16.hip) share: the shape contract and the
// D = rowdot(dO, O) pass of the input-VJP.
#pragma once
#include "common.h"

constexpr int ATTN_FMAX = 448;          // largest head dimension (7 octaves x 64 bins)

// D[b][h][n] = sum_f dO[f][n] O[f][n]; grid (ceil(T/256), H, B), 256 threads
static __global__ __launch_bounds__(256) void attn_rowdot_kernel(const float* __restrict__ dout, const float* __restrict__ out,
                                                                 float* __restrict__ D, int H, int F, int T) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= T) return;
    const long base = ((long)blockIdx.z * H + blockIdx.y) * F * T + n;
    float s = 0.f;
    for (int f = 0; f < F; ++f) s += dout[base + (long)f * T] * out[base + (long)f * T];
    D[((long)blockIdx.z * H + blockIdx.y) * T + n] = s;
}

static inline int attn_check_shape(const char* who, int B, int H, int F, int T, int nbk) {
    BABE_CHECK_ARG(B > 0 && H > 0 && T > 0, "%s: bad shape B=%d H=%d T=%d", who, B, H, T);
    BABE_CHECK_ARG(F % 64 == 0 && F >= 64 && F <= ATTN_FMAX, "%s: F=%d unsupported (need a multiple of 64, at most %d)", who, F,
                   ATTN_FMAX);
    BABE_CHECK_ARG(nbk >= 0 && nbk <= 64, "%s: %d buckets unsupported (at most 64)", who, nbk);
    return BABE_OK;
}
