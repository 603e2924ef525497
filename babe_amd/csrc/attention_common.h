// What the fp32 and the bf16 time-attention kernels (attention.hip, attention_bf16.hip, attention_train.hip) share: the shape
// contract, the D = rowdot(dO, O) pass of the input-VJP, and the last passes of the table and qk-bias gradients.
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

// Parameter-gradient passes of both cores (attention_train.hip, and attention_bf16.hip's babe_attn_param_vjp_bf16).
// demb_rows[b][k][h] = sum over query tiles, ascending; grid (B), 256 threads
static __global__ __launch_bounds__(256) void attn_demb_sum_kernel(const float* __restrict__ part, int nqt, int nbk, int H,
                                                       float* __restrict__ rows, long rows_bs) {
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < nbk * H; i += 256) {
        const int k = i / H, h = i % H;
        const float* p = part + ((long)b * H + h) * nqt * nbk + k;
        float v = 0.f;
        for (int q = 0; q < nqt; ++q) v += p[(long)q * nbk];
        rows[(long)b * rows_bs + i] = v;
    }
}

// rows[b][r] = sum_t x[b][r][t]; one wave per row; grid (ceil(R/4), B), 256 threads
static __global__ __launch_bounds__(256) void attn_rowsum_t_kernel(const float* __restrict__ x, int R, int T, float* __restrict__ rows,
                                                       long rows_bs) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, b = blockIdx.y;
    if (r >= R) return;
    const float* p = x + ((long)b * R + r) * T;
    double s = 0;
    for (int t = lane; t < T; t += 64) s += (double)p[t];
    s = wave_sum(s);
    if (lane == 0) rows[(long)b * rows_bs + r] = (float)s;
}

static inline int attn_check_shape(const char* who, int B, int H, int F, int T, int nbk) {
    BABE_CHECK_ARG(B > 0 && H > 0 && T > 0, "%s: bad shape B=%d H=%d T=%d", who, B, H, T);
    BABE_CHECK_ARG(F % 64 == 0 && F >= 64 && F <= ATTN_FMAX, "%s: F=%d unsupported (need a multiple of 64, at most %d)", who, F,
                   ATTN_FMAX);
    BABE_CHECK_ARG(nbk >= 0 && nbk <= 64, "%s: %d buckets unsupported (at most 64)", who, nbk);
    return BABE_OK;
}
