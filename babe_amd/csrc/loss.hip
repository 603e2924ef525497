// A-weighted training loss (diff_params/edm.py:201-206 with utils/training_utils.py:124-138): the FIR pre-emphasis of the error
// fused with the subtraction in front of it and the square behind it, and its transpose fused with the square's derivative.
//   forward : d = est - tgt;   ew[n] = sum_k taps[k] d[n + k - K/2];   err2 = ew * ew
//   backward: h = 2 g ew;      dest[m] = sum_k taps[k] h[m - k + K/2]  = the same FIR over h with the taps reversed (K odd)
// One pass over HBM per direction.  Grid (ceil(L / 2048), B); a workgroup of 256 threads stages its 2048 outputs' inputs plus the
// K-1 halo into LDS once (zeros outside the signal) and every thread produces two runs of 4 consecutive outputs, 1024 apart, from
// 16-byte LDS reads (lane l reads 4 consecutive floats at 4 l: no bank conflict) that both runs' taps share.  The window starts at
// a multiple of 4 samples - the taps are shifted right by (4 - K/2 % 4) % 4 zeros to make up for it - so global loads and stores
// are 16 bytes wide wherever the row is 16-byte aligned.  Every output is written once, each sum runs k = 0 .. K-1 in order.
#include "common.h"
#include "../../include/babe_hip.h"
#include "prof.h"

namespace {

constexpr int LS_TILE = 2048;                    // outputs per workgroup
constexpr int LS_KMAX = 255;                     // taps; shifted by up to 3 and padded to a multiple of 4: 256
constexpr int LS_KPAD = 256;
constexpr int LS_WIN = LS_TILE + LS_KPAD;        // staged samples (the reads of the last run end at TILE - 4 + KPAD + 3)

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Keeps a 16-byte LDS read whole: without it the compiler carries 3 window values instead of 4 and fetches the next 4 from an
// odd offset as pairs of 4-byte reads, which cost twice the LDS cycles of one ds_read_b128.
__device__ __forceinline__ float4 whole(float4 v) {
    asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
    return v;
}

// BWD = false: a = est, b = tgt, staged value a - b, outputs o1 = ew and o2 = ew^2
// BWD = true : a = g,   b = ew,  staged value 2 a b, taps reversed, output o1 = dest
template <bool BWD>
__global__ __launch_bounds__(256) void fir_sqerr_kernel(const float* __restrict__ a, long a_bs, const float* __restrict__ b,
                                                        long b_bs, const float* __restrict__ taps, int K,
                                                        float* __restrict__ o1, float* __restrict__ o2, int L) {
    __shared__ __attribute__((aligned(16))) float st[LS_KPAD];
    __shared__ __attribute__((aligned(16))) float sx[LS_WIN];
    const int row = blockIdx.y;
    const long n0 = (long)blockIdx.x * LS_TILE;
    const int P = K / 2;
    const int P4 = (P + 3) & ~3;                 // the window starts at n0 - P4, a multiple of 4
    const int shift = P4 - P;
    const int Kp = (K + shift + 3) & ~3;         // <= 256
    const int W = LS_TILE + Kp;
    const float* pa = a + (long)row * a_bs;
    const float* pb = b + (long)row * b_bs;

    for (int i = threadIdx.x; i < Kp; i += 256) {
        const int k = i - shift;
        st[i] = (k >= 0 && k < K) ? taps[BWD ? K - 1 - k : k] : 0.f;
    }
    const bool vec_in = aligned16(pa) && aligned16(pb);
    const long lo = n0 - P4;
    for (int i = threadIdx.x * 4; i < W; i += 1024) {
        const long s = lo + i;
        float4 v;
        if (vec_in && s >= 0 && s + 3 < L) {
            const float4 x = *reinterpret_cast<const float4*>(pa + s);
            const float4 y = *reinterpret_cast<const float4*>(pb + s);
            if (BWD) {
                v.x = 2.f * x.x * y.x; v.y = 2.f * x.y * y.y; v.z = 2.f * x.z * y.z; v.w = 2.f * x.w * y.w;
            } else {
                v.x = x.x - y.x; v.y = x.y - y.y; v.z = x.z - y.z; v.w = x.w - y.w;
            }
        } else {
            float e[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long t = s + q;
                float r = 0.f;
                if (t >= 0 && t < L) r = BWD ? 2.f * pa[t] * pb[t] : pa[t] - pb[t];
                e[q] = r;
            }
            v.x = e[0]; v.y = e[1]; v.z = e[2]; v.w = e[3];
        }
        *reinterpret_cast<float4*>(&sx[i]) = v;
    }
    __syncthreads();

    // out[n0 + j + r] = sum_i st[i] * sx[j + r + i],  j = 4 * tid (+ 1024), r = 0..3
    const int j = threadIdx.x * 4;
    float acc0[4] = {0.f, 0.f, 0.f, 0.f}, acc1[4] = {0.f, 0.f, 0.f, 0.f};
    float4 w0 = *reinterpret_cast<const float4*>(&sx[j]);
    float4 w1 = *reinterpret_cast<const float4*>(&sx[j + 1024]);
    for (int i = 0; i < Kp; i += 4) {
        const float4 t = *reinterpret_cast<const float4*>(&st[i]);
        const float4 n0v = whole(*reinterpret_cast<const float4*>(&sx[j + i + 4]));
        const float4 n1v = whole(*reinterpret_cast<const float4*>(&sx[j + 1024 + i + 4]));
        const float x0[8] = {w0.x, w0.y, w0.z, w0.w, n0v.x, n0v.y, n0v.z, n0v.w};
        const float x1[8] = {w1.x, w1.y, w1.z, w1.w, n1v.x, n1v.y, n1v.z, n1v.w};
        const float tt[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc0[r] = __builtin_fmaf(tt[q], x0[q + r], acc0[r]);
                acc1[r] = __builtin_fmaf(tt[q], x1[q + r], acc1[r]);
            }
        }
        w0 = n0v;
        w1 = n1v;
    }

    float* q1 = o1 + (long)row * L;
    float* q2 = BWD ? nullptr : o2 + (long)row * L;
    const bool vec_out = aligned16(q1) && (BWD || aligned16(q2));
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float* acc = p ? acc1 : acc0;
        const long n = n0 + j + p * 1024;
        if (n >= L) continue;
        if (vec_out && n + 3 < L) {
            *reinterpret_cast<float4*>(q1 + n) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            if (!BWD) *reinterpret_cast<float4*>(q2 + n) = make_float4(acc[0] * acc[0], acc[1] * acc[1], acc[2] * acc[2], acc[3] * acc[3]);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (n + r < L) {
                    q1[n + r] = acc[r];
                    if (!BWD) q2[n + r] = acc[r] * acc[r];
                }
            }
        }
    }
}

// Frequency-resolved error of the training log: out[b][f] = (1/T) sum_t |c[b][.][f][t]|^2 of planar CQT coefficients.  One
// workgroup of 256 threads per (b, f) row pair.  The sum has ONE order whatever the run: per thread serially over its samples
// (stride 256, or four consecutive samples at stride 1024 from 16-byte loads when both rows allow them), then down the wave of 64
// lanes by halving offsets, then the four waves' sums from LDS as (s0 + s1) + (s2 + s3), then one division.  No atomics.
// Every term is non-negative and no partial sum passes more than ceil(T / 256) + 11 roundings, which bounds the relative error.
constexpr int BE_THREADS = 256;

__global__ __launch_bounds__(BE_THREADS) void plane_bin_energy_kernel(const float* __restrict__ c, float* __restrict__ out,
                                                                      int F, int T) {
    __shared__ float part[BE_THREADS / 64];
    const long row = blockIdx.x;                         // b * F + f
    const long b = row / F, f = row - b * F;
    const float* re = c + ((b * 2) * F + f) * (long)T;
    const float* im = re + (long)F * T;
    float acc = 0.f;
    if ((T & 3) == 0 && aligned16(re) && aligned16(im)) {
        for (int i = threadIdx.x * 4; i < T; i += BE_THREADS * 4) {
            const float4 x = *reinterpret_cast<const float4*>(re + i);
            const float4 y = *reinterpret_cast<const float4*>(im + i);
            const float t0 = __builtin_fmaf(y.x, y.x, x.x * x.x), t1 = __builtin_fmaf(y.y, y.y, x.y * x.y);
            const float t2 = __builtin_fmaf(y.z, y.z, x.z * x.z), t3 = __builtin_fmaf(y.w, y.w, x.w * x.w);
            acc += (t0 + t1) + (t2 + t3);
        }
    } else {
        for (int i = threadIdx.x; i < T; i += BE_THREADS) {
            const float x = re[i], y = im[i];
            acc += __builtin_fmaf(y, y, x * x);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[row] = ((part[0] + part[1]) + (part[2] + part[3])) / (float)T;
}

}  // namespace

extern "C" int babe_plane_bin_energy(const float* c, float* out, int B, int F, int T, void* stream) {
    BABE_CHECK_ARG(c && out, "plane_bin_energy: null pointer");
    BABE_CHECK_ARG(B >= 1 && F >= 1 && T >= 1, "plane_bin_energy: bad shape (B %d, F %d, T %d)", B, F, T);
    BABE_CHECK_ARG((long)B * F <= 2147483647L, "plane_bin_energy: B * F = %ld rows (at most 2^31 - 1)", (long)B * F);
    BabeProfScope prof(BABE_SLOT_SAMPLER, 8.0 * B * F * (double)T + 4.0 * B * F, 4.0 * B * F * (double)T, 0, stream);
    hipLaunchKernelGGL(plane_bin_energy_kernel, dim3((unsigned)((long)B * F)), dim3(BE_THREADS), 0, (hipStream_t)stream, c, out,
                       F, T);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" int babe_fir_sqerr_fwd(const float* est, long est_bs, const float* tgt, long tgt_bs, const float* taps, int K,
                                  float* ew, float* err2, int B, int L, void* stream) {
    BABE_CHECK_ARG(est && tgt && taps && ew && err2, "fir_sqerr_fwd: null pointer");
    BABE_CHECK_ARG(K >= 1 && K <= LS_KMAX && (K & 1), "fir_sqerr_fwd: K = %d (odd, 1 .. 255)", K);
    BABE_CHECK_ARG(B >= 1 && B <= 65535 && L >= 1, "fir_sqerr_fwd: bad shape (B %d, L %d)", B, L);
    BabeProfScope prof(BABE_SLOT_SAMPLER, 16.0 * B * (double)L, 2.0 * B * (double)L * K, 0, stream);
    hipLaunchKernelGGL(fir_sqerr_kernel<false>, dim3(cdiv(L, LS_TILE), B), dim3(256), 0, (hipStream_t)stream, est, est_bs, tgt,
                       tgt_bs, taps, K, ew, err2, L);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" int babe_fir_sqerr_bwd(const float* g, long g_bs, const float* ew, const float* taps, int K, float* dest, int B,
                                  int L, void* stream) {
    BABE_CHECK_ARG(g && ew && taps && dest, "fir_sqerr_bwd: null pointer");
    BABE_CHECK_ARG(K >= 1 && K <= LS_KMAX && (K & 1), "fir_sqerr_bwd: K = %d (odd, 1 .. 255)", K);
    BABE_CHECK_ARG(B >= 1 && B <= 65535 && L >= 1, "fir_sqerr_bwd: bad shape (B %d, L %d)", B, L);
    BabeProfScope prof(BABE_SLOT_SAMPLER, 12.0 * B * (double)L, 2.0 * B * (double)L * K, 0, stream);
    hipLaunchKernelGGL(fir_sqerr_kernel<true>, dim3(cdiv(L, LS_TILE), B), dim3(256), 0, (hipStream_t)stream, g, g_bs, ew,
                       (long)L, taps, K, dest, (float*)nullptr, L);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}
