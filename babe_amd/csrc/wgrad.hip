// Parameter gradients of the CQTDiff+ UNet for training (fp32, gfx950): conv weight gradients on the fp32 MFMA pipe (and, as an
// opt-in, with bf16 operands on the bf16 MFMA pipe: wgrad_bf16_partial_kernel below), the FiLM gate
// gradient from the same per-row partials, the per-channel GroupNorm * FiLM reduction and the Linear backward of the FiLM /
// embedding MLP.  Replaces autograd's convolution_backward (weight), the GroupNorm / Linear parameter backward of
// the reference's networks/cqtdiff+.py:382-493 and :167-211 in its trainer's loss.backward().
//
// No float atomics anywhere: every sum has one fixed order, so results are bit-identical run to run and the per-batch-row
// results do not depend on which other rows were in the same call (the UNet's clip lanes split rows between calls).
//
// Conv weight gradient as a GEMM per batch row b:  P_b[co][(ci, kh, kw)] = sum_pos G[co][pos] * X[ci][pos + shift(kh, kw)].
// M = output channels (A operand = output gradient), N = input channels x taps (B operand = shifted activations), K = positions.
// A workgroup owns 64 output x 32 input channels and ALL taps of a chunk of positions; a step stages one frequency row of 64
// time steps: G [64][64] and the activation halo X [32][KH rows at the dilated offsets][64 + KW - 1] once in LDS, and every
// tap reads its shifted window from that halo.  Four waves: (output half, tap parity) for the (5,3) kernel (8 / 7 taps per
// wave, one 32x32 accumulator each), (output half, position half) for (1,1) with the two halves added in a fixed order.
// Chunks of positions give each (b, chunk) its own partial tile in the workspace; babe_conv_wgrad_rows adds the chunks in
// order.  Chunk count depends on the shape only (not on B).
#include "common.h"
#include "../../include/babe_hip.h"
#include "gelu.h"

namespace {

typedef float wg_f32x16 __attribute__((ext_vector_type(16)));

constexpr int TT = 64;                   // positions (time steps of one frequency row) per step
constexpr int CO_T = 64, CI_T = 32;      // output x input channels per workgroup

template <int KH, int KW>
__global__ __launch_bounds__(256, 2) void wgrad_partial_kernel(babe_wgrad_args a, float* __restrict__ ws, int nchunks, int per,
                                                                int ntt, int ci_tiles) {
    constexpr int NT = KH * KW;
    constexpr int XW = TT + KW - 1;
    constexpr int XS = (KH * XW) | 1;    // odd channel stride: the 32 channels a half-wave reads fall in distinct banks
    constexpr int GS = TT + 1;
    constexpr int TAPW = NT == 1 ? 1 : (NT + 1) / 2;
    __shared__ float Gs[CO_T * GS];
    __shared__ float Xs[(CI_T * XS) > 2048 ? (CI_T * XS) : 2048];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int cw = wave & 1, tw = wave >> 1;
    const int co0 = (blockIdx.x / ci_tiles) * CO_T, ci0 = (blockIdx.x % ci_tiles) * CI_T;
    const int chunk = blockIdx.y, b = blockIdx.z;
    const long nwork = (long)a.F * ntt;
    const long w0 = (long)chunk * per;
    const long w1 = w0 + per < nwork ? w0 + per : nwork;
    wg_f32x16 acc[TAPW];
#pragma unroll
    for (int j = 0; j < TAPW; ++j)
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    const float* gb = a.g + (long)b * a.g_bs;
    const float* xb = a.x + (long)b * a.x_bs;
    const float* x2b = a.x2 ? a.x2 + (long)b * a.x2_bs : nullptr;
    const int split = a.x2 ? a.cin_split : a.Cin;
    const int kk0 = NT == 1 ? tw * (TT / 4) : 0;
    const int kk1 = NT == 1 ? kk0 + TT / 4 : TT / 2;
    for (long w = w0; w < w1; ++w) {
        const int f = (int)(w / ntt);
        const int t0 = (int)(w % ntt) * TT;
        for (int i = tid; i < CO_T * TT; i += 256) {
            const int co = i / TT, t = i % TT;
            float v = 0.f;
            if (co0 + co < a.Cout && t0 + t < a.T) v = gb[(long)(co0 + co) * a.g_cs + (long)f * a.T + t0 + t];
            Gs[co * GS + t] = v;
        }
        for (int i = tid; i < CI_T * KH * XW; i += 256) {
            const int ci = i / (KH * XW);
            const int r = i % (KH * XW);
            const int kh = r / XW, j = r % XW;
            const int fr = f + a.dil * (kh - KH / 2);
            const int t = t0 + j - KW / 2;
            const int c = ci0 + ci;
            float v = 0.f;
            if (c < a.Cin && fr >= 0 && fr < a.F && t >= 0 && t < a.T) {
                const float* src = c < split ? xb + (long)c * a.x_cs : x2b + (long)(c - split) * a.x2_cs;
                v = src[(long)fr * a.T + t];
            }
            Xs[ci * XS + kh * XW + j] = v;
        }
        __syncthreads();
        for (int kk = kk0; kk < kk1; ++kk) {
            const int p = 2 * kk + h;
            const float av = Gs[(cw * 32 + l31) * GS + p];
#pragma unroll
            for (int j = 0; j < TAPW; ++j) {
                const int tap = NT == 1 ? 0 : tw + 2 * j;
                if (tap < NT) {
                    const int kh = tap / KW, kw = tap % KW;
                    const float bv = Xs[l31 * XS + kh * XW + p + kw];
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[j], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    if (NT == 1) {                        // (1,1): the two position halves, added in a fixed order
        if (tw == 1)
            for (int r = 0; r < 16; ++r) Xs[(cw * 16 + r) * 64 + lane] = acc[0][r];
        __syncthreads();
        if (tw == 1) return;
        for (int r = 0; r < 16; ++r) acc[0][r] += Xs[(cw * 16 + r) * 64 + lane];
    }
    const long K = (long)a.Cin * NT;
    float* dst = ws + ((long)b * nchunks + chunk) * a.Cout * K;
    const int ci = ci0 + l31;
    if (ci >= a.Cin) return;
#pragma unroll
    for (int j = 0; j < TAPW; ++j) {
        const int tap = NT == 1 ? 0 : tw + 2 * j;
        if (tap >= NT) continue;
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + cw * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (co < a.Cout) dst[(long)co * K + (long)ci * NT + tap] = acc[j][r];
        }
    }
}

// ---- bf16 operands (babe_conv_wgrad_bf16_rows): the same GEMM, tile (64 output x 32 input channels), step (one frequency row of
// 64 time steps), chunking and workspace layout as above, on v_mfma_f32_32x32x16_bf16.  g and X are read as fp32, rounded once
// to bf16 (round to nearest even) and kept in LDS as bf16 pairs; positions are the MFMA's k index, so a lane's A fragment is 8
// consecutive time steps of a g row (one aligned 16-byte LDS read) and its B fragment 8 consecutive time steps of an X row
// shifted by kw - 1.  An X row sits in LDS with its left neighbour in front and its body 16-byte aligned; the lane reads the 6
// dwords that cover its 8 steps and both neighbours once per frequency tap and forms the three time taps in registers: kw = 1
// is the aligned 16-byte read as it is, kw = 0 and kw = 2 are 16-bit funnel shifts (v_alignbit_b32 / v_perm_b32) of it with
// the dword before and the dword after.  Waves: (output half, taps
// 0..7 | 8..14) for (5,3) - a wave reads only 3 of the 5 frequency-tap rows -, (output half, position half) for (1,1).
// Staging: where every row is 16-byte aligned (T % 4 == 0, aligned bases and strides) a thread's float4 loads of step j+1
// are issued before step j's MFMAs (all addressing precomputed outside the loop), converted and written to the OTHER LDS
// buffer after them: one barrier per step.  Anything else takes the element-wise staging of the fp32 kernel (into the other
// buffer as well), which is correct for any alignment and not fast.
typedef __bf16 wg_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 wg_bf16x2 __attribute__((ext_vector_type(2)));
typedef float wg_f32x2 __attribute__((ext_vector_type(2)));
typedef float wg_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned wg_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned wg_u32x2 __attribute__((ext_vector_type(2)));

constexpr int BRW = 36;                  // dwords per LDS row (72 bf16): 16-byte aligned rows, 32 lanes' b128 reads spread over the banks

__device__ __forceinline__ unsigned wg_pack(float lo, float hi) {      // two fp32 -> bf16 pair, round to nearest even (v_cvt_pk_bf16_f32)
    wg_f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, wg_bf16x2));
}
__device__ __forceinline__ unsigned short wg_bf16_bits(float v) {
    return __builtin_bit_cast(unsigned short, (__bf16)v);
}

// the MFMAs of one staged step for wave (cw, TW); G: [64][BRW] dwords, X: [32][KH][BRW] dwords
template <int KH, int KW, int TW, int NACC>
__device__ __forceinline__ void wg_bf16_mma(const unsigned* __restrict__ G, const unsigned* __restrict__ X, int cw, int l31, int h,
                                            wg_f32x16 (&acc)[NACC]) {
    constexpr int NT = KH * KW;
    const unsigned* grow = G + (cw * 32 + l31) * BRW + 4 * h;
    const unsigned* xrow = X + l31 * (KH * BRW) + 4 * h;
    if constexpr (NT == 1) {
#pragma unroll
        for (int ks = 2 * TW; ks < 2 * TW + 2; ++ks) {
            const wg_u32x4 av = *(const wg_u32x4*)(grow + 8 * ks);
            const wg_u32x4 bv = *(const wg_u32x4*)(xrow + 8 * ks);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(wg_bf16x8, av), __builtin_bit_cast(wg_bf16x8, bv), acc[0],
                                                            0, 0, 0);
        }
    } else {
        static_assert(KW == 3 || NT == 1, "time taps are formed for KW == 3");
#pragma unroll 1
        for (int ks = 0; ks < TT / 16; ++ks) {
            const wg_u32x4 av = *(const wg_u32x4*)(grow + 8 * ks);
            const wg_bf16x8 a = __builtin_bit_cast(wg_bf16x8, av);
#pragma unroll
            for (int kh = 0; kh < KH; ++kh) {
                if (kh * KW + KW - 1 < TW * 8 || kh * KW >= TW * 8 + 8) continue;     // no tap of this wave in the row
                const unsigned* xr = xrow + kh * BRW + 8 * ks;                         // dwords 3 | 4..7 | 8 of the lane's window
                const unsigned p = xr[3], e = xr[8];
                const wg_u32x4 d = *(const wg_u32x4*)(xr + 4);
#pragma unroll
                for (int kw = 0; kw < KW; ++kw) {
                    const int j = kh * KW + kw - TW * 8;
                    if (j < 0 || j >= 8) continue;
                    wg_u32x4 bv;
                    if (kw == 0)
                        bv = wg_u32x4{__builtin_amdgcn_alignbit(d[0], p, 16), __builtin_amdgcn_alignbit(d[1], d[0], 16),
                                      __builtin_amdgcn_alignbit(d[2], d[1], 16), __builtin_amdgcn_alignbit(d[3], d[2], 16)};
                    else if (kw == 1)
                        bv = d;
                    else
                        bv = wg_u32x4{__builtin_amdgcn_alignbit(d[1], d[0], 16), __builtin_amdgcn_alignbit(d[2], d[1], 16),
                                      __builtin_amdgcn_alignbit(d[3], d[2], 16), __builtin_amdgcn_alignbit(e, d[3], 16)};
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(wg_bf16x8, bv), acc[j], 0, 0, 0);
                }
            }
        }
    }
}

template <int KH, int KW, bool ALIGNED>
__global__ __launch_bounds__(256, 2) void wgrad_bf16_partial_kernel(babe_wgrad_args a, float* __restrict__ ws, int nchunks, int per,
                                                                     int ntt, int ci_tiles) {
    constexpr int NT = KH * KW;
    constexpr int NACC = NT == 1 ? 1 : 8;
    constexpr int XO = NT == 1 ? 0 : 2;             // an X row in LDS: element jj = t - t0 + XO sits in dword XD + jj / 2 of its row, so
    constexpr int XD = NT == 1 ? 0 : 3;             // that the body starts 16-byte aligned (dword 4); dword 36 is the next row's unused dword 0
    constexpr int XCS = KH * BRW;                   // dwords per X channel
    constexpr int NGQ = CO_T * (TT / 4) / 256;      // float4 loads of g per thread and step (4)
    constexpr int NXQ = CI_T * KH * (TT / 4) / 256; // ... of X (2 KH: two channels, every tap row)
    __shared__ __attribute__((aligned(16))) unsigned Gs[2][CO_T * BRW];
    __shared__ __attribute__((aligned(16))) unsigned Xs[2][CI_T * XCS + 4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int cw = wave & 1, tw = wave >> 1;
    const int co0 = (blockIdx.x / ci_tiles) * CO_T, ci0 = (blockIdx.x % ci_tiles) * CI_T;
    const int chunk = blockIdx.y, b = blockIdx.z;
    const long nwork = (long)a.F * ntt;
    const long w0 = (long)chunk * per;
    const long w1 = w0 + per < nwork ? w0 + per : nwork;
    wg_f32x16 acc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j)
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    const float* gb = a.g + (long)b * a.g_bs;
    const float* xb = a.x + (long)b * a.x_bs;
    const float* x2b = a.x2 ? a.x2 + (long)b * a.x2_bs : nullptr;
    const int split = a.x2 ? a.cin_split : a.Cin;
    const int T = a.T, F = a.F;

    // loop-invariant addressing of the aligned staging: thread (r16, quad column q4) loads the g rows r16 + 16 k and every tap
    // row of the X channels r16 and r16 + 16; what changes with the step, (f + dil (kh - KH/2)) T + t0, is wave-uniform
    const int q4 = (tid & 15) * 4, r16 = tid >> 4;
    const float* gsrc = gb + (long)(co0 + r16) * a.g_cs + q4;
    const long g16 = 16 * a.g_cs;
    const float* xsrc[2];
    const float* hsrc = nullptr;                   // halo columns t0 - 1 and t0 + 64: thread i < 32 KH owns (channel, tap row) i
    int hdf = 0;
    if constexpr (ALIGNED) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int c = ci0 + r16 + 16 * k;
            xsrc[k] = c >= a.Cin ? nullptr : (c < split ? xb + (long)c * a.x_cs : x2b + (long)(c - split) * a.x2_cs) + q4;
        }
        if (NT > 1 && tid < CI_T * KH) {
            const int c = ci0 + tid / KH;
            hdf = a.dil * (tid % KH - KH / 2);
            hsrc = c >= a.Cin ? nullptr : (c < split ? xb + (long)c * a.x_cs : x2b + (long)(c - split) * a.x2_cs);
        }
    }
    wg_f32x4 gq[NGQ], xq[NXQ];
    float hl = 0.f, hr = 0.f;

    auto load = [&](int f, int t0) {               // ALIGNED: global -> registers
        const wg_f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const bool tin = t0 + q4 < T;              // T % 4 == 0: a quad is inside or outside as a whole
        const long gofs = (long)f * T + t0;
#pragma unroll
        for (int k = 0; k < NGQ; ++k)
            gq[k] = (co0 + r16 + 16 * k < a.Cout && tin) ? *(const wg_f32x4*)(gsrc + k * g16 + gofs) : z;
#pragma unroll
        for (int kh = 0; kh < KH; ++kh) {
            const int fr = f + a.dil * (kh - KH / 2);
            const bool fin = fr >= 0 && fr < F;
            const long xofs = (long)fr * T + t0;
#pragma unroll
            for (int k = 0; k < 2; ++k) xq[k * KH + kh] = (xsrc[k] && tin && fin) ? *(const wg_f32x4*)(xsrc[k] + xofs) : z;
        }
        if (NT > 1) {
            const int fr = f + hdf;
            const bool ok = hsrc && fr >= 0 && fr < F;
            hl = (ok && t0 > 0) ? hsrc[(long)fr * T + t0 - 1] : 0.f;
            hr = (ok && t0 + TT < T) ? hsrc[(long)fr * T + t0 + TT] : 0.f;
        }
    };
    auto store = [&](int buf) {                    // ALIGNED: registers -> bf16 pairs in LDS
#pragma unroll
        for (int k = 0; k < NGQ; ++k) {
            unsigned* d = &Gs[buf][(r16 + 16 * k) * BRW + (tid & 15) * 2];
            d[0] = wg_pack(gq[k][0], gq[k][1]);
            d[1] = wg_pack(gq[k][2], gq[k][3]);
        }
#pragma unroll
        for (int k = 0; k < NXQ; ++k) {
            unsigned* d = &Xs[buf][(r16 + 16 * (k / KH)) * XCS + (k % KH) * BRW + (tid & 15) * 2 + XD + XO / 2];
            d[0] = wg_pack(xq[k][0], xq[k][1]);
            d[1] = wg_pack(xq[k][2], xq[k][3]);
        }
        if (NT > 1 && tid < CI_T * KH) {
            unsigned* d = &Xs[buf][(tid / KH) * XCS + (tid % KH) * BRW + XD];
            d[0] = wg_pack(0.f, hl);               // jj = 0 (never used), 1 (t0 - 1)
            d[TT / 2 + 1] = wg_pack(hr, 0.f);      // jj = 66 (t0 + 64), 67 (never used)
        }
    };
    auto stage_any = [&](int buf, int f, int t0) { // element-wise: any alignment, any T
        unsigned short* G16 = (unsigned short*)Gs[buf];
        unsigned short* X16 = (unsigned short*)Xs[buf];
        for (int i = tid; i < CO_T * TT; i += 256) {
            const int co = i / TT, t = i % TT;
            float v = 0.f;
            if (co0 + co < a.Cout && t0 + t < T) v = gb[(long)(co0 + co) * a.g_cs + (long)f * T + t0 + t];
            G16[co * (2 * BRW) + t] = wg_bf16_bits(v);
        }
        constexpr int XW = TT + 2 * XO;            // jj = 0 .. 67 for (5,3): every element a fragment read can touch
        for (int i = tid; i < CI_T * KH * XW; i += 256) {
            const int ci = i / (KH * XW);
            const int r = i % (KH * XW);
            const int kh = r / XW, jj = r % XW;
            const int fr = f + a.dil * (kh - KH / 2);
            const int t = t0 + jj - XO;
            const int c = ci0 + ci;
            float v = 0.f;
            if (c < a.Cin && fr >= 0 && fr < F && t >= 0 && t < T && jj >= XO - KW / 2 && jj < XO + TT + KW / 2) {
                const float* src = c < split ? xb + (long)c * a.x_cs : x2b + (long)(c - split) * a.x2_cs;
                v = src[(long)fr * T + t];
            }
            X16[ci * (2 * XCS) + kh * (2 * BRW) + 2 * XD + jj] = wg_bf16_bits(v);
        }
    };

    int f = (int)(w0 / ntt), tt = (int)(w0 % ntt);
    if (w0 < w1) {
        if constexpr (ALIGNED) {
            load(f, tt * TT);
            store(0);
        } else {
            stage_any(0, f, tt * TT);
        }
    }
    __syncthreads();
    int buf = 0;
    for (long w = w0; w < w1; ++w) {
        if (++tt == ntt) tt = 0, ++f;              // (f, tt) of step w + 1
        const bool more = w + 1 < w1;
        if constexpr (ALIGNED)
            if (more) load(f, tt * TT);
        if (tw == 0)
            wg_bf16_mma<KH, KW, 0>(Gs[buf], Xs[buf], cw, l31, h, acc);
        else
            wg_bf16_mma<KH, KW, 1>(Gs[buf], Xs[buf], cw, l31, h, acc);
        if (more) {
            if constexpr (ALIGNED)
                store(buf ^ 1);
            else
                stage_any(buf ^ 1, f, tt * TT);
        }
        __syncthreads();
        buf ^= 1;
    }
    if (NT == 1) {                        // (1,1): the two position halves, added in a fixed order
        float* red = (float*)Xs;
        if (tw == 1)
            for (int r = 0; r < 16; ++r) red[(cw * 16 + r) * 64 + lane] = acc[0][r];
        __syncthreads();
        if (tw == 1) return;
        for (int r = 0; r < 16; ++r) acc[0][r] += red[(cw * 16 + r) * 64 + lane];
    }
    const long K = (long)a.Cin * NT;
    float* dst = ws + ((long)b * nchunks + chunk) * a.Cout * K;
    const int ci = ci0 + l31;
    if (ci >= a.Cin) return;
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
        const int tap = NT == 1 ? 0 : tw * 8 + j;
        if (tap >= NT) continue;
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + cw * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (co < a.Cout) dst[(long)co * K + (long)ci * NT + tap] = acc[j][r];
        }
    }
}

__device__ double block_sum_d(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// grid (Cout, B): chunks added in order, scaled row written, optional gate dot
__global__ __launch_bounds__(256) void wgrad_rows_kernel(const float* __restrict__ ws, int nchunks, int Cout, long K,
                                                         const float* __restrict__ oscale, float alpha,
                                                         const float* __restrict__ w, float* __restrict__ dgate, long dgate_bs,
                                                         float galpha, float* __restrict__ rows, long rows_bs) {
    __shared__ double sh[256];
    const int co = blockIdx.x, b = blockIdx.y;
    const float s = alpha * (oscale ? oscale[(long)b * Cout + co] : 1.f);
    double dot = 0;
    for (long k = threadIdx.x; k < K; k += 256) {
        float v = 0.f;
        for (int c = 0; c < nchunks; ++c) v += ws[(((long)b * nchunks + c) * Cout + co) * K + k];
        rows[(long)b * rows_bs + (long)co * K + k] = s * v;
        if (w) dot += (double)w[(long)co * K + k] * (double)v;
    }
    if (dgate) {
        dot = block_sum_d(dot, sh);
        if (threadIdx.x == 0) dgate[(long)b * dgate_bs + co] = (float)((double)galpha * dot);
    }
}

__global__ __launch_bounds__(256) void rows_sum_kernel(const float* __restrict__ rows, long rows_bs, int B, long n,
                                                       float* __restrict__ out, float beta) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = 0.f;
    for (int b = 0; b < B; ++b) v += rows[(long)b * rows_bs + i];
    out[i] = beta == 0.f ? v : beta * out[i] + v;
}

// grid (C, B).  GELU = false: a = z * scale without the GELU (norm2 / affine2 of the attention branch); scale is not read.
template <bool GELU>
__global__ __launch_bounds__(256) void gn_param_kernel(const float* __restrict__ z, const float* __restrict__ da,
                                                       const float* __restrict__ scale, const float* __restrict__ stats,
                                                       const float* __restrict__ gamma, const float* __restrict__ film,
                                                       long film_bs, float cs, float* __restrict__ dg, long dg_bs,
                                                       float* __restrict__ dfilm, long dfilm_bs, int C, int G, long hw) {
    __shared__ double sh[256];
    const int c = blockIdx.x, b = blockIdx.y;
    const long base = ((long)b * C + c) * hw;
    double s = 0;
    if (GELU) {
        const float sc = scale[(long)b * C + c];
        for (long i = threadIdx.x; i < hw; i += 256) {
            const float x = z[base + i];
            s += (double)(da[base + i] * babe_gelu::gelu_grad_f(x * sc)) * (double)x;
        }
    } else {
        for (long i = threadIdx.x; i < hw; i += 256) s += (double)da[base + i] * (double)z[base + i];
    }
    s = block_sum_d(s, sh);
    if (threadIdx.x == 0) {
        const double ds = (double)cs * s;
        const double r = stats[((long)b * G + c / (C / G)) * 3 + 2];
        dg[(long)b * dg_bs + c] = (float)(ds * ((double)film[(long)b * film_bs + c] + 1.0) * r);
        dfilm[(long)b * dfilm_bs + c] = (float)(ds * (double)gamma[c] * r);
    }
}

__device__ __forceinline__ float lin_dp(const float* dy, const float* y, long i) {
    const float d = dy[i];
    return (y && !(y[i] > 0.f)) ? 0.f : d;
}

__global__ __launch_bounds__(256) void linear_bwd_w_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                           const float* __restrict__ x, float* __restrict__ dW,
                                                           float* __restrict__ db, int B, int K, int J, float beta) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)J * K) return;
    const int j = (int)(i / K), k = (int)(i % K);
    float s = 0.f, sb = 0.f;
    for (int b = 0; b < B; ++b) {
        const float dp = lin_dp(dy, y, (long)b * J + j);
        s += dp * x[(long)b * K + k];
        sb += dp;
    }
    dW[i] = beta == 0.f ? s : beta * dW[i] + s;
    if (k == 0 && db) db[j] = beta == 0.f ? sb : beta * db[j] + sb;
}

constexpr int LIN_JS = 256;      // rows of W per dx partial

// grid (ceil(K/64), S): ws[(s*B + b)*K + k] = sum over j in split s of dp[b][j] W[j][k]
__global__ __launch_bounds__(256) void linear_bwd_x_partial(const float* __restrict__ dy, const float* __restrict__ y,
                                                            const float* __restrict__ W, float* __restrict__ ws, int B, int K,
                                                            int J) {
    __shared__ float sh[4][64];
    const int kk = threadIdx.x & 63, jl = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + kk;
    const int s = blockIdx.y;
    const int j0 = s * LIN_JS, j1 = j0 + LIN_JS < J ? j0 + LIN_JS : J;
    for (int b = 0; b < B; ++b) {
        float acc = 0.f;
        if (k < K)
            for (int j = j0 + jl; j < j1; j += 4) acc += lin_dp(dy, y, (long)b * J + j) * W[(long)j * K + k];
        sh[jl][kk] = acc;
        __syncthreads();
        if (jl == 0 && k < K) ws[((long)s * B + b) * K + k] = ((sh[0][kk] + sh[1][kk]) + sh[2][kk]) + sh[3][kk];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void linear_bwd_x_final(const float* __restrict__ ws, float* __restrict__ dx, int B, int K,
                                                          int S) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * K) return;
    float v = 0.f;
    for (int s = 0; s < S; ++s) v += ws[(long)s * B * K + i];
    dx[i] = v;
}

inline void wg_plan(const babe_wgrad_args& a, int& ntt, int& ci_tiles, int& tiles, int& nchunks, int& per) {
    ntt = cdiv(a.T, TT);
    ci_tiles = cdiv(a.Cin, CI_T);
    tiles = cdiv(a.Cout, CO_T) * ci_tiles;
    const long nwork = (long)a.F * ntt;
    // ~256 workgroups per batch row, each chunk at least 32 steps (2048 positions) so that writing its partial tile costs
    // little next to its MFMA work
    long c = (256 + tiles - 1) / tiles;
    const long cmax = (nwork + 31) / 32;
    if (c > cmax) c = cmax;
    if (c < 1) c = 1;
    per = (int)((nwork + c - 1) / c);
    nchunks = (int)((nwork + per - 1) / per);
}

bool wg_args_ok(const babe_wgrad_args* a) {
    return a && a->x && a->g && a->B > 0 && a->Cin > 0 && a->Cout > 0 && a->F > 0 && a->T > 0 && a->dil >= 1 &&
           ((a->KH == 5 && a->KW == 3) || (a->KH == 1 && a->KW == 1)) && a->Cin <= 512 && a->Cout <= 512 &&
           (!a->x2 || (a->cin_split > 0 && a->cin_split < a->Cin));
}

}  // namespace

extern "C" long babe_conv_wgrad_workspace(const babe_wgrad_args* a) {
    if (!wg_args_ok(a)) return -1;
    int ntt, ci_tiles, tiles, nchunks, per;
    wg_plan(*a, ntt, ci_tiles, tiles, nchunks, per);
    return (long)a->B * nchunks * a->Cout * a->Cin * a->KH * a->KW;
}

extern "C" int babe_conv_wgrad_rows(const babe_wgrad_args* a, float* ws, const float* oscale, float alpha, const float* w,
                                    float* dgate, long dgate_bs, float galpha, float* rows, long rows_bs, void* stream) {
    BABE_CHECK_ARG(wg_args_ok(a), "conv_wgrad: unsupported arguments (KH x KW must be 5x3 or 1x1, channels <= 512)");
    BABE_CHECK_ARG(ws && rows && (!dgate || w), "conv_wgrad: bad pointers");
    const long K = (long)a->Cin * a->KH * a->KW;
    BABE_CHECK_ARG(rows_bs >= (long)a->Cout * K, "conv_wgrad: rows_bs %ld < Cout*Cin*KH*KW", rows_bs);
    int ntt, ci_tiles, tiles, nchunks, per;
    wg_plan(*a, ntt, ci_tiles, tiles, nchunks, per);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(tiles, nchunks, a->B);
    if (a->KH == 5)
        hipLaunchKernelGGL((wgrad_partial_kernel<5, 3>), grid, dim3(256), 0, s, *a, ws, nchunks, per, ntt, ci_tiles);
    else
        hipLaunchKernelGGL((wgrad_partial_kernel<1, 1>), grid, dim3(256), 0, s, *a, ws, nchunks, per, ntt, ci_tiles);
    BABE_LAUNCH_CHECK();
    hipLaunchKernelGGL(wgrad_rows_kernel, dim3(a->Cout, a->B), dim3(256), 0, s, ws, nchunks, a->Cout, K, oscale, alpha, w, dgate,
                       dgate_bs, galpha, rows, rows_bs);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" long babe_conv_wgrad_bf16_workspace(const babe_wgrad_args* a) { return babe_conv_wgrad_workspace(a); }

extern "C" int babe_conv_wgrad_bf16_rows(const babe_wgrad_args* a, float* ws, const float* oscale, float alpha, const float* w,
                                         float* dgate, long dgate_bs, float galpha, float* rows, long rows_bs, void* stream) {
    BABE_CHECK_ARG(wg_args_ok(a), "conv_wgrad_bf16: unsupported arguments (KH x KW must be 5x3 or 1x1, channels <= 512)");
    BABE_CHECK_ARG(ws && rows && (!dgate || w), "conv_wgrad_bf16: bad pointers");
    const long K = (long)a->Cin * a->KH * a->KW;
    BABE_CHECK_ARG(rows_bs >= (long)a->Cout * K, "conv_wgrad_bf16: rows_bs %ld < Cout*Cin*KH*KW", rows_bs);
    int ntt, ci_tiles, tiles, nchunks, per;
    wg_plan(*a, ntt, ci_tiles, tiles, nchunks, per);
    // float4 staging: every row of every view starts on a 16-byte boundary
    auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    const bool aligned = a->T % 4 == 0 && al(a->x) && al(a->g) && a->x_cs % 4 == 0 && a->g_cs % 4 == 0 &&
                         (a->B == 1 || (a->x_bs % 4 == 0 && a->g_bs % 4 == 0)) &&
                         (!a->x2 || (al(a->x2) && a->x2_cs % 4 == 0 && (a->B == 1 || a->x2_bs % 4 == 0)));
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(tiles, nchunks, a->B);
#define WG_BF16_LAUNCH(KH, KW, AL) \
    hipLaunchKernelGGL((wgrad_bf16_partial_kernel<KH, KW, AL>), grid, dim3(256), 0, s, *a, ws, nchunks, per, ntt, ci_tiles)
    if (a->KH == 5) {
        if (aligned) WG_BF16_LAUNCH(5, 3, true); else WG_BF16_LAUNCH(5, 3, false);
    } else {
        if (aligned) WG_BF16_LAUNCH(1, 1, true); else WG_BF16_LAUNCH(1, 1, false);
    }
#undef WG_BF16_LAUNCH
    BABE_LAUNCH_CHECK();
    hipLaunchKernelGGL(wgrad_rows_kernel, dim3(a->Cout, a->B), dim3(256), 0, s, ws, nchunks, a->Cout, K, oscale, alpha, w, dgate,
                       dgate_bs, galpha, rows, rows_bs);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" int babe_rows_sum(const float* rows, long rows_bs, int B, long n, float* out, float beta, void* stream) {
    BABE_CHECK_ARG(rows && out && B > 0 && n > 0 && (B == 1 || rows_bs >= n), "rows_sum: bad arguments");
    hipLaunchKernelGGL(rows_sum_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, rows, rows_bs, B, n, out, beta);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

static int gn_param_launch(bool gelu, const float* z, const float* da, const float* scale, const float* stats, const float* gamma,
                           const float* film_aff, long film_bs, float cs, float* dgamma_rows, long dg_bs, float* dfilm,
                           long dfilm_bs, int B, int C, int G, long hw, void* stream) {
    BABE_CHECK_ARG(z && da && (scale || !gelu) && stats && gamma && film_aff && dgamma_rows && dfilm && B > 0 && C > 0 && G > 0 &&
                   C % G == 0 && hw > 0, "gn_param_grad: bad arguments");
    if (gelu)
        hipLaunchKernelGGL(gn_param_kernel<true>, dim3(C, B), dim3(256), 0, (hipStream_t)stream, z, da, scale, stats, gamma, film_aff,
                           film_bs, cs, dgamma_rows, dg_bs, dfilm, dfilm_bs, C, G, hw);
    else
        hipLaunchKernelGGL(gn_param_kernel<false>, dim3(C, B), dim3(256), 0, (hipStream_t)stream, z, da, scale, stats, gamma, film_aff,
                           film_bs, cs, dgamma_rows, dg_bs, dfilm, dfilm_bs, C, G, hw);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" int babe_gn_param_grad(const float* z, const float* da, const float* scale, const float* stats, const float* gamma,
                                  const float* film_aff, long film_bs, float cs, float* dgamma_rows, long dg_bs, float* dfilm,
                                  long dfilm_bs, int B, int C, int G, long hw, void* stream) {
    return gn_param_launch(true, z, da, scale, stats, gamma, film_aff, film_bs, cs, dgamma_rows, dg_bs, dfilm, dfilm_bs, B, C, G, hw,
                           stream);
}

/* babe_gn_param_grad for a = z * scale without the GELU (norm2 / affine2 of the attention branch) */
extern "C" int babe_gn_param_grad_nogelu(const float* z, const float* da, const float* stats, const float* gamma,
                                         const float* film_aff, long film_bs, float cs, float* dgamma_rows, long dg_bs, float* dfilm,
                                         long dfilm_bs, int B, int C, int G, long hw, void* stream) {
    return gn_param_launch(false, z, da, nullptr, stats, gamma, film_aff, film_bs, cs, dgamma_rows, dg_bs, dfilm, dfilm_bs, B, C, G, hw,
                           stream);
}

extern "C" long babe_linear_bwd_workspace(int B, int K, int J) {
    if (B <= 0 || K <= 0 || J <= 0) return -1;
    return (long)cdiv(J, LIN_JS) * B * K;
}

extern "C" int babe_linear_bwd(const float* dy, const float* y, const float* x, const float* W, float* dW, float* db, float* dx,
                               float* ws, int B, int K, int J, float beta, void* stream) {
    BABE_CHECK_ARG(dy && x && W && dW && B > 0 && K > 0 && J > 0 && (!dx || ws), "linear_bwd: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(linear_bwd_w_kernel, dim3(cdiv((long)J * K, 256)), dim3(256), 0, s, dy, y, x, dW, db, B, K, J, beta);
    BABE_LAUNCH_CHECK();
    if (dx) {
        const int S = cdiv(J, LIN_JS);
        hipLaunchKernelGGL(linear_bwd_x_partial, dim3(cdiv(K, 64), S), dim3(256), 0, s, dy, y, W, ws, B, K, J);
        BABE_LAUNCH_CHECK();
        hipLaunchKernelGGL(linear_bwd_x_final, dim3(cdiv((long)B * K, 256)), dim3(256), 0, s, ws, dx, B, K, S);
        BABE_LAUNCH_CHECK();
    }
    return BABE_OK;
}
