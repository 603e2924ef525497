// What the fp32 and the bf16 time-attention kernels (attention.hip, attention_bf16.hip, attention_train.hip) share: the shape
// contract and the dispatch on F / 64, the head pointers, the lane-group reductions of the softmax, the D = rowdot(dO, O) pass
// of the input-VJP, the diagonal sums and the last passes of the table and qk-bias gradients, and the host body of each
// entry-point pair (a core supplies its kernels, its rows per workgroup and its LDS test).
#pragma once
#include "common.h"
#include <type_traits>

constexpr int ATTN_FMAX = 448;          // largest head dimension (7 octaves x 64 bins)

typedef float floatx4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float max16x4(float v) {           // max over the 4 lane groups that share l % 16
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float sum16x4(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// The operands of head blockIdx.y of batch item blockIdx.z, for the bf16 kernels and the fp32 table kernel.  (The fp32 forward
// and input-VJP kernels of attention.hip keep this preamble written out: taking it from here they compiled to other address
// code and register allocation, and attn_fwd at F = 192 and attn_vjp at F = 320 measured 0.3 - 1.2 % slower.)
struct Head {
    const float *Q, *K, *qb, *kb, *V;   // Q rows (K rows follow at + F*T), their biases (nullptr: none), a[b][h]
    long hb;                    // (b * H + h): the head's index into [B][H][...] tensors
};
__device__ __forceinline__ Head head_of(const float* qk, const float* qkb, const float* a, int H, int F, int T) {
    const int h = blockIdx.y, b = blockIdx.z;
    Head p;
    p.Q = qk + ((long)b * 2 * H * F + (long)h * 2 * F) * T;
    p.K = p.Q + (long)F * T;
    p.qb = qkb ? qkb + h * 2 * F : nullptr;
    p.kb = qkb ? p.qb + F : nullptr;
    p.hb = (long)b * H + h;
    p.V = a + p.hb * F * T;
    return p;
}

// Table gradient of both cores: a wave has parked a 16 x 16 dS tile as tile[m - m0][n - n0] (row stride 17); lane j < 31 adds
// the diagonal (m - m0) - (n - n0) = j - 15, queries ascending, to diag[j] (the caller passes the tile's place in its array of
// diagonals and has made the tile visible to the wave)
__device__ __forceinline__ void attn_diag_add(const float* tile, float* diag, int lane) {
    if (lane < 31) {
        const int lo = lane < 15 ? 15 - lane : 0, hi = lane > 15 ? 30 - lane : 15;
        float sum = 0.f;
        for (int q = lo; q <= hi; ++q) sum += tile[(q + lane - 15) * 17 + q];
        diag[lane] += sum;
    }
}
// entry j of the diagonals of the query tile at nb holds the offset m - n = j - 15 - nb: does it fall in bucket k?
__device__ __forceinline__ bool attn_diag_in_bucket(const int* bucket, int j, int nb, int T, int k) {
    const int idx = j - 15 - nb + T - 1;
    return idx >= 0 && idx <= 2 * T - 2 && bucket[idx] == k;
}

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

// The one switch on F / 64 (attn_check_shape has passed): fn(std::integral_constant<int, FB>) -> status, FB = F / 64 = 1..7
template <class Fn>
static inline int attn_dispatch(int F, Fn fn) {
    switch (F / 64) {
        case 1: return fn(std::integral_constant<int, 1>{});
        case 2: return fn(std::integral_constant<int, 2>{});
        case 3: return fn(std::integral_constant<int, 3>{});
        case 4: return fn(std::integral_constant<int, 4>{});
        case 5: return fn(std::integral_constant<int, 5>{});
        case 6: return fn(std::integral_constant<int, 6>{});
        default: return fn(std::integral_constant<int, 7>{});
    }
}

// ---------------------------------------------------------------- host bodies, one per entry-point pair
// `who` is the caller's name for the messages.  A Core has ROWS (own rows of a workgroup) and the launchers the body names,
// templates on FB = F / 64 that return a status with its message set; what only one core checks (the bf16 core's pointer
// alignment, its LDS opt-in) stays with that core.  A body uses only the members it names, so a Core need not have them all:
// the fp32 core is F32Core (attention.hip: fwd, vjp) and F32Table (attention_train.hip: tbl and its LDS test), one per source.
template <class Core>
static int attn_fwd_host(const char* who, const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb,
                         int num_buckets, float* out, float* lse, int B, int H, int F, int T, float scale, void* stream) {
    BABE_CHECK_ARG(qk && a && out && lse, "%s: null pointer", who);
    BABE_CHECK_ARG(!bucket == !emb, "%s: bucket table and embedding go together", who);
    const int nbk = bucket ? num_buckets : 0;
    if (int e = attn_check_shape(who, B, H, F, T, nbk)) return e;
    const dim3 grid(cdiv(T, Core::ROWS), H, B);
    BABE_TRY(attn_dispatch(F, [&](auto fb) {
        return Core::template fwd<decltype(fb)::value>(who, grid, (hipStream_t)stream, qk, qk_bias, a, bucket, emb, nbk, out, lse, H, T,
                                                       scale);
    }));
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

template <class Core>
static int attn_vjp_host(const char* who, const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb,
                         int num_buckets, const float* out, const float* lse, const float* dout, float* D, float* dqk, float* dv,
                         int B, int H, int F, int T, float scale, void* stream) {
    BABE_CHECK_ARG(qk && a && out && lse && dout && D && dqk && dv, "%s: null pointer", who);
    BABE_CHECK_ARG(!bucket == !emb, "%s: bucket table and embedding go together", who);
    const int nbk = bucket ? num_buckets : 0;
    if (int e = attn_check_shape(who, B, H, F, T, nbk)) return e;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(attn_rowdot_kernel, dim3(cdiv(T, 256), H, B), dim3(256), 0, s, dout, out, D, H, F, T);
    BABE_LAUNCH_CHECK();
    const dim3 grid(cdiv(T, Core::ROWS), H, B);
    BABE_TRY(attn_dispatch(F, [&](auto fb) {
        return Core::template vjp<decltype(fb)::value>(who, grid, s, qk, qk_bias, a, bucket, emb, nbk, dout, lse, D, dqk, dv, H, T,
                                                       scale);
    }));
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

// Table and qk-bias gradients.  The core's table pass, Core::tbl, writes part [B][H][ceil(T/16)][nbk] from the D this body forms
// with the kernel and the operands of the input-VJP; its LDS grows with T: Core::tbl_lds_bytes against Core::TBL_LDS_LIMIT.
template <class Core>
static int attn_param_vjp_host(const char* who, const float* qk, const float* qk_bias, const float* a, const int* bucket,
                               const float* emb, int num_buckets, const float* out, const float* lse, const float* dout,
                               const float* dqk, float* ws, float* demb_rows, long demb_bs, float* dqkb_rows, long dqkb_bs, int B,
                               int H, int F, int T, float scale, void* stream) {
    BABE_CHECK_ARG(!bucket == !emb && !bucket == !demb_rows, "%s: bucket table, embedding and demb_rows go together", who);
    const int nbk = bucket ? num_buckets : 0;
    if (int e = attn_check_shape(who, B, H, F, T, nbk)) return e;
    BABE_CHECK_ARG(demb_rows || dqkb_rows, "%s: nothing to compute", who);
    BABE_CHECK_ARG(!dqkb_rows || (dqk && dqkb_bs >= 2L * H * F), "%s: dqkb_rows needs dqk and dqkb_bs >= 2HF", who);
    hipStream_t s = (hipStream_t)stream;
    if (demb_rows) {
        BABE_CHECK_ARG(qk && a && out && lse && dout && ws, "%s: null pointer", who);
        BABE_CHECK_ARG(nbk > 0 && demb_bs >= (long)nbk * H, "%s: demb_bs %ld < num_buckets*H", who, demb_bs);
        BABE_CHECK_ARG(Core::tbl_lds_bytes(F, T) <= Core::TBL_LDS_LIMIT, "%s: F=%d with T=%d needs %ld bytes of LDS (limit %d)", who,
                       F, T, Core::tbl_lds_bytes(F, T), Core::TBL_LDS_LIMIT);
        float* D = ws;
        float* part = ws + (long)B * H * T;
        hipLaunchKernelGGL(attn_rowdot_kernel, dim3(cdiv(T, 256), H, B), dim3(256), 0, s, dout, out, D, H, F, T);
        BABE_LAUNCH_CHECK();
        const dim3 grid(cdiv(T, Core::ROWS), H, B);
        BABE_TRY(attn_dispatch(F, [&](auto fb) {
            return Core::template tbl<decltype(fb)::value>(who, grid, s, qk, qk_bias, a, bucket, emb, nbk, dout, lse, D, part, H, T,
                                                           scale);
        }));
        BABE_LAUNCH_CHECK();
        hipLaunchKernelGGL(attn_demb_sum_kernel, dim3(B), dim3(256), 0, s, part, cdiv(T, 16), nbk, H, demb_rows, demb_bs);
        BABE_LAUNCH_CHECK();
    }
    if (dqkb_rows) {
        const int R = 2 * H * F;
        hipLaunchKernelGGL(attn_rowsum_t_kernel, dim3(cdiv(R, 4), B), dim3(256), 0, s, dqk, R, T, dqkb_rows, dqkb_bs);
        BABE_LAUNCH_CHECK();
    }
    return BABE_OK;
}
