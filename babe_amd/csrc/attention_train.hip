// Parameter gradients of the time-attention branch (csrc/attention.hip is its forward and input-VJP), fp32, gfx950.  Training
// only: nothing here is launched by the sampler, and the kernels of attention.hip are untouched.
//
// No float atomics: every sum has one fixed order, so results are bit-identical run to run; the per-batch-row outputs do not
// depend on which other rows share the call (the UNet's clip lanes split rows between calls).
//
// 1. qk weight gradient  dW[co][ci] = alpha * sum_b sum_t dqk[b][co][t] * a1[b][ci][t] (+ beta * dW), a GEMM with M = 2HF output
//    rows, N = HF columns and K = (b, t), both operands K-contiguous.  Summed over the batch inside the kernel: a per-row result
//    would be B x 103 MB at the deepest level.  A workgroup (four waves, 2 x 2, a 64 x 64 block of v_mfma_f32_32x32x2_f32
//    accumulators each) owns a 128 x 128 output tile and walks K in ascending (b, t) order, 32 time steps per stage through LDS
//    (row stride 33: the 32 rows a half-wave reads fall in distinct banks), the next stage's global loads in flight under the
//    MFMAs.  Time steps are loaded one float at a time, so any T works (rows need no alignment); past T they are zero.
//    The small levels (F = 64: 1024 x 512 = 32 tiles) split K into chunks of whole stages, each chunk's partial tile in the
//    workspace and a second pass adding the chunks in order; the chunk count depends on (HF, T, B) only.
//    babe_attn_qk_wgrad_bf16 is the same GEMM with both operands rounded once to bf16 on their way into LDS, on
//    v_mfma_f32_32x32x16_bf16 (mixed-precision training on the bf16 attention core); plan, workspace and reduce pass are shared.
//    Operand layout of v_mfma_f32_32x32x2_f32 (lane l): A[i][k] = A[l%32][l/32], B[k][j] = B[l/32][l%32],
//    D[i][j]: lane l holds D[(r%4) + 8*(r/4) + 4*(l/32)][l%32], r = 0..15.
//
// 2. relative-position table gradient  demb[b][k][h] = sum_{n,m: bucket[m-n+T-1] = k} scale * dS[b,h,n,m], dS = P o (dP - D) as in
//    attention.hip.  A kernel of its own whose dS tile is attn_vjp_q_kernel's (ds_tile_q, attention_f32.h: one function, so the
//    same P): a wave owns 16 queries, parks each 16 x 16 dS tile in LDS, one lane per diagonal of the tile adds its
//    sum (ascending query) into the wave's LDS array of diagonals, key tiles in ascending order; at the end lane k adds the
//    diagonals of bucket k in ascending offset and writes the query tile's partial; a last pass adds the query tiles in order.
//    The qk bias gradient is the row sum of dqk over t (double, fixed order).
//
// 3. norm2 / affine2: the plain per-channel scale pass that rebuilds proj_in's input (their parameter gradient,
//    babe_gn_param_grad_nogelu, sits beside its GELU twin in wgrad.hip).
#include "attention_f32.h"
#include "../../include/babe_hip.h"
#include <cmath>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------- qk weight gradient
constexpr int QT = 128;            // output tile (rows and columns)
constexpr int QK = 32;             // time steps per stage
constexpr int QS = QK + 1;         // LDS row stride
constexpr int HF_STEP = 512, HF_MAX = 3584;

struct QkPlan {
    int nst;        // stages per batch row
    int nsplit;     // K chunks
    int per;        // stages per chunk
    int tiles;
};

inline QkPlan qk_plan(int B, int HF, int T) {
    QkPlan p;
    p.nst = cdiv(T, QK);
    p.tiles = (2 * HF / QT) * (HF / QT);
    const long total = (long)B * p.nst;
    long want = 256 / p.tiles;                       // about one workgroup per CU
    const long cap = total / 8;                      // a chunk is at least 8 stages (256 steps of K)
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    p.per = (int)((total + want - 1) / want);
    p.nsplit = (int)((total + p.per - 1) / p.per);
    return p;
}

inline bool qk_shape_ok(int B, int HF, int T) {
    return B > 0 && T > 0 && HF >= HF_STEP && HF <= HF_MAX && HF % HF_STEP == 0;
}

// grid (tiles, nsplit), 256 threads.  direct: the only chunk, out = alpha * acc (+ beta * out); otherwise the raw partial tile.
// Tile indices, chunk bounds, accumulator clear and the epilogue are written out in this kernel and in its bf16 twin below:
// moved into shared device functions they compile to other index code ahead of the MFMA loop, which the F = 192 level's time follows.
__global__ __launch_bounds__(256) void qk_wgrad_kernel(const float* __restrict__ dqk, const float* __restrict__ a1,
                                                       float* __restrict__ out, int M, int N, int T, int B, int nst, int per,
                                                       float alpha, float beta, int direct) {
    __shared__ float Gs[QT * QS];
    __shared__ float Xs[QT * QS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int wm = wave & 1, wn = wave >> 1;
    const int tiles_n = N / QT;
    const int co0 = (blockIdx.x / tiles_n) * QT, ci0 = (blockIdx.x % tiles_n) * QT;
    const long total = (long)B * nst;
    const long s0 = (long)blockIdx.y * per;
    const long s1 = s0 + per < total ? s0 + per : total;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // loader: thread (lt, lr0) fetches time step lt of the rows lr0 + 8 i of both operands
    const int lt = tid & 31, lr0 = tid >> 5;
    float gr[16], xr[16];
    auto load = [&](long s) {
        const int b = (int)(s / nst);
        const int t = (int)(s % nst) * QK + lt;
        const bool in = t < T;
        const float* gp = dqk + ((long)b * M + co0 + lr0) * T + t;
        const float* xp = a1 + ((long)b * N + ci0 + lr0) * T + t;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            gr[i] = in ? gp[(long)8 * i * T] : 0.f;
            xr[i] = in ? xp[(long)8 * i * T] : 0.f;
        }
    };
    if (s0 < s1) load(s0);
    for (long s = s0; s < s1; ++s) {
        __syncthreads();                   // the previous stage's reads are done
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            Gs[(lr0 + 8 * i) * QS + lt] = gr[i];
            Xs[(lr0 + 8 * i) * QS + lt] = xr[i];
        }
        __syncthreads();
        if (s + 1 < s1) load(s + 1);
#pragma unroll 4
        for (int kk = 0; kk < QK / 2; ++kk) {
            const int p = 2 * kk + h;
            const float a0 = Gs[(wm * 64 + l31) * QS + p];
            const float a1v = Gs[(wm * 64 + 32 + l31) * QS + p];
            const float b0 = Xs[(wn * 64 + l31) * QS + p];
            const float b1 = Xs[(wn * 64 + 32 + l31) * QS + p];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1v, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1v, b1, acc[1][1], 0, 0, 0);
        }
    }
    float* dst = direct ? out : out + (long)blockIdx.y * M * N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int ci = ci0 + wn * 64 + j * 32 + l31;
                const long o = (long)co * N + ci;
                const float v = acc[i][j][r];
                if (direct)
                    dst[o] = beta == 0.f ? alpha * v : alpha * v + beta * dst[o];
                else
                    dst[o] = v;
            }
}

__global__ __launch_bounds__(256) void qk_wgrad_reduce_kernel(const float* __restrict__ ws, int nsplit, long n,
                                                              float* __restrict__ out, float alpha, float beta) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = 0.f;
    for (int s = 0; s < nsplit; ++s) v += ws[(long)s * n + i];
    out[i] = beta == 0.f ? alpha * v : alpha * v + beta * out[i];
}

// ---- bf16 operands (babe_attn_qk_wgrad_bf16): the same GEMM, tile, stage, chunk plan (qk_plan), workspace layout and reduce pass
// on v_mfma_f32_32x32x16_bf16.  dqk and a1 are read as fp32 (two adjacent time steps per load pair, any T, zero past T), rounded
// once to bf16 (to nearest even) and kept in LDS as bf16 pairs, row stride QB = 40 elements (80 bytes: rows stay 16-byte aligned
// and the 16 rows of a ds_read_b128 lane group start 20 banks apart, on 16 distinct 4-bank slots of the 64).  Positions are the
// MFMA's k index: lane l's fragment is the 8 consecutive time steps 16 ks + 8 (l / 32) + j of row l % 32, one 16-byte LDS read,
// two k steps per stage in ascending t.  Accumulators and output map are those of the fp32 kernel.
typedef __bf16 qk_bf16x8 __attribute__((ext_vector_type(8)));
constexpr int QB = QK + 8;

__device__ __forceinline__ unsigned qk_pack(float lo, float hi) {      // two fp32 -> bf16 pair, round to nearest even
    return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)lo) | ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)hi) << 16);
}

__global__ __launch_bounds__(256) void qk_wgrad_bf16_kernel(const float* __restrict__ dqk, const float* __restrict__ a1,
                                                            float* __restrict__ out, int M, int N, int T, int B, int nst, int per,
                                                            float alpha, float beta, int direct) {
    __shared__ __align__(16) unsigned short Gs[QT * QB];
    __shared__ __align__(16) unsigned short Xs[QT * QB];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int wm = wave & 1, wn = wave >> 1;
    const int tiles_n = N / QT;
    const int co0 = (blockIdx.x / tiles_n) * QT, ci0 = (blockIdx.x % tiles_n) * QT;
    const long total = (long)B * nst;
    const long s0 = (long)blockIdx.y * per;
    const long s1 = s0 + per < total ? s0 + per : total;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // loader: thread (lp, lr0) fetches the time steps 2 lp, 2 lp + 1 of the rows lr0 + 16 i of both operands
    const int lp = tid & 15, lr0 = tid >> 4;
    float gr[8][2], xr[8][2];
    auto load = [&](long s) {
        const int b = (int)(s / nst);
        const int t = (int)(s % nst) * QK + 2 * lp;
        const bool in0 = t < T, in1 = t + 1 < T;
        const float* gp = dqk + ((long)b * M + co0 + lr0) * T + t;
        const float* xp = a1 + ((long)b * N + ci0 + lr0) * T + t;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            gr[i][0] = in0 ? gp[(long)16 * i * T] : 0.f;
            gr[i][1] = in1 ? gp[(long)16 * i * T + 1] : 0.f;
            xr[i][0] = in0 ? xp[(long)16 * i * T] : 0.f;
            xr[i][1] = in1 ? xp[(long)16 * i * T + 1] : 0.f;
        }
    };
    if (s0 < s1) load(s0);
    for (long s = s0; s < s1; ++s) {
        __syncthreads();                   // the previous stage's reads are done
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            *reinterpret_cast<unsigned*>(Gs + (lr0 + 16 * i) * QB + 2 * lp) = qk_pack(gr[i][0], gr[i][1]);
            *reinterpret_cast<unsigned*>(Xs + (lr0 + 16 * i) * QB + 2 * lp) = qk_pack(xr[i][0], xr[i][1]);
        }
        __syncthreads();
        if (s + 1 < s1) load(s + 1);
#pragma unroll
        for (int ks = 0; ks < QK / 16; ++ks) {
            const int k = 16 * ks + 8 * h;
            const qk_bf16x8 a0 = *reinterpret_cast<const qk_bf16x8*>(Gs + (wm * 64 + l31) * QB + k);
            const qk_bf16x8 a1v = *reinterpret_cast<const qk_bf16x8*>(Gs + (wm * 64 + 32 + l31) * QB + k);
            const qk_bf16x8 b0 = *reinterpret_cast<const qk_bf16x8*>(Xs + (wn * 64 + l31) * QB + k);
            const qk_bf16x8 b1 = *reinterpret_cast<const qk_bf16x8*>(Xs + (wn * 64 + 32 + l31) * QB + k);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1v, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1v, b1, acc[1][1], 0, 0, 0);
        }
    }
    float* dst = direct ? out : out + (long)blockIdx.y * M * N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int ci = ci0 + wn * 64 + j * 32 + l31;
                const long o = (long)co * N + ci;
                const float v = acc[i][j][r];
                if (direct)
                    dst[o] = beta == 0.f ? alpha * v : alpha * v + beta * dst[o];
                else
                    dst[o] = v;
            }
}

// ---------------------------------------------------------------- table / bias gradients
inline int diag_len(int T) { return ((T + 15) & ~15) + 16; }

// grid (ceil(T/16), H, B), 64 threads, dynamic LDS diag_len(T) floats.  part [B][H][gridDim.x][nbk]
template <int FB>
__global__ __launch_bounds__(64) void attn_demb_kernel(const float* __restrict__ qk, const float* __restrict__ qkb,
                                                       const float* __restrict__ a, const int* __restrict__ bucket,
                                                       const float* __restrict__ emb, int nbk, const float* __restrict__ dout,
                                                       const float* __restrict__ lse, const float* __restrict__ D,
                                                       float* __restrict__ part, int H, int T, float scale) {
    constexpr int F = FB * 64;
    __shared__ float Qs[F * 16];
    __shared__ float dOs[F * 16];
    __shared__ float emb_lds[64];
    __shared__ float tile[16 * 17];            // dS[m - m0][n - n0]
    extern __shared__ float diag[];            // entry j: the sum over the diagonal m - n = j - 15 - n0 of this wave's queries
    const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
    const int n0 = blockIdx.x * 16, h = blockIdx.y;
    const Head p = head_of(qk, qkb, a, H, F, T);
    const int nd = ((T + 15) & ~15) + 16;
    if (lane < nbk) emb_lds[lane] = emb[lane * H + h];
    for (int i = lane; i < nd; i += 64) diag[i] = 0.f;
    stage16(Qs, p.Q, p.qb, F, T, n0);
    stage16(dOs, dout + p.hb * F * T, nullptr, F, T, n0);
    __syncthreads();
    const int n = n0 + lr;
    const bool nin = n < T;
    const float L = nin ? lse[p.hb * T + n] : 0.f;
    const float Dn = nin ? D[p.hb * T + n] : 0.f;
    for (int m0 = 0; m0 < T; m0 += 16) {
        float ds[4];
        ds_tile_q<F>(p.K, p.kb, p.V, Qs, dOs, bucket, emb_lds, m0, n, nin, L, Dn, T, scale, ds);
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[(4 * lg + r) * 17 + lr] = ds[r];
        __syncthreads();
        attn_diag_add(tile, diag + m0, lane);
        __syncthreads();
    }
    if (lane < nbk) {
        float accb = 0.f;
        for (int j = 0; j < nd; ++j)
            if (attn_diag_in_bucket(bucket, j, n0, T, lane)) accb += diag[j];
        part[((long)p.hb * gridDim.x + blockIdx.x) * nbk + lane] = accb * scale;
    }
}

// the table half of the fp32 core (the other half is attention.hip's F32Core), behind attention_common.h's attn_param_vjp_host
struct F32Table {
    static constexpr int ROWS = 16;
    static constexpr int TBL_LDS_LIMIT = 65536;        // static + dynamic: no opt-in
    // static LDS of attn_demb_kernel<F/64> + its diagonals
    static long tbl_lds_bytes(int F, int T) { return 4L * (2L * F * 16 + 64 + 16 * 17 + diag_len(T)); }
    template <int FB>
    static int tbl(const char*, dim3 grid, hipStream_t s, const float* qk, const float* qkb, const float* a, const int* bucket,
                   const float* emb, int nbk, const float* dout, const float* lse, const float* D, float* part, int H, int T,
                   float scale) {
        hipLaunchKernelGGL(attn_demb_kernel<FB>, grid, dim3(64), diag_len(T) * sizeof(float), s, qk, qkb, a, bucket, emb, nbk, dout,
                           lse, D, part, H, T, scale);
        return BABE_OK;
    }
};

// ---------------------------------------------------------------- scale pass
// grid (ceil(hw/1024), C, B), 256 threads
__global__ __launch_bounds__(256) void scale_channels_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                             float* __restrict__ out, int C, long hw) {
    const float sc = scale[(long)blockIdx.z * C + blockIdx.y];
    const long base = ((long)blockIdx.z * C + blockIdx.y) * hw;
    const long i0 = (long)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long i = i0 + 256 * k;
        if (i < hw) out[base + i] = x[base + i] * sc;
    }
}

// babe_attn_qk_wgrad (`who` = "attn_qk_wgrad") and babe_attn_qk_wgrad_bf16: the same plan, workspace and reduce pass around `kernel`
template <class Kernel>
int qk_wgrad_host(const char* who, Kernel kernel, const float* dqk, const float* a1, float* dW, float* ws, int B, int HF, int T,
                  float alpha, float beta, void* stream) {
    BABE_CHECK_ARG(dqk && a1 && dW, "%s: null pointer", who);
    BABE_CHECK_ARG(qk_shape_ok(B, HF, T), "%s: unsupported shape B=%d HF=%d T=%d (HF a multiple of %d, at most %d)", who, B, HF, T,
                   HF_STEP, HF_MAX);
    const QkPlan p = qk_plan(B, HF, T);
    BABE_CHECK_ARG(p.nsplit == 1 || ws, "%s: this shape needs a workspace (babe_%s_workspace)", who, who);
    hipStream_t s = (hipStream_t)stream;
    const int M = 2 * HF, N = HF;
    const int direct = p.nsplit == 1;
    hipLaunchKernelGGL(kernel, dim3(p.tiles, p.nsplit), dim3(256), 0, s, dqk, a1, direct ? dW : ws, M, N, T, B, p.nst, p.per, alpha,
                       beta, direct);
    BABE_LAUNCH_CHECK();
    if (!direct) {
        const long n = (long)M * N;
        hipLaunchKernelGGL(qk_wgrad_reduce_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, ws, p.nsplit, n, dW, alpha, beta);
        BABE_LAUNCH_CHECK();
    }
    return BABE_OK;
}

}  // namespace

extern "C" long babe_attn_qk_wgrad_workspace(int B, int HF, int T) {
    if (!qk_shape_ok(B, HF, T)) return -1;
    const QkPlan p = qk_plan(B, HF, T);
    return p.nsplit > 1 ? (long)p.nsplit * 2 * HF * HF : 0;
}

extern "C" int babe_attn_qk_wgrad(const float* dqk, const float* a1, float* dW, float* ws, int B, int HF, int T, float alpha,
                                  float beta, void* stream) {
    return qk_wgrad_host("attn_qk_wgrad", qk_wgrad_kernel, dqk, a1, dW, ws, B, HF, T, alpha, beta, stream);
}

extern "C" long babe_attn_qk_wgrad_bf16_workspace(int B, int HF, int T) { return babe_attn_qk_wgrad_workspace(B, HF, T); }

extern "C" int babe_attn_qk_wgrad_bf16(const float* dqk, const float* a1, float* dW, float* ws, int B, int HF, int T, float alpha,
                                       float beta, void* stream) {
    return qk_wgrad_host("attn_qk_wgrad_bf16", qk_wgrad_bf16_kernel, dqk, a1, dW, ws, B, HF, T, alpha, beta, stream);
}

extern "C" long babe_attn_param_vjp_workspace(int B, int H, int T, int num_buckets) {
    if (B <= 0 || H <= 0 || T <= 0 || num_buckets < 0 || num_buckets > 64) return -1;
    return (long)B * H * T + (long)B * H * cdiv(T, 16) * num_buckets;
}

extern "C" int babe_attn_param_vjp(const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb,
                                   int num_buckets, const float* out, const float* lse, const float* dout, const float* dqk,
                                   float* ws, float* demb_rows, long demb_bs, float* dqkb_rows, long dqkb_bs, int B, int H, int F,
                                   int T, float scale, void* stream) {
    return attn_param_vjp_host<F32Table>("attn_param_vjp", qk, qk_bias, a, bucket, emb, num_buckets, out, lse, dout, dqk, ws, demb_rows,
                                         demb_bs, dqkb_rows, dqkb_bs, B, H, F, T, scale, stream);
}

extern "C" int babe_scale_channels(const float* x, const float* scale, float* out, int B, int C, long hw, void* stream) {
    BABE_CHECK_ARG(x && scale && out && B > 0 && C > 0 && hw > 0 && B <= 65535 && C <= 65535, "scale_channels: bad arguments");
    hipLaunchKernelGGL(scale_channels_kernel, dim3(cdiv(hw, 1024), C, B), dim3(256), 0, (hipStream_t)stream, x, scale, out, C, hw);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}
