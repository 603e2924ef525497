// Time attention of the CQTDiff+ ResnetBlock (TimeAttentionBlock, networks/cqtdiff+.py in the reference): forward and input-VJP.
//
// Per batch item b and head h, with F frequency features and T time steps, read in their native channel-major layout
// (T contiguous), straight from the qk Conv1d output and the head projection a:
//   Q[f][n] = qk[b][h*2F + f][n] (+ qb[h*2F + f]),  K[f][m] = qk[b][h*2F + F + f][m] (+ qb[...]),  V[f][m] = a[b][h][f][m]
//   S[n][m] = (sum_f Q[f][n] K[f][m] + bias_h(m - n)) * scale,    bias_h(d) = emb[bucket[d + T - 1]][h]   (0 without rel-pos)
//   O[f][n] = sum_m softmax_m(S)[n][m] V[f][m],   lse[n] = log sum_m exp S[n][m]
// VJP (inputs only; the weight and bias-table gradients are attention_train.hip's), D[n] = sum_f dO[f][n] O[f][n], P recomputed
// from Q, K and lse:
//   dS = P o (dP - D), dP[n][m] = sum_f dO[f][n] V[f][m]
//   dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO
// Two VJP kernels, one over query tiles (dQ) and one over key tiles (dK, dV), each owning the rows it writes: no atomics, the
// result does not depend on scheduling (bit-identical run to run and across streams).
//
// Every product is a v_mfma_f32_16x16x4_f32 (exact fp32).  One wave per workgroup owns 16 rows of its side (queries for the
// forward and dQ, keys for dK/dV); those 16 columns of the wave's own operands sit in LDS, the streamed side is read from
// global memory (L2-resident: one head's Q, K, V are at most 3 x 448 x 4096 floats).  The softmax is online over 16-key tiles,
// so any T works, including a ragged last tile (masked keys get probability 0, masked queries are never stored).
// Operand layout of v_mfma_f32_16x16x4_f32 (lane l):  A[i][k] = A[l%16][l/16],  B[k][j] = B[l/16][l%16],
// D[i][j]: lane l holds D[4*(l/16) + r][l%16], r = 0..3.
// The scores are formed TRANSPOSED where the probabilities feed the next product as its B operand (forward, dQ: S^T, rows =
// keys) and untransposed where they feed it as B over queries (dK/dV: S, rows = queries): the accumulator's four rows per lane
// are then exactly the k-slots of four consecutive MFMA steps, so P never leaves its registers.
#include "attention_f32.h"
#include "../../include/babe_hip.h"
#include <cmath>

namespace {

// ---------------------------------------------------------------- forward (FB = F / 64)
// grid (ceil(T/16), H, B), 64 threads
template <int FB>
__global__ __launch_bounds__(64) void attn_fwd_kernel(const float* __restrict__ qk, const float* __restrict__ qkb,
                                                      const float* __restrict__ a, const int* __restrict__ bucket,
                                                      const float* __restrict__ emb, int nbk, float* __restrict__ out,
                                                      float* __restrict__ lse, int H, int T, float scale) {
    constexpr int F = FB * 64, NFT = F / 16;
    __shared__ float Qs[F * 16];
    __shared__ float emb_lds[64];
    const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
    const int n0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
    const float* Q = qk + ((long)b * 2 * H * F + (long)h * 2 * F) * T;
    const float* K = Q + (long)F * T;
    const float* qb = qkb ? qkb + h * 2 * F : nullptr;
    const float* kb = qkb ? qb + F : nullptr;
    const float* V = a + ((long)b * H + h) * F * T;
    if (bucket && lane < nbk) emb_lds[lane] = emb[lane * H + h];
    stage16(Qs, Q, qb, F, T, n0);
    __syncthreads();
    const int n = n0 + lr;
    floatx4 acc[NFT];
#pragma unroll
    for (int t = 0; t < NFT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    float mrow = -INFINITY, l = 0.f;
    for (int m0 = 0; m0 < T; m0 += 16) {
        // S^T[m][n]: A = K^T (rows m), B = Q (columns n)
        floatx4 s = {0.f, 0.f, 0.f, 0.f};
        const int mk = m0 + lr;
        const bool kin = mk < T;
#pragma unroll 8
        for (int f0 = 0; f0 < F; f0 += 4) {
            const int f = f0 + lg;
            const float av = kin ? K[(long)f * T + mk] + (kb ? kb[f] : 0.f) : 0.f;
            s = mfma(av, Qs[f * 16 + lr], s);
        }
        float x[4], bm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 4 * lg + r;
            x[r] = m < T ? (s[r] + rel_bias(bucket, emb_lds, m, n < T ? n : 0, T)) * scale : -INFINITY;
            bm = fmaxf(bm, x[r]);
        }
        bm = max16x4(bm);                         // finite: key m0 < T is in every tile
        const float mnew = fmaxf(mrow, bm);
        const float alpha = expf(mrow - mnew);    // 0 on the first tile
        float pr[4], ps = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pr[r] = expf(x[r] - mnew);            // exp(-inf) = 0 for masked keys
            ps += pr[r];
        }
        l = l * alpha + sum16x4(ps);
        mrow = mnew;
        // O^T[f][n] = alpha O^T + sum_m V[f][m] P^T[m][n]: step r takes the keys m0 + 4*(l/16) + r
#pragma unroll
        for (int t = 0; t < NFT; ++t) {
            acc[t] *= alpha;
            const float* vr = V + (long)(t * 16 + lr) * T + m0 + 4 * lg;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t] = mfma(m0 + 4 * lg + r < T ? vr[r] : 0.f, pr[r], acc[t]);
        }
    }
    if (n < T) {
        const float il = 1.f / l;
        float* o = out + ((long)b * H + h) * F * T;
#pragma unroll
        for (int t = 0; t < NFT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[(long)(t * 16 + 4 * lg + r) * T + n] = acc[t][r] * il;
        if (lg == 0) lse[((long)b * H + h) * T + n] = mrow + logf(l);
    }
}

// ---------------------------------------------------------------- VJP, query side: dQ
template <int FB>
__global__ __launch_bounds__(64) void attn_vjp_q_kernel(const float* __restrict__ qk, const float* __restrict__ qkb,
                                                        const float* __restrict__ a, const int* __restrict__ bucket,
                                                        const float* __restrict__ emb, int nbk, const float* __restrict__ dout,
                                                        const float* __restrict__ lse, const float* __restrict__ D,
                                                        float* __restrict__ dqk, int H, int T, float scale) {
    constexpr int F = FB * 64, NFT = F / 16;
    __shared__ float Qs[F * 16];
    __shared__ float dOs[F * 16];
    __shared__ float emb_lds[64];
    const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
    const int n0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
    const float* Q = qk + ((long)b * 2 * H * F + (long)h * 2 * F) * T;
    const float* K = Q + (long)F * T;
    const float* qb = qkb ? qkb + h * 2 * F : nullptr;
    const float* kb = qkb ? qb + F : nullptr;
    const float* V = a + ((long)b * H + h) * F * T;
    const float* dO = dout + ((long)b * H + h) * F * T;
    if (bucket && lane < nbk) emb_lds[lane] = emb[lane * H + h];
    stage16(Qs, Q, qb, F, T, n0);
    stage16(dOs, dO, nullptr, F, T, n0);
    __syncthreads();
    const int n = n0 + lr;
    const bool nin = n < T;
    const float L = nin ? lse[((long)b * H + h) * T + n] : 0.f;
    const float Dn = nin ? D[((long)b * H + h) * T + n] : 0.f;
    floatx4 acc[NFT];
#pragma unroll
    for (int t = 0; t < NFT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int m0 = 0; m0 < T; m0 += 16) {
        float ds[4];
        ds_tile_q<F>(K, kb, V, Qs, dOs, bucket, emb_lds, m0, n, nin, L, Dn, T, scale, ds);
        // dQ^T[f][n] += sum_m K[f][m] dS^T[m][n]
#pragma unroll
        for (int t = 0; t < NFT; ++t) {
            const int f = t * 16 + lr;
            const float* kr = K + (long)f * T + m0 + 4 * lg;
            const float kbf = kb ? kb[f] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t] = mfma(m0 + 4 * lg + r < T ? kr[r] + kbf : 0.f, ds[r], acc[t]);
        }
    }
    if (nin) {
        float* o = dqk + ((long)b * 2 * H * F + (long)h * 2 * F) * T;
#pragma unroll
        for (int t = 0; t < NFT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[(long)(t * 16 + 4 * lg + r) * T + n] = acc[t][r] * scale;
    }
}

// ---------------------------------------------------------------- VJP, key side: dK, dV
template <int FB>
__global__ __launch_bounds__(64) void attn_vjp_kv_kernel(const float* __restrict__ qk, const float* __restrict__ qkb,
                                                         const float* __restrict__ a, const int* __restrict__ bucket,
                                                         const float* __restrict__ emb, int nbk, const float* __restrict__ dout,
                                                         const float* __restrict__ lse, const float* __restrict__ D,
                                                         float* __restrict__ dqk, float* __restrict__ dv, int H, int T,
                                                         float scale) {
    constexpr int F = FB * 64, NFT = F / 16;
    __shared__ float Ks[F * 16];
    __shared__ float Vs[F * 16];
    __shared__ float emb_lds[64];
    const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
    const int m0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
    const float* Q = qk + ((long)b * 2 * H * F + (long)h * 2 * F) * T;
    const float* K = Q + (long)F * T;
    const float* qb = qkb ? qkb + h * 2 * F : nullptr;
    const float* kb = qkb ? qb + F : nullptr;
    const float* V = a + ((long)b * H + h) * F * T;
    const float* dO = dout + ((long)b * H + h) * F * T;
    const float* lseh = lse + ((long)b * H + h) * T;
    const float* Dh = D + ((long)b * H + h) * T;
    if (bucket && lane < nbk) emb_lds[lane] = emb[lane * H + h];
    stage16(Ks, K, kb, F, T, m0);
    stage16(Vs, V, nullptr, F, T, m0);
    __syncthreads();
    const int m = m0 + lr;
    const bool kin = m < T;
    floatx4 adk[NFT], adv[NFT];
#pragma unroll
    for (int t = 0; t < NFT; ++t) adk[t] = adv[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < T; n0 += 16) {
        // S[n][m]: A = Q^T (rows n), B = K (columns m); dP likewise with dO and V
        floatx4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
        const int nq = n0 + lr;
        const bool qin = nq < T;
#pragma unroll 8
        for (int f0 = 0; f0 < F; f0 += 4) {
            const int f = f0 + lg;
            const float qv = qin ? Q[(long)f * T + nq] + (qb ? qb[f] : 0.f) : 0.f;
            const float ov = qin ? dO[(long)f * T + nq] : 0.f;
            s = mfma(qv, Ks[f * 16 + lr], s);
            dp = mfma(ov, Vs[f * 16 + lr], dp);
        }
        float pr[4], ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + 4 * lg + r;
            const bool ok = kin && n < T;
            const float pv = ok ? expf((s[r] + rel_bias(bucket, emb_lds, m, n, T)) * scale - lseh[n]) : 0.f;
            pr[r] = pv;
            ds[r] = ok ? pv * (dp[r] - Dh[n]) : 0.f;
        }
        // dV^T[f][m] += sum_n dO[f][n] P[n][m];  dK^T[f][m] += sum_n Q[f][n] dS[n][m]   (step r: queries n0 + 4*(l/16) + r)
#pragma unroll
        for (int t = 0; t < NFT; ++t) {
            const int f = t * 16 + lr;
            const float* orow = dO + (long)f * T + n0 + 4 * lg;
            const float* qrow = Q + (long)f * T + n0 + 4 * lg;
            const float qbf = qb ? qb[f] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool in = n0 + 4 * lg + r < T;
                adv[t] = mfma(in ? orow[r] : 0.f, pr[r], adv[t]);
                adk[t] = mfma(in ? qrow[r] + qbf : 0.f, ds[r], adk[t]);
            }
        }
    }
    if (kin) {
        float* ok_ = dqk + ((long)b * 2 * H * F + (long)h * 2 * F + F) * T;
        float* ov = dv + ((long)b * H + h) * F * T;
#pragma unroll
        for (int t = 0; t < NFT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long o = (long)(t * 16 + 4 * lg + r) * T + m;
                ok_[o] = adk[t][r] * scale;
                ov[o] = adv[t][r];
            }
    }
}

// the fp32 core behind attention_common.h's host bodies: one wave, 16 own rows per workgroup
struct F32Core {
    static constexpr int ROWS = 16;
    template <int FB>
    static int fwd(const char*, dim3 grid, hipStream_t s, const float* qk, const float* qkb, const float* a, const int* bucket,
                   const float* emb, int nbk, float* out, float* lse, int H, int T, float scale) {
        hipLaunchKernelGGL(attn_fwd_kernel<FB>, grid, dim3(64), 0, s, qk, qkb, a, bucket, emb, nbk, out, lse, H, T, scale);
        return BABE_OK;
    }
    template <int FB>
    static int vjp(const char*, dim3 grid, hipStream_t s, const float* qk, const float* qkb, const float* a, const int* bucket,
                   const float* emb, int nbk, const float* dout, const float* lse, const float* D, float* dqk, float* dv, int H,
                   int T, float scale) {
        hipLaunchKernelGGL(attn_vjp_q_kernel<FB>, grid, dim3(64), 0, s, qk, qkb, a, bucket, emb, nbk, dout, lse, D, dqk, H, T, scale);
        BABE_LAUNCH_CHECK();
        hipLaunchKernelGGL(attn_vjp_kv_kernel<FB>, grid, dim3(64), 0, s, qk, qkb, a, bucket, emb, nbk, dout, lse, D, dqk, dv, H, T,
                           scale);
        return BABE_OK;
    }
};

}  // namespace

extern "C" int babe_attn_fwd(const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb,
                             int num_buckets, float* out, float* lse, int B, int H, int F, int T, float scale, void* stream) {
    return attn_fwd_host<F32Core>("attn_fwd", qk, qk_bias, a, bucket, emb, num_buckets, out, lse, B, H, F, T, scale, stream);
}

extern "C" int babe_attn_vjp(const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb,
                             int num_buckets, const float* out, const float* lse, const float* dout, float* D, float* dqk,
                             float* dv, int B, int H, int F, int T, float scale, void* stream) {
    return attn_vjp_host<F32Core>("attn_vjp", qk, qk_bias, a, bucket, emb, num_buckets, out, lse, dout, D, dqk, dv, B, H, F, T, scale,
                                  stream);
}
