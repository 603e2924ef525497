// Tile pieces of the fp32 attention core, shared by its forward / input-VJP (attention.hip) and its table gradient
// (attention_train.hip).  One wave per workgroup; operand layout of v_mfma_f32_16x16x4_f32 in attention.hip's header.
#pragma once
#include "attention_common.h"

__device__ __forceinline__ floatx4 mfma(float a, float b, floatx4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// 16 columns (time steps c0..c0+15) of a [F][T] operand into LDS [F][16], zero past T, plus an optional per-row bias
__device__ __forceinline__ void stage16(float* dst, const float* src, const float* rb, int F, int T, int c0) {
    for (int i = threadIdx.x; i < F * 16; i += 64) {
        const int f = i >> 4, c = c0 + (i & 15);
        dst[i] = c < T ? src[(long)f * T + c] + (rb ? rb[f] : 0.f) : 0.f;
    }
}

__device__ __forceinline__ float rel_bias(const int* bucket, const float* emb_lds, int m, int n, int T) {
    return bucket ? emb_lds[bucket[m - n + T - 1]] : 0.f;
}

// The query side's dS of the key tile at m0, for the lane's query n (nin: n < T; L = lse[n], Dn = D[n]; Qs, dOs the staged
// query columns; K, kb, V the head's key rows, their bias or nullptr, and a[b][h]): S^T[m][n] and dP^T[m][n] over f (A = K^T and V^T, rows m; B = Q and dO, columns n), then
// ds[r] = P o (dP - D) for the keys m0 + 4 * (l / 16) + r, 0 for a masked key or query.  dQ (attn_vjp_q_kernel) and the table
// gradient (attn_demb_kernel) both take their dS from here: the table gradient belongs to exactly the P of the dQ pass.  rel_bias
// tests the bucket pointer for dQ's sake; the table kernel, which always has one, carries that test too (4 scalar branches a tile).
template <int F>
__device__ __forceinline__ void ds_tile_q(const float* K, const float* kb, const float* V, const float* Qs, const float* dOs,
                                          const int* bucket, const float* emb_lds, int m0, int n, bool nin, float L, float Dn, int T,
                                          float scale, float (&ds)[4]) {
    const int lane = threadIdx.x, lr = lane & 15, lg = lane >> 4;
    floatx4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
    const int mk = m0 + lr;
    const bool kin = mk < T;
#pragma unroll 8
    for (int f0 = 0; f0 < F; f0 += 4) {
        const int f = f0 + lg;
        const float kv = kin ? K[(long)f * T + mk] + (kb ? kb[f] : 0.f) : 0.f;
        const float vv = kin ? V[(long)f * T + mk] : 0.f;
        s = mfma(kv, Qs[f * 16 + lr], s);
        dp = mfma(vv, dOs[f * 16 + lr], dp);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + 4 * lg + r;
        const float pv = (m < T && nin) ? expf((s[r] + rel_bias(bucket, emb_lds, m, n, T)) * scale - L) : 0.f;
        ds[r] = pv * (dp[r] - Dn);
    }
}
