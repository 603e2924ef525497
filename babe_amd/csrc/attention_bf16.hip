// Time attention of the CQTDiff+ ResnetBlock on the bf16 MFMA pipe: babe_attn_fwd_bf16 / babe_attn_vjp_bf16, and for training on
// this core babe_attn_param_vjp_bf16 (the relative-position table gradient as a fourth mode of the VJP kernel, so that it belongs
// to exactly the P of the dQ pass; the qk bias gradient is the shared row sum of dqk).  Layouts, mathematics
// and contract are those of attention.hip's header (Q and K rows straight from the qk Conv1d output, bias before scale,
// lse [B][H][T], the VJP writes the gradients w.r.t. the qk rows and w.r.t. V; F a multiple of 64 up to 448, any T >= 1).
//
// Arithmetic (the project's bf16 convention: activations stay fp32 in HBM).  Q + bias, K + bias, V and dO are rounded once, to
// nearest even, on their way into LDS; both products of every pass are bf16 MFMAs with fp32 accumulators; the relative-position
// bias is added to the fp32 score; the online maximum and sum, lse and D stay fp32, the softmax denominator sums the unrounded
// exponentials; P and dS are rounded in registers only as the operand of the second product.
//
// Tiling.  A workgroup of four waves owns 32 rows of its side (queries for the forward and dQ, keys for dK and dV) and walks the
// other side in chunks of 32 time steps.  All 256 threads stage a chunk through LDS with coalesced row reads (consecutive lanes
// read consecutive time steps of one [f] row), as up to two bf16 images:
//   transposed  Xt[time][F + 8]   one 16-byte read is a lane's operand of v_mfma_f32_16x16x32_bf16 over k = f (the score products)
//   natural     Xn[f][32 + 8]     one  8-byte read is a lane's operand of v_mfma_f32_16x16x16_bf16 over k = time (the second product)
// (the 8-element row pads keep both reads off a common bank).  Wave w takes own-row tile rt = w / 2 (16 rows) and streamed tile
// st = w % 2 (16 time steps) of every chunk.  The score tile is formed with the streamed index on the accumulator's rows, so a
// lane's four values are exactly the k slots 4 * (lane / 16) + j of the 16x16x16 product that follows: P and dS never leave their
// registers.  The two waves of an own-row tile each hold a partial over their half of the streamed side - the forward's
// (max, sum, acc), the VJP's acc - and merge them through LDS in the fixed order st = 0, st = 1; a wave that got no tile (T <= 16
// mod 32 on the last chunk, or T <= 16 at all) contributes (-inf, 0, 0).  Every output element is written once, by the st = 0 wave
// of its tile: no atomics, bit-identical run to run and across streams.
// The input-VJP is three launches of one kernel over the recomputed P = exp(S - lse): dQ (own queries; streams K, V), dK (own
// keys; streams Q, dO) and dV (own keys; streams Q, dO).  dK and dV are separate because their streamed images together
// (Qt, dOt, Qn, dOn at F = 448) do not fit the 160 KiB of LDS next to the own side.
// Operand maps (lane l, lr = l % 16, lg = l / 16): 16x16x32  A[lr][8 lg + j], B[8 lg + j][lr], j = 0..7;  16x16x16  A[lr][4 lg + j],
// B[4 lg + j][lr], j = 0..3;  C/D of both: lane l holds D[4 lg + r][lr], r = 0..3.
#include "attention_common.h"
#include "../../include/babe_hip.h"
#include <atomic>
#include <cmath>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int NTH = 256;           // four waves
constexpr int TS = 32;             // time steps per side: own rows of a workgroup, streamed rows of a chunk
constexpr int NPAD = TS + 8;       // row stride of a natural image, bf16 elements (80 bytes)
constexpr int PPAD = 17;           // row stride of the merge image, floats

__device__ __forceinline__ unsigned bf(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }   // to nearest even

__device__ __forceinline__ floatx4 mfma32(const unsigned short* a, const unsigned short* b, floatx4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(a), *reinterpret_cast<const bf16x8*>(b), c, 0,
                                                   0, 0);
}
__device__ __forceinline__ floatx4 mfma16(const unsigned short* a, s16x4 b, floatx4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(*reinterpret_cast<const s16x4*>(a), b, c, 0, 0, 0);
}
__device__ __forceinline__ s16x4 pack4(const float* v) {
    const u32x2 w = {bf(v[0]) | (bf(v[1]) << 16), bf(v[2]) | (bf(v[3]) << 16)};
    return __builtin_bit_cast(s16x4, w);
}

// Time steps c0 .. c0 + 31 of a [F][T] operand (+ an optional per-row bias, added in fp32) as the transposed image dst[32][F + 8]:
// zero past T.  A thread takes one time step of 8 rows; consecutive lanes take consecutive time steps.
template <int F>
__device__ __forceinline__ void stage_t(unsigned short* dst, const float* __restrict__ src, const float* __restrict__ rb, int T,
                                        int c0) {
    for (int i = threadIdx.x; i < TS * (F / 8); i += NTH) {
        const int c = i & (TS - 1), g = i >> 5, col = c0 + c;
        u32x4 w = {0u, 0u, 0u, 0u};
        if (col < T) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = src[(long)(8 * g + j) * T + col] + (rb ? rb[8 * g + j] : 0.f);
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = bf(v[2 * j]) | (bf(v[2 * j + 1]) << 16);
        }
        *reinterpret_cast<u32x4*>(dst + c * (F + 8) + 8 * g) = w;
    }
}

// The same time steps as the natural image dst[F][NPAD].  A thread takes two time steps of one row.
template <int F>
__device__ __forceinline__ void stage_n(unsigned short* dst, const float* __restrict__ src, const float* __restrict__ rb, int T,
                                        int c0) {
    for (int i = threadIdx.x; i < F * (TS / 2); i += NTH) {
        const int p = i & (TS / 2 - 1), f = i >> 4, col = c0 + 2 * p;
        const float b = rb ? rb[f] : 0.f;
        const float v0 = col < T ? src[(long)f * T + col] + b : 0.f;
        const float v1 = col + 1 < T ? src[(long)f * T + col + 1] + b : 0.f;
        *reinterpret_cast<unsigned*>(dst + f * NPAD + 2 * p) = bf(v0) | (bf(v1) << 16);
    }
}

// score tile over k = f: rows = the 16 time steps of image A at `a`, columns = those of image B at `b` (both lane-resolved)
template <int F>
__device__ __forceinline__ floatx4 score_tile(const unsigned short* a, const unsigned short* b) {
    floatx4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};     // two chains: the MFMAs of one do not wait for each other
#pragma unroll
    for (int k = 0; k < F; k += 64) {
        s0 = mfma32(a + k, b + k, s0);
        s1 = mfma32(a + k + 32, b + k + 32, s1);
    }
    return s0 + s1;
}

// table pass (MODE 3 of the VJP kernel): floats of a wave's parked dS tile, and of its array of diagonals.  A key tile at sb
// (a multiple of 16 below T) touches the entries sb .. sb + 30
constexpr int TILE_F = 16 * 17;
__host__ __device__ constexpr int tbl_diag_len(int T) { return ((T + 31) & ~31) + 32; }

// LDS bytes: transposed images, natural images, the bias table, the forward's (max, sum) slots
constexpr int lds_bytes(int F, int nt, int nn) { return nt * TS * (F + 8) * 2 + nn * F * NPAD * 2 + 64 * 4 + 4 * 16 * 2 * 4; }

// ---------------------------------------------------------------- forward.  grid (ceil(T/32), H, B), 256 threads
template <int FB>
__global__ __launch_bounds__(NTH) void attn_fwd_bf16_kernel(const float* __restrict__ qk, const float* __restrict__ qkb,
                                                            const float* __restrict__ a, const int* __restrict__ bucket,
                                                            const float* __restrict__ emb, int nbk, float* __restrict__ out,
                                                            float* __restrict__ lse, int H, int T, float scale) {
    constexpr int F = FB * 64, NFT = F / 16, FP = F + 8;
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned short* Qt = reinterpret_cast<unsigned short*>(smem);      // [32][FP]  own
    unsigned short* Kt = Qt + TS * FP;                                 // [32][FP]  streamed
    unsigned short* Vn = Kt + TS * FP;                                 // [F][NPAD] streamed
    float* emb_lds = reinterpret_cast<float*>(Vn + F * NPAD);          // [64]
    float* ml = emb_lds + 64;                                          // [4][16][2]
    float* part = reinterpret_cast<float*>(Kt);                        // after the loop: [2][F][PPAD] (136 F <= 144 F + 512 bytes)
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4, rt = w >> 1, st = w & 1;
    const int n0 = blockIdx.x * TS, h = blockIdx.y;
    const Head p = head_of(qk, qkb, a, H, F, T);
    if (bucket && tid < nbk) emb_lds[tid] = emb[tid * H + h];
    stage_t<F>(Qt, p.Q, p.qb, T, n0);
    const int n = n0 + 16 * rt + lr;
    const bool qact = n0 + 16 * rt < T, nin = n < T;
    floatx4 acc[NFT];
#pragma unroll
    for (int t = 0; t < NFT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    float mrow = -INFINITY, l = 0.f;
    for (int m0 = 0; m0 < T; m0 += TS) {
        __syncthreads();                                  // the previous chunk has been read
        stage_t<F>(Kt, p.K, p.kb, T, m0);
        stage_n<F>(Vn, p.V, nullptr, T, m0);
        __syncthreads();
        const int mb = m0 + 16 * st;
        if (!qact || mb >= T) continue;                   // wave-uniform
        // S^T[m][n]: A = K^T (rows m), B = Q (columns n)
        const floatx4 s = score_tile<F>(Kt + (16 * st + lr) * FP + 8 * lg, Qt + (16 * rt + lr) * FP + 8 * lg);
        float x[4], bm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = mb + 4 * lg + r;
            const float rb = (bucket && m < T && nin) ? emb_lds[bucket[m - n + T - 1]] : 0.f;
            x[r] = m < T ? (s[r] + rb) * scale : -INFINITY;
            bm = fmaxf(bm, x[r]);
        }
        bm = max16x4(bm);                                 // finite: key mb < T is in the tile
        const float mnew = fmaxf(mrow, bm);
        const float alpha = expf(mrow - mnew);            // 0 on the wave's first tile
        float pr[4], ps = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pr[r] = expf(x[r] - mnew);                    // exp(-inf) = 0 for masked keys
            ps += pr[r];
        }
        l = l * alpha + sum16x4(ps);                      // the unrounded exponentials
        mrow = mnew;
        // O^T[f][n] = alpha O^T + sum_m V[f][m] P^T[m][n]: k slot 4 lg + j is the key mb + 4 lg + j
        const s16x4 pb = pack4(pr);
        const unsigned short* va = Vn + lr * NPAD + 16 * st + 4 * lg;
#pragma unroll
        for (int t = 0; t < NFT; ++t) {
            acc[t] *= alpha;
            acc[t] = mfma16(va + t * 16 * NPAD, pb, acc[t]);
        }
    }
    // merge the two key halves of every query tile, st = 0 then st = 1
    __syncthreads();
    if (lg == 0) {
        ml[(w * 16 + lr) * 2] = mrow;
        ml[(w * 16 + lr) * 2 + 1] = l;
    }
    __syncthreads();
    const float mo = ml[((w ^ 1) * 16 + lr) * 2], lo = ml[((w ^ 1) * 16 + lr) * 2 + 1];
    const float M = fmaxf(mrow, mo);
    const float cs = mrow == -INFINITY ? 0.f : expf(mrow - M), co = mo == -INFINITY ? 0.f : expf(mo - M);
    float* pt = part + (long)rt * F * PPAD + lr;
    if (st == 1) {
#pragma unroll
        for (int t = 0; t < NFT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) pt[(t * 16 + 4 * lg + r) * PPAD] = acc[t][r] * cs;
    }
    __syncthreads();
    if (st == 0 && nin) {
        const float L = l * cs + lo * co, il = 1.f / L;
        float* o = out + p.hb * F * T;
#pragma unroll
        for (int t = 0; t < NFT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = t * 16 + 4 * lg + r;
                o[(long)f * T + n] = (acc[t][r] * cs + pt[f * PPAD]) * il;
            }
        if (lg == 0) lse[p.hb * T + n] = M + logf(L);
    }
}

// ---------------------------------------------------------------- input-VJP.  grid (ceil(T/32), H, B), 256 threads
// MODE 0: dQ (own = queries; streamed K, V);  1: dK (own = keys; streamed Q, dO);  2: dV (own = keys; streamed Q, dO);
// 3: the relative-position table gradient (babe_attn_param_vjp_bf16): the dQ pass up to its fp32 dS - the same images, the same
// score_tile calls, the same exponential - without the second product and its sn image.  Every wave parks its 16 x 16 dS tile in
// LDS, one lane per diagonal of the tile adds its sum (ascending query) into the wave's LDS array of diagonals, key chunks in
// ascending order; at the end lane k of the st = 0 wave adds the diagonals of bucket k in ascending offset, each as (st = 0) +
// (st = 1), and writes the 16-query tile's partial to tpart [B][H][ceil(T/16)][nbk]; demb_sum_kernel adds the query tiles in order.
// own1/own2 and s1/s2 are the transposed images of the two score products (S: s1 x own1, dP: s2 x own2; dV has no dP), sn the
// natural image of the last product's A operand: acc^T[f][own] += sum_streamed sn[f][streamed] * val[streamed][own], with
// val = dS (dQ, dK) or P (dV).
template <int FB, int MODE>
__global__ __launch_bounds__(NTH) void attn_vjp_bf16_kernel(const float* __restrict__ qk, const float* __restrict__ qkb,
                                                            const float* __restrict__ a, const int* __restrict__ bucket,
                                                            const float* __restrict__ emb, int nbk, const float* __restrict__ dout,
                                                            const float* __restrict__ lse, const float* __restrict__ D,
                                                            float* __restrict__ dqk, float* __restrict__ dv,
                                                            float* __restrict__ tpart, int H, int T, float scale) {
    constexpr int F = FB * 64, NFT = F / 16, FP = F + 8;
    constexpr bool DP = MODE != 2;                                     // the pass needs dP = dO . V
    constexpr bool TBL = MODE == 3, QOWN = MODE == 0 || MODE == 3;     // table gradient; the own side is the queries
    constexpr int IMG = TS * FP;
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned short* own1 = reinterpret_cast<unsigned short*>(smem);
    unsigned short* own2 = own1 + IMG;                                 // (absent without dP: the images below move up)
    unsigned short* s1 = own1 + (DP ? 2 : 1) * IMG;
    unsigned short* s2 = s1 + IMG;
    unsigned short* sn = s1 + (DP ? 2 : 1) * IMG;                      // [F][NPAD]
    float* emb_lds = reinterpret_cast<float*>(sn + (TBL ? 0 : F * NPAD));      // [64]  (the table pass has no sn)
    float* part = reinterpret_cast<float*>(s1);                        // after the loop: [2][F][PPAD]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, lr = lane & 15, lg = lane >> 4, rt = w >> 1, st = w & 1;
    const int DL = tbl_diag_len(T);
    float* tile = emb_lds + 64 + w * TILE_F;                           // table pass: this wave's dS[m - sb][n - nb], [16][17]
    float* diag = emb_lds + 64 + 4 * TILE_F + w * DL;                  // table pass: entry j = the diagonal m - n = j - 15 - nb
    const int o0 = blockIdx.x * TS, h = blockIdx.y;
    const Head p = head_of(qk, qkb, a, H, F, T);
    const float* dO = dout + p.hb * F * T;
    const float* lseh = lse + p.hb * T;
    const float* Dh = D + p.hb * T;
    if (bucket && tid < nbk) emb_lds[tid] = emb[tid * H + h];
    if (TBL)
        for (int i = tid; i < 4 * DL; i += NTH) emb_lds[64 + 4 * TILE_F + i] = 0.f;
    if (QOWN) {
        stage_t<F>(own1, p.Q, p.qb, T, o0);
        stage_t<F>(own2, dO, nullptr, T, o0);
    } else {
        stage_t<F>(own1, p.K, p.kb, T, o0);
        if (DP) stage_t<F>(own2, p.V, nullptr, T, o0);
    }
    const int oc = o0 + 16 * rt + lr;                                  // this lane's own column: a query (dQ) or a key
    const bool oact = o0 + 16 * rt < T, oin = oc < T;
    const float Lq = (QOWN && oin) ? lseh[oc] : 0.f, Dq = (QOWN && oin) ? Dh[oc] : 0.f;
    floatx4 acc[NFT];
#pragma unroll
    for (int t = 0; t < NFT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < T; c0 += TS) {
        __syncthreads();
        if (QOWN) {
            stage_t<F>(s1, p.K, p.kb, T, c0);
            stage_t<F>(s2, p.V, nullptr, T, c0);
            if (!TBL) stage_n<F>(sn, p.K, p.kb, T, c0);
        } else {
            stage_t<F>(s1, p.Q, p.qb, T, c0);
            if (DP) {
                stage_t<F>(s2, dO, nullptr, T, c0);
                stage_n<F>(sn, p.Q, p.qb, T, c0);
            } else {
                stage_n<F>(sn, dO, nullptr, T, c0);
            }
        }
        __syncthreads();
        const int sb = c0 + 16 * st;
        if (!oact || sb >= T) continue;                   // wave-uniform
        const int ao = (16 * st + lr) * FP + 8 * lg, bo = (16 * rt + lr) * FP + 8 * lg;
        const floatx4 s = score_tile<F>(s1 + ao, own1 + bo);           // rows = streamed, columns = own
        floatx4 dp = {0.f, 0.f, 0.f, 0.f};
        if (DP) dp = score_tile<F>(s2 + ao, own2 + bo);
        float val[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int sr = sb + 4 * lg + r;                            // streamed row: a key (dQ) or a query
            const int m = QOWN ? sr : oc, n = QOWN ? oc : sr;
            const bool ok = sr < T && oin;
            float pv = 0.f, Dn = Dq;
            if (ok) {
                const float rb = bucket ? emb_lds[bucket[m - n + T - 1]] : 0.f;
                pv = expf((s[r] + rb) * scale - (QOWN ? Lq : lseh[n]));
                if (MODE == 1) Dn = Dh[n];
            }
            val[r] = DP ? pv * (dp[r] - Dn) : pv;
        }
        if (TBL) {                                        // the fp32 dS, before it would be rounded for the second product
#pragma unroll
            for (int r = 0; r < 4; ++r) tile[(4 * lg + r) * 17 + lr] = val[r];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // the tile is this wave's own: no workgroup barrier
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            attn_diag_add(tile, diag + sb, lane);
            continue;                                     // (the next chunk's barrier comes before the tile is written again)
        }
        const s16x4 vb = pack4(val);
        const unsigned short* na = sn + lr * NPAD + 16 * st + 4 * lg;
#pragma unroll
        for (int t = 0; t < NFT; ++t) acc[t] = mfma16(na + t * 16 * NPAD, vb, acc[t]);
    }
    // merge the two streamed halves of every own tile, st = 0 then st = 1
    __syncthreads();
    if (TBL) {
        const int nqt = (T + 15) >> 4, qt = 2 * blockIdx.x + rt, nb = o0 + 16 * rt;
        if (st == 0 && lane < nbk && qt < nqt) {
            const float* d1 = diag + DL;                  // the st = 1 wave of this query tile
            float accb = 0.f;
            for (int j = 0; j < DL; ++j)
                if (attn_diag_in_bucket(bucket, j, nb, T, lane)) accb += diag[j] + d1[j];
            tpart[((long)p.hb * nqt + qt) * nbk + lane] = accb * scale;
        }
        return;
    }
    float* pt = part + (long)rt * F * PPAD + lr;
    if (st == 1) {
#pragma unroll
        for (int t = 0; t < NFT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) pt[(t * 16 + 4 * lg + r) * PPAD] = acc[t][r];
    }
    __syncthreads();
    if (st == 0 && oin) {
        float* o = MODE == 2 ? dv + p.hb * F * T : dqk + (p.Q - qk) + (MODE == 1 ? (long)F * T : 0);
        const float c = MODE == 2 ? 1.f : scale;
#pragma unroll
        for (int t = 0; t < NFT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = t * 16 + 4 * lg + r;
                o[(long)f * T + oc] = (acc[t][r] + pt[f * PPAD]) * c;
            }
    }
}

// a kernel's opt-in for `bytes` of dynamic LDS (babe_lds_optin; `done` is the call site's), the failure under the caller's name
int optin(const char* who, std::atomic<unsigned long long>& done, const void* kernel, int bytes) {
    if (babe_lds_optin(done, {kernel}, bytes) == hipSuccess) return BABE_OK;
    babe_set_error("%s: could not reserve the kernel's LDS: %s", who, hipGetErrorString(hipGetLastError()));
    return BABE_ERR_HIP;
}

// the bf16 core behind attention_common.h's host bodies: four waves, 32 own rows per workgroup
struct Bf16Core {
    static constexpr int ROWS = TS;
    static constexpr int TBL_LDS_LIMIT = 160 * 1024;
    // the table pass (MODE 3): two own and two streamed transposed images, the bias table, four parked tiles, four arrays of diagonals
    static long tbl_lds_bytes(int F, int T) { return 4L * TS * (F + 8) * 2 + 64 * 4 + 4L * TILE_F * 4 + 4L * tbl_diag_len(T) * 4; }

    template <int FB>
    static int fwd(const char* who, dim3 grid, hipStream_t s, const float* qk, const float* qkb, const float* a, const int* bucket,
                   const float* emb, int nbk, float* out, float* lse, int H, int T, float scale) {
        constexpr int lds = lds_bytes(FB * 64, 2, 1);
        static std::atomic<unsigned long long> done{0};
        BABE_TRY(optin(who, done, reinterpret_cast<const void*>(&attn_fwd_bf16_kernel<FB>), lds));
        hipLaunchKernelGGL(attn_fwd_bf16_kernel<FB>, grid, dim3(NTH), lds, s, qk, qkb, a, bucket, emb, nbk, out, lse, H, T, scale);
        return BABE_OK;
    }

    template <int FB, int MODE>
    static int vjp_mode(const char* who, dim3 grid, hipStream_t s, const float* qk, const float* qkb, const float* a,
                        const int* bucket, const float* emb, int nbk, const float* dout, const float* lse, const float* D, float* dqk,
                        float* dv, int H, int T, float scale) {
        constexpr int lds = MODE == 2 ? lds_bytes(FB * 64, 2, 1) : lds_bytes(FB * 64, 4, 1);
        static_assert(lds <= 160 * 1024, "the images of one workgroup must fit the CU's LDS");
        static std::atomic<unsigned long long> done{0};
        BABE_TRY(optin(who, done, reinterpret_cast<const void*>(&attn_vjp_bf16_kernel<FB, MODE>), lds));
        hipLaunchKernelGGL((attn_vjp_bf16_kernel<FB, MODE>), grid, dim3(NTH), lds, s, qk, qkb, a, bucket, emb, nbk, dout, lse, D, dqk,
                           dv, nullptr, H, T, scale);
        return BABE_OK;
    }
    template <int FB>
    static int vjp(const char* who, dim3 grid, hipStream_t s, const float* qk, const float* qkb, const float* a, const int* bucket,
                   const float* emb, int nbk, const float* dout, const float* lse, const float* D, float* dqk, float* dv, int H,
                   int T, float scale) {
        BABE_TRY((vjp_mode<FB, 0>(who, grid, s, qk, qkb, a, bucket, emb, nbk, dout, lse, D, dqk, dv, H, T, scale)));
        BABE_LAUNCH_CHECK();
        BABE_TRY((vjp_mode<FB, 1>(who, grid, s, qk, qkb, a, bucket, emb, nbk, dout, lse, D, dqk, dv, H, T, scale)));
        BABE_LAUNCH_CHECK();
        return vjp_mode<FB, 2>(who, grid, s, qk, qkb, a, bucket, emb, nbk, dout, lse, D, dqk, dv, H, T, scale);
    }

    // its LDS grows with T (tbl_lds_bytes, checked by the host body), so the opt-in is for the whole CU
    template <int FB>
    static int tbl(const char* who, dim3 grid, hipStream_t s, const float* qk, const float* qkb, const float* a, const int* bucket,
                   const float* emb, int nbk, const float* dout, const float* lse, const float* D, float* tpart, int H, int T,
                   float scale) {
        static std::atomic<unsigned long long> done{0};
        BABE_TRY(optin(who, done, reinterpret_cast<const void*>(&attn_vjp_bf16_kernel<FB, 3>), TBL_LDS_LIMIT));
        hipLaunchKernelGGL((attn_vjp_bf16_kernel<FB, 3>), grid, dim3(NTH), tbl_lds_bytes(FB * 64, T), s, qk, qkb, a, bucket, emb, nbk,
                           dout, lse, D, nullptr, nullptr, tpart, H, T, scale);
        return BABE_OK;
    }
};

bool aligned4(std::initializer_list<const void*> ps) {
    for (const void* q : ps)
        if (reinterpret_cast<uintptr_t>(q) & 3) return false;
    return true;
}

}  // namespace

extern "C" int babe_attn_fwd_bf16(const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb,
                                  int num_buckets, float* out, float* lse, int B, int H, int F, int T, float scale, void* stream) {
    BABE_CHECK_ARG(aligned4({qk, qk_bias, a, bucket, emb, out, lse}), "attn_fwd_bf16: a pointer is not 4-byte aligned");
    return attn_fwd_host<Bf16Core>("attn_fwd_bf16", qk, qk_bias, a, bucket, emb, num_buckets, out, lse, B, H, F, T, scale, stream);
}

extern "C" int babe_attn_vjp_bf16(const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb,
                                  int num_buckets, const float* out, const float* lse, const float* dout, float* D, float* dqk,
                                  float* dv, int B, int H, int F, int T, float scale, void* stream) {
    BABE_CHECK_ARG(aligned4({qk, qk_bias, a, bucket, emb, out, lse, dout, D, dqk, dv}),
                   "attn_vjp_bf16: a pointer is not 4-byte aligned");
    return attn_vjp_host<Bf16Core>("attn_vjp_bf16", qk, qk_bias, a, bucket, emb, num_buckets, out, lse, dout, D, dqk, dv, B, H, F, T,
                                   scale, stream);
}

extern "C" long babe_attn_param_vjp_bf16_workspace(int B, int H, int T, int num_buckets) {
    return babe_attn_param_vjp_workspace(B, H, T, num_buckets);
}

extern "C" int babe_attn_param_vjp_bf16(const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb,
                                        int num_buckets, const float* out, const float* lse, const float* dout, const float* dqk,
                                        float* ws, float* demb_rows, long demb_bs, float* dqkb_rows, long dqkb_bs, int B, int H,
                                        int F, int T, float scale, void* stream) {
    BABE_CHECK_ARG(aligned4({qk, qk_bias, a, bucket, emb, out, lse, dout, dqk, ws, demb_rows, dqkb_rows}),
                   "attn_param_vjp_bf16: a pointer is not 4-byte aligned");
    return attn_param_vjp_host<Bf16Core>("attn_param_vjp_bf16", qk, qk_bias, a, bucket, emb, num_buckets, out, lse, dout, dqk, ws,
                                         demb_rows, demb_bs, dqkb_rows, dqkb_bs, B, H, F, T, scale, stream);
}
