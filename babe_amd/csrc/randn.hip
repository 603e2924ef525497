// Counter-based Gaussian noise for the sampler: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11; the Random123 constants) -> exact float32 uniforms -> Box-Muller.  One definition per element, independent of grid,
// block and batch composition - element i of clip c, draw k, under seed s:
//     counter = (q & 0xffffffff, q >> 32, c, k), q = i / 4;  key = (s & 0xffffffff, s >> 32);  word = i % 4
//     u1 = ((r >> 9) + 0.5) * 2^-23 in (0, 1),  u2 = (r' >> 9) * 2^-23 in [0, 1)          (r, r' = words (0,1) or (2,3))
//     z  = sqrt(-2 ln u1) * (cospi(2 u2), sinpi(2 u2))                                       |z| <= sqrt(48 ln 2) = 5.77
// logf / sqrtf / sincospif, not the fast intrinsics: sincospif reduces its argument exactly, so the relative error also holds
// next to the zeros of the cosine.  A pure write stream (B n 4 bytes) behind ~100 integer and ~60 float operations per four
// samples: one Philox call per thread and loop trip, one 16-byte store where the row starts on a 16-byte boundary, four dword
// stores where it does not, a bounds-checked tail for n % 4 != 0.
#include "common.h"
#include "../../include/babe_hip.h"

namespace {

__host__ __device__ inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

__device__ __forceinline__ void box_muller(uint32_t r0, uint32_t r1, float& z0, float& z1) {
    const float u1 = ((float)(r0 >> 9) + 0.5f) * 0x1p-23f;        // exact: 23 bits + a half fit the 24-bit significand
    const float u2 = (float)(r1 >> 9) * 0x1p-23f;
    const float rad = sqrtf(-2.f * logf(u1));
    float s, c;
    sincospif(2.f * u2, &s, &c);
    z0 = rad * c;
    z1 = rad * s;
}

// grid (bx, B), grid-stride over the quads of one row.  NORMAL: floats through Box-Muller; otherwise the raw words.
template <bool NORMAL>
__global__ __launch_bounds__(256) void randn_kernel(uint32_t* __restrict__ out, long out_bs, long n, uint32_t key0, uint32_t key1,
                                                    uint32_t clip0, uint32_t draw) {
    uint32_t* row = out + (long)blockIdx.y * out_bs;
    const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;       // wave-uniform: one row per blockIdx.y
    const uint32_t key[2] = {key0, key1};
    const long nq = (n + 3) >> 2;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long)gridDim.x * blockDim.x) {
        const uint32_t ctr[4] = {(uint32_t)q, (uint32_t)((unsigned long)q >> 32), clip0 + blockIdx.y, draw};
        uint32_t w[4];
        philox4x32_10(ctr, key, w);
        if (NORMAL) {
            float z[4];
            box_muller(w[0], w[1], z[0], z[1]);
            box_muller(w[2], w[3], z[2], z[3]);
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = __float_as_uint(z[j]);
        }
        const long i = q << 2;
        if (i + 4 <= n) {
            if (aligned) {
                *reinterpret_cast<uint4*>(row + i) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) row[i + j] = w[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i + j < n) row[i + j] = w[j];
        }
    }
}

int launch(bool normal, void* out, long out_bs, int B, long n, long seed, long clip0, long draw, void* stream, const char* who) {
    BABE_CHECK_ARG(out && B >= 1 && B <= 65535 && n >= 1, "%s: bad arguments", who);
    BABE_CHECK_ARG(B == 1 || out_bs >= n, "%s: row stride %ld below n = %ld", who, out_bs, n);
    BABE_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0, "%s: out is not 4-byte aligned", who);
    BABE_CHECK_ARG(clip0 >= 0 && clip0 + B <= 0x100000000L && draw >= 0 && draw < 0x100000000L,
                   "%s: clip0 = %ld (+ B = %d), draw = %ld outside the 32-bit counter words", who, clip0, B, draw);
    const long nq = (n + 3) >> 2;
    long bx = (nq + 255) / 256;
    const long cap = 2048 / B > 1 ? 2048 / B : 1;              // ~8 workgroups per CU over the whole batch, grid-stride beyond
    if (bx > cap) bx = cap;
    const uint32_t k0 = (uint32_t)((unsigned long)seed & 0xffffffffu), k1 = (uint32_t)((unsigned long)seed >> 32);
    if (normal)
        hipLaunchKernelGGL(randn_kernel<true>, dim3((unsigned)bx, B), dim3(256), 0, (hipStream_t)stream, static_cast<uint32_t*>(out),
                           out_bs, n, k0, k1, (uint32_t)clip0, (uint32_t)draw);
    else
        hipLaunchKernelGGL(randn_kernel<false>, dim3((unsigned)bx, B), dim3(256), 0, (hipStream_t)stream, static_cast<uint32_t*>(out),
                           out_bs, n, k0, k1, (uint32_t)clip0, (uint32_t)draw);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

}  // namespace

extern "C" int babe_philox4x32(const int* ctr, const int* key, int* out) {
    BABE_CHECK_ARG(ctr && key && out, "philox4x32: bad arguments");
    uint32_t c[4], k[2], o[4];
    memcpy(c, ctr, sizeof c);
    memcpy(k, key, sizeof k);
    philox4x32_10(c, k, o);
    memcpy(out, o, sizeof o);
    return BABE_OK;
}

extern "C" int babe_randn(float* out, long out_bs, int B, long n, long seed, long clip0, long draw, void* stream) {
    return launch(true, out, out_bs, B, n, seed, clip0, draw, stream, "randn");
}

extern "C" int babe_rand_bits(int* out, long out_bs, int B, long n, long seed, long clip0, long draw, void* stream) {
    return launch(false, out, out_bs, B, n, seed, clip0, draw, stream, "rand_bits");
}
