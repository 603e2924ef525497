// The tail of a training iteration on gfx950: L2 norm of all gradients, clipping, Adam and the EMA of the weights, over a
// device-resident TABLE of tensors (a network has hundreds: too many for kernel arguments) cut into chunks by a host-side
// builder.  One workgroup per chunk; a chunk never crosses a tensor, so its five base pointers are wave-uniform.
//   babe_grad_sqnorm    partials[c] = sum over chunk c of g^2 (double), then ONE workgroup adds the partials and writes the norm
//   babe_adam_ema_step  reads the norm from device memory (no host synchronisation), p, g, m, v, ema once; writes p, m, v, ema once
// Streaming and HBM-bound: 9 x 4 B per parameter in the step, 4 B in the norm.  A thread moves 16 B per array and iteration,
// five independent loads before the first use, and 94 registers leave 5 waves per SIMD: 1280 threads x 5 x 16 B = 100 KB of
// loads in flight per CU, several times what an HBM miss needs hidden.  Plain stores.
// Arithmetic: the moments are torch.optim.Adam's fp32 operations with the two fused multiply-adds torch's own element-wise
// kernels are compiled to - lerp: fma(1 - beta1, g' - m, m); mul + addcmul: fma(1 - beta2, g' g', beta2 v) - and nothing else
// contracted, so from equal inputs m and v have torch's bits (measured in the trainer test: all of them).  The parameter update
// and the EMA are evaluated in DOUBLE from those fp32 moments and rounded once where they are stored: torch's element-wise passes
// put some six fp32 roundings between m, v and p, and the EMA inherits the error of the p it averages - amplified where
// p - update cancels (measured against a float64 statement: stock tail up to 6.7 eps (|ema| + |p_new|), this kernel with an
// fp32 update the same, with the double update 2.9).  Some 40 fp64 operations per element, under the time its 36 bytes take.
// Order is fixed: the element -> thread map depends on the chunk alone, not on alignment (an entry whose pointers are not all
// 16-byte aligned - a view that starts inside an allocation - takes the same loop with 4-byte accesses), every sum is a double
// in one order (thread's quads ascending, then the tail element, lanes by butterfly, waves in order; the partials strided over
// 256 threads, then the same block sum).  Same inputs, same bits.
#include "common.h"
#include "../../include/babe_hip.h"
#include "prof.h"
#include <climits>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256, NW = NT / 64;

struct StepK {
    double max_norm, step, bc2s, eps, es, e1;
    float b1m, b2, b2m;                     // 1 - beta1, beta2, 1 - beta2: each rounded from double once, as torch's scalars are
};

__device__ __forceinline__ bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The table's pointers come from memory, so the compiler cannot tell their address space and would emit FLAT accesses (which
// also tick the LDS counter); they are global memory by contract.
#define BABE_GLOBAL __attribute__((address_space(1)))
typedef float f4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float ldg(const float* p) { return *(const BABE_GLOBAL float*)p; }
__device__ __forceinline__ void stg(float* p, float x) { *(BABE_GLOBAL float*)p = x; }

template <bool VEC>
__device__ __forceinline__ float4 ld4(const float* p, int q) {
    p += 4 * (long)q;
    if (VEC) {
        const f4_t x = *(const BABE_GLOBAL f4_t*)p;
        return make_float4(x.x, x.y, x.z, x.w);
    }
    return make_float4(ldg(p), ldg(p + 1), ldg(p + 2), ldg(p + 3));
}
template <bool VEC>
__device__ __forceinline__ void st4(float* p, int q, float4 x) {
    p += 4 * (long)q;
    if (VEC) {
        f4_t y = {x.x, x.y, x.z, x.w};
        *(BABE_GLOBAL f4_t*)p = y;
    } else {
        stg(p, x.x), stg(p + 1, x.y), stg(p + 2, x.z), stg(p + 3, x.w);
    }
}

__device__ __forceinline__ void sq_add(double& acc, float g) { acc += (double)g * (double)g; }

template <bool VEC>
__device__ __forceinline__ double sq_quads(const float* g, int nq) {
    double acc = 0.0;
#pragma unroll 4
    for (int q = threadIdx.x; q < nq; q += NT) {
        const float4 x = ld4<VEC>(g, q);
        sq_add(acc, x.x), sq_add(acc, x.y), sq_add(acc, x.z), sq_add(acc, x.w);
    }
    return acc;
}

// grid (nchunks), 256 threads
__global__ __launch_bounds__(NT) void grad_sqnorm_kernel(const babe_opt_tensor* __restrict__ table,
                                                         const babe_opt_chunk* __restrict__ chunks, double* __restrict__ partials) {
    __shared__ double sh[NW];
    const babe_opt_chunk c = chunks[blockIdx.x];
    const float* g = table[c.t].g;
    double acc = 0.0;
    if (g) {
        g += c.off;
        const int nq = c.n >> 2;
        acc = al16(g) ? sq_quads<true>(g, nq) : sq_quads<false>(g, nq);
        if ((int)threadIdx.x < (c.n & 3)) sq_add(acc, ldg(g + 4 * nq + threadIdx.x));
    }
    acc = block_sum<NW>(acc, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// one workgroup: thread t adds partials t, t + 256, ... in ascending order, then the block sum
__global__ __launch_bounds__(NT) void grad_norm_finish_kernel(const double* __restrict__ partials, long n,
                                                              double* __restrict__ norm_out) {
    __shared__ double sh[NW];
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += NT) acc += partials[i];
    acc = block_sum<NW>(acc, sh);
    if (threadIdx.x == 0) norm_out[0] = sqrt(acc);
}

// torch.optim.Adam's update.  Moments in fp32, as torch's kernels compute them: exp_avg.lerp_(g, 1 - beta1) (weight below 0.5:
// a + w (b - a), one fma), exp_avg_sq.mul_(beta2).addcmul_(g, g, value = 1 - beta2) (a + value (b c), one fma).  Update in double
// from the stored moments: denom = exp_avg_sq.sqrt() / bc2_sqrt + eps, param.addcdiv_(exp_avg, denom, value = -step_size).
// All-zero g, m, v: 0 / eps = 0 and p keeps its bits.
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, float coef, const StepK& k) {
    g = coef * g;
    m = fmaf(k.b1m, g - m, m);
    v = fmaf(k.b2m, g * g, k.b2 * v);
    p = (float)((double)p - k.step * ((double)m / (sqrt((double)v) / k.bc2s + k.eps)));
}
// p: the NEW parameter as stored - the EMA averages the weights the network has
__device__ __forceinline__ float ema1(float e, float p, const StepK& k) { return (float)((double)e * k.es + (double)p * k.e1); }

template <bool VEC, bool HAS_G, bool HAS_E>
__device__ __forceinline__ void step_chunk(const babe_opt_tensor& t, long off, int n, float coef, const StepK& k) {
    float* p = t.p + off;
    const float* g = HAS_G ? t.g + off : nullptr;
    float* m = HAS_G ? t.m + off : nullptr;
    float* v = HAS_G ? t.v + off : nullptr;
    float* e = HAS_E ? t.ema + off : nullptr;
    const int nq = n >> 2;
#pragma unroll 2
    for (int q = threadIdx.x; q < nq; q += NT) {
        float4 P = ld4<VEC>(p, q), G, M, V, E;
        if (HAS_G) G = ld4<VEC>(g, q), M = ld4<VEC>(m, q), V = ld4<VEC>(v, q);
        if (HAS_E) E = ld4<VEC>(e, q);
        if (HAS_G) {
            adam1(P.x, G.x, M.x, V.x, coef, k);
            adam1(P.y, G.y, M.y, V.y, coef, k);
            adam1(P.z, G.z, M.z, V.z, coef, k);
            adam1(P.w, G.w, M.w, V.w, coef, k);
            st4<VEC>(p, q, P), st4<VEC>(m, q, M), st4<VEC>(v, q, V);
        }
        if (HAS_E) {
            E.x = ema1(E.x, P.x, k), E.y = ema1(E.y, P.y, k), E.z = ema1(E.z, P.z, k), E.w = ema1(E.w, P.w, k);
            st4<VEC>(e, q, E);
        }
    }
    if ((int)threadIdx.x < (n & 3)) {
        const int i = 4 * nq + threadIdx.x;
        float P = ldg(p + i);
        if (HAS_G) {
            float M = ldg(m + i), V = ldg(v + i);
            adam1(P, ldg(g + i), M, V, coef, k);
            stg(p + i, P), stg(m + i, M), stg(v + i, V);
        }
        if (HAS_E) stg(e + i, ema1(ldg(e + i), P, k));
    }
}

template <bool HAS_G, bool HAS_E>
__device__ __forceinline__ void step_entry(const babe_opt_tensor& t, long off, int n, float coef, const StepK& k) {
    bool vec = al16(t.p + off);
    if (HAS_G) vec = vec && al16(t.g + off) && al16(t.m + off) && al16(t.v + off);
    if (HAS_E) vec = vec && al16(t.ema + off);
    if (vec)
        step_chunk<true, HAS_G, HAS_E>(t, off, n, coef, k);
    else
        step_chunk<false, HAS_G, HAS_E>(t, off, n, coef, k);
}

// grid (nchunks), 256 threads.  Every branch on the entry's pointers is workgroup-uniform.
__global__ __launch_bounds__(NT) void adam_ema_step_kernel(const babe_opt_tensor* __restrict__ table,
                                                           const babe_opt_chunk* __restrict__ chunks,
                                                           const double* __restrict__ norm, StepK k) {
    const babe_opt_chunk c = chunks[blockIdx.x];
    const babe_opt_tensor t = table[c.t];
    float coef = 1.f;
    if (norm) {
        // clip_grad_norm_: max_norm / (norm + 1e-6) clamped to 1.  `x > 1 ? 1 : x` keeps a NaN norm a NaN coefficient, as
        // torch.clamp does; an infinite norm gives 0, and 0 * inf = NaN in the gradient that caused it
        const double x = k.max_norm / (norm[0] + 1e-6);
        coef = (float)(x > 1.0 ? 1.0 : x);
    }
    if (t.g) {
        if (t.ema)
            step_entry<true, true>(t, c.off, c.n, coef, k);
        else
            step_entry<true, false>(t, c.off, c.n, coef, k);
    } else if (t.ema) {
        step_entry<false, true>(t, c.off, c.n, coef, k);
    }
}

}  // namespace

extern "C" long babe_opt_chunks(const long* n, long nt, long chunk, babe_opt_chunk* out, long cap) {
    if (!n || nt <= 0 || nt > INT_MAX) {
        babe_set_error("opt_chunks: bad arguments (n=%p, nt=%ld)", (const void*)n, nt);
        return -1;
    }
    if (chunk <= 0 || (chunk & 3) || chunk > (1L << 30)) {
        babe_set_error("opt_chunks: chunk=%ld must be a positive multiple of 4, at most 2^30", chunk);
        return -1;
    }
    long count = 0;
    for (long t = 0; t < nt; ++t) {
        if (n[t] <= 0) {
            babe_set_error("opt_chunks: tensor %ld has n=%ld elements", t, n[t]);
            return -1;
        }
        for (long off = 0; off < n[t]; off += chunk, ++count) {
            if (!out) continue;
            if (count >= cap) {
                babe_set_error("opt_chunks: more than cap=%ld chunks", cap);
                return -1;
            }
            out[count].off = off;
            out[count].t = (int)t;
            out[count].n = (int)(n[t] - off < chunk ? n[t] - off : chunk);
        }
    }
    if (count > INT_MAX) {
        babe_set_error("opt_chunks: %ld chunks exceed one launch", count);
        return -1;
    }
    return count;
}

extern "C" int babe_grad_sqnorm(const babe_opt_tensor* table, const babe_opt_chunk* chunks, long nchunks, double* partials,
                                double* norm_out, void* stream) {
    BABE_CHECK_ARG(table && chunks && partials && norm_out, "grad_sqnorm: null pointer");
    BABE_CHECK_ARG(nchunks > 0 && nchunks <= INT_MAX, "grad_sqnorm: nchunks=%ld (1 .. 2^31 - 1)", nchunks);
    BabeProfScope prof(BABE_SLOT_AXPBY, 0.0, 0.0, 0, stream);
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)nchunks), dim3(NT), 0, (hipStream_t)stream, table, chunks, partials);
    BABE_LAUNCH_CHECK();
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, partials, nchunks, norm_out);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" int babe_adam_ema_step(const babe_opt_tensor* table, const babe_opt_chunk* chunks, long nchunks, const double* norm,
                                  double max_norm, double lr_over_bc1, double bc2_sqrt, double beta1, double beta2, double eps,
                                  double ema_s, double ema_1ms, void* stream) {
    BABE_CHECK_ARG(table && chunks, "adam_ema_step: null table");
    BABE_CHECK_ARG(nchunks > 0 && nchunks <= INT_MAX, "adam_ema_step: nchunks=%ld (1 .. 2^31 - 1)", nchunks);
    BABE_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adam_ema_step: betas (%g, %g) outside [0, 1)", beta1,
                   beta2);                                                              // (a NaN fails this and every check below)
    BABE_CHECK_ARG(eps > 0.0, "adam_ema_step: eps=%g must be positive", eps);
    BABE_CHECK_ARG(lr_over_bc1 >= 0.0, "adam_ema_step: negative learning rate (lr / bc1 = %g)", lr_over_bc1);
    BABE_CHECK_ARG(bc2_sqrt > 0.0, "adam_ema_step: bc2_sqrt=%g must be positive", bc2_sqrt);
    BABE_CHECK_ARG(!norm || max_norm >= 0.0, "adam_ema_step: max_norm=%g must not be negative", max_norm);
    StepK k;
    k.max_norm = max_norm, k.step = lr_over_bc1, k.bc2s = bc2_sqrt, k.eps = eps, k.es = ema_s, k.e1 = ema_1ms;
    k.b1m = (float)(1.0 - beta1), k.b2 = (float)beta2, k.b2m = (float)(1.0 - beta2);
    BabeProfScope prof(BABE_SLOT_AXPBY, 0.0, 0.0, 0, stream);
    hipLaunchKernelGGL(adam_ema_step_kernel, dim3((unsigned)nchunks), dim3(NT), 0, (hipStream_t)stream, table, chunks, norm, k);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}
