// Known degradations of BlindSampler.predict_bwe beyond the FIR: 'cheby1' / 'biquad' (torchaudio.functional.lfilter /
// biquad), 'decimate' (x[..., 0:-1:factor]) and the adjoint of 'resample' (the sinc resampler of resample_sinc.hip), each with
// its adjoint for the guidance VJP (the reference's testing/blind_bwe_sampler.py:219-230).
//
// IIR filter, lfilter semantics: w[n] = sum_{k=0..N} b_k x[n-k], y[n] = w[n] - sum_{k=1..N} a_k y[n-k], zero initial state,
// coefficients normalised by a_0 on the host (fp32, as lfilter), optional clamp of the output to [-1, 1].  The operator is causal
// LTI, so its adjoint is reverse(lfilter(reverse(g))): ONE kernel family, the direction flag only maps sample n to L-1-n.  With
// clamping the forward leaves the mask |y| <= 1 (torch's clamp gradient: 1 on the closed interval) and the adjoint zeroes its
// seed outside it first.
//
// Parallel over time, exact (nothing truncated), state in fp64.  Chunks of C samples (C a multiple of N+1, ~256):
//   1. iir_chunk_kernel<N, false>: every chunk's zero-state response, keeping its last N outputs E[c]; N extra threads run the
//      homogeneous recursion from the unit states for C samples: the columns of P = M^C (M = companion matrix).
//   2. iir_carry_kernel: incoming states S[c+1] = P S[c] + E[c], S[0] = 0, as a two-level scan per row: 64 superchunks of G
//      chunks each carry their own zero-state end F[k] (in parallel), one sequential pass carries the superchunk states with
//      Q = P^G, and each superchunk then replays its G chunks from its incoming state.  3 sweeps of ~sqrt(nc) steps instead of nc.
//   3. iir_chunk_kernel<N, true>: every chunk re-runs its recursion from S[c] and writes y.
// One thread per chunk; the recursion's history lives in registers as circular buffers of N+1 slots whose indices are
// compile-time (the sample loop is unrolled by N+1 and chunks start at multiples of N+1).  No atomics: deterministic, and every
// row is computed independently of the batch size.
#include "common.h"
#include "../../include/babe_hip.h"
#include "prof.h"

namespace {

constexpr int IIR_MAXN = 16;
constexpr int IIR_CHUNK = 256;
constexpr int IIR_SLOTS = 64;

inline long iir_chunk_len(int N) { return (long)(N + 1) * (IIR_CHUNK / (N + 1)); }

struct IirArgs {
    const float* x; long x_bs;
    float* y; long y_bs;
    unsigned char* mask; long mask_bs;
    const float* b; const float* a;
    double* E; double* S; double* P;
    long L, C, nc;
    int B, adjoint, clamp;
};

// MODE_OUT: phase 3 (from S[c], write y); otherwise phase 1 (zero state, write E[c]; the N threads past the chunks compute P)
template <int N, bool MODE_OUT>
__global__ __launch_bounds__(64) void iir_chunk_kernel(IirArgs p) {
    constexpr int M = N + 1;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nchunks = (long)p.B * p.nc;
    int col = -1;                                  // phase 1 only: column of P this thread computes
    if (t >= nchunks) {
        if (MODE_OUT || t >= nchunks + N) return;
        col = (int)(t - nchunks);
    }
    double bc[M], ac[M];
#pragma unroll
    for (int k = 0; k < M; ++k) {
        bc[k] = (double)p.b[k];
        ac[k] = (double)p.a[k];
    }
    const int row = col >= 0 ? 0 : (int)(t / p.nc);
    const long c = col >= 0 ? 0 : t - (long)row * p.nc;
    const long cs = c * p.C;
    const long ce = col >= 0 ? p.C : (cs + p.C < p.L ? cs + p.C : p.L);
    const float* xb = p.x + (long)row * p.x_bs;
    float* yb = p.y + (long)row * p.y_bs;
    unsigned char* mb = p.mask ? p.mask + (long)row * p.mask_bs : nullptr;
    const bool has_in = col < 0;
    const bool mask_in = p.adjoint && p.clamp;
    auto ld = [&](long n) -> double {
        const long q = p.adjoint ? p.L - 1 - n : n;
        float v = xb[q];
        if (mask_in && !mb[q]) v = 0.f;
        return (double)v;
    };
    const double* Sin = MODE_OUT ? p.S + ((long)row * p.nc + c) * IIR_MAXN : nullptr;
    double xh[M], yh[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {                  // slot j holds position cs - M + j, i.e. state index i = M - 1 - j
        const long q = cs - M + j;
        xh[j] = (has_in && q >= 0) ? ld(q) : 0.0;
        const int i = M - 1 - j;
        double s = 0.0;
        if (i < N) {
            if (MODE_OUT) s = Sin[i];
            else if (col >= 0) s = (i == col) ? 1.0 : 0.0;
        }
        yh[j] = s;
    }
    for (long n0 = cs; n0 < ce; n0 += M) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const long n = n0 + j;
            if (n < ce) {
                const double xv = has_in ? ld(n) : 0.0;
                xh[j] = xv;
                double acc = bc[0] * xv;
#pragma unroll
                for (int k = 1; k <= N; ++k) acc = fma(bc[k], xh[(j - k + M) % M], acc);
#pragma unroll
                for (int k = N; k >= 1; --k) acc = fma(-ac[k], yh[(j - k + M) % M], acc);   // a_1 y[n-1] last: 1 FMA on the chain
                yh[j] = acc;
                if (MODE_OUT) {
                    const long q = p.adjoint ? p.L - 1 - n : n;
                    float v = (float)acc;
                    if (p.clamp && !p.adjoint) {
                        const bool in = v >= -1.f && v <= 1.f;
                        if (mb) mb[q] = in ? 1 : 0;
                        v = fminf(fmaxf(v, -1.f), 1.f);
                    }
                    yb[q] = v;
                }
            }
        }
    }
    if (!MODE_OUT) {
        // end state: position ce - 1 - i sits in slot (ce - 1 - i - cs) mod M (cs is a multiple of M)
        const int last = (int)((ce - 1 - cs) % M);
        double* dst = col >= 0 ? nullptr : p.E + ((long)row * p.nc + c) * IIR_MAXN;
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int i = (last - j + M) % M;      // slot j holds state index i
            if (i < N) {
                if (col >= 0) p.P[i * IIR_MAXN + col] = yh[j];
                else dst[i] = yh[j];
            }
        }
    }
}

// one workgroup per row: S[c] for every chunk from E and P (see the top of the file)
__global__ __launch_bounds__(1024) void iir_carry_kernel(const double* __restrict__ E, const double* __restrict__ P,
                                                         double* __restrict__ S, int N, long nc) {
    __shared__ double sP[IIR_MAXN][IIR_MAXN], sQ[IIR_MAXN][IIR_MAXN], sF[IIR_SLOTS][IIR_MAXN], sT[IIR_SLOTS][IIR_MAXN];
    const int t = threadIdx.x, k = t >> 4, i = t & 15;
    const long nsc = nc < IIR_SLOTS ? nc : IIR_SLOTS;
    const long G = (nc + nsc - 1) / nsc;
    const double* Eb = E + (long)blockIdx.x * nc * IIR_MAXN;
    double* Sb = S + (long)blockIdx.x * nc * IIR_MAXN;
    if (t < IIR_MAXN * IIR_MAXN) {
        const int r = t >> 4, cc = t & 15;
        const double v = (r < N && cc < N) ? P[r * IIR_MAXN + cc] : 0.0;
        sP[r][cc] = v;
        sQ[r][cc] = v;
    }
    __syncthreads();
    for (long g = 1; g < G && nsc > 1; ++g) {      // Q = P^G (needed only to carry from one superchunk to the next)
        double v = 0.0;
        if (t < IIR_MAXN * IIR_MAXN) {
            const int r = t >> 4, cc = t & 15;
            for (int l = 0; l < N; ++l) v = fma(sQ[r][l], sP[l][cc], v);
        }
        __syncthreads();
        if (t < IIR_MAXN * IIR_MAXN) sQ[t >> 4][t & 15] = v;
        __syncthreads();
    }
    const bool active = k < nsc;
    // (a) zero-state end of every superchunk
    double s = 0.0;
    if (active) {
        for (long j = 0; j < G; ++j) {
            const long c = k * G + j;
            const bool ok = c < nc;
            double ns = (ok && i < N) ? Eb[c * IIR_MAXN + i] : 0.0;
            for (int l = 0; l < N; ++l) ns = fma(sP[i][l], __shfl(s, l, 16), ns);
            if (ok) s = ns;
        }
        sF[k][i] = s;
    }
    __syncthreads();
    // (b) incoming state of every superchunk, sequentially
    if (t < 16) {
        double s2 = 0.0;
        for (long kk = 0; kk < nsc; ++kk) {
            sT[kk][i] = s2;
            double ns = sF[kk][i];
            for (int l = 0; l < N; ++l) ns = fma(sQ[i][l], __shfl(s2, l, 16), ns);
            s2 = ns;
        }
    }
    __syncthreads();
    // (c) incoming state of every chunk
    if (active) {
        s = sT[k][i];
        for (long j = 0; j < G; ++j) {
            const long c = k * G + j;
            const bool ok = c < nc;
            if (ok && i < N) Sb[c * IIR_MAXN + i] = s;
            double ns = (ok && i < N) ? Eb[c * IIR_MAXN + i] : 0.0;
            for (int l = 0; l < N; ++l) ns = fma(sP[i][l], __shfl(s, l, 16), ns);
            if (ok) s = ns;
        }
    }
}

template <int N>
hipError_t iir_launch(const IirArgs& a, hipStream_t st) {
    const long threads1 = (long)a.B * a.nc + N;
    hipLaunchKernelGGL((iir_chunk_kernel<N, false>), dim3((unsigned)((threads1 + 63) / 64)), dim3(64), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(iir_carry_kernel, dim3(a.B), dim3(1024), 0, st, a.E, a.P, a.S, N, a.nc);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long threads3 = (long)a.B * a.nc;
    hipLaunchKernelGGL((iir_chunk_kernel<N, true>), dim3((unsigned)((threads3 + 63) / 64)), dim3(64), 0, st, a);
    return hipGetLastError();
}

using IirLaunch = hipError_t (*)(const IirArgs&, hipStream_t);
const IirLaunch kIirLaunch[IIR_MAXN] = {iir_launch<1>,  iir_launch<2>,  iir_launch<3>,  iir_launch<4>,
                                        iir_launch<5>,  iir_launch<6>,  iir_launch<7>,  iir_launch<8>,
                                        iir_launch<9>,  iir_launch<10>, iir_launch<11>, iir_launch<12>,
                                        iir_launch<13>, iir_launch<14>, iir_launch<15>, iir_launch<16>};

__global__ __launch_bounds__(256) void decimate_kernel(const float* __restrict__ in, long in_bs, float* __restrict__ out,
                                                       long out_bs, long L_full, long L_dec, int factor, int adjoint) {
    const int b = blockIdx.y;
    const long n_out = adjoint ? L_full : L_dec;
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < n_out; m += (long)gridDim.x * blockDim.x) {
        float v;
        if (adjoint) {                              // zero-stuffing scatter written as a gather
            const long q = m / factor;
            v = (m - q * factor == 0 && q < L_dec) ? in[(long)b * in_bs + q] : 0.f;
        } else {
            v = in[(long)b * in_bs + m * factor];
        }
        out[(long)b * out_bs + m] = v;
    }
}

inline __device__ long floordiv(long a, long b) {
    const long q = a / b;
    return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}

// transpose of resample_sinc_kernel: gx[p] = sum over the (output m = i new + j, tap k) with i orig - width + k = p of
// kern[j][k] g[m]; a gather per input sample (phases j ascending, then i ascending)
__global__ __launch_bounds__(256) void resample_sinc_adjoint_kernel(const float* __restrict__ g, long g_bs, float* __restrict__ out,
                                                                    long out_bs, long L_in, long L_out,
                                                                    const float* __restrict__ kern, const int* __restrict__ krange,
                                                                    int orig, int new_, int width, int taps) {
    const int b = blockIdx.y;
    const float* gb = g + (long)b * g_bs;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < L_in; p += (long)gridDim.x * blockDim.x) {
        float acc = 0.f;
        for (int j = 0; j < new_; ++j) {
            const int k0 = krange[2 * j], k1 = krange[2 * j + 1];
            if (k0 >= k1 || L_out - 1 - j < 0) continue;
            long i0 = floordiv(p + width - k1, orig) + 1;
            long i1 = floordiv(p + width - k0, orig);
            const long imax = (L_out - 1 - j) / new_;
            if (i0 < 0) i0 = 0;
            if (i1 > imax) i1 = imax;
            const float* kj = kern + (long)j * taps;
            for (long i = i0; i <= i1; ++i) acc = fmaf(kj[p + width - i * orig], gb[i * new_ + j], acc);
        }
        out[(long)b * out_bs + p] = acc;
    }
}

}  // namespace

extern "C" long babe_iir_workspace(int B, long L, int order) {
    if (B <= 0 || L <= 0 || order < 1 || order > IIR_MAXN) return -1;
    const long nc = (L + iir_chunk_len(order) - 1) / iir_chunk_len(order);
    return 8L * (2L * B * nc * IIR_MAXN + IIR_MAXN * IIR_MAXN);
}

extern "C" int babe_iir_filter(const float* x, long x_bs, float* y, long y_bs, int B, long L, const float* b, const float* a,
                               int order, int clamp, int adjoint, unsigned char* mask, long mask_bs, void* workspace,
                               long workspace_bytes, void* stream) {
    BABE_CHECK_ARG(x && y && b && a && workspace && B > 0 && L > 0, "iir_filter: bad arguments");
    BABE_CHECK_ARG(order >= 1 && order <= IIR_MAXN, "iir_filter: order %d outside 1..%d", order, IIR_MAXN);
    BABE_CHECK_ARG(x != y, "iir_filter: in-place filtering is not supported");
    BABE_CHECK_ARG(x_bs >= L && y_bs >= L, "iir_filter: row strides %ld / %ld below L = %ld", x_bs, y_bs, L);
    BABE_CHECK_ARG(!(clamp && adjoint) || mask, "iir_filter: the clamped adjoint needs the forward's mask");
    BABE_CHECK_ARG(!mask || mask_bs >= L, "iir_filter: mask row stride %ld below L = %ld", mask_bs, L);
    const long need = babe_iir_workspace(B, L, order);
    BABE_CHECK_ARG(workspace_bytes >= need, "iir_filter: workspace %ld bytes, need %ld", workspace_bytes, need);
    IirArgs p;
    p.x = x; p.x_bs = x_bs; p.y = y; p.y_bs = y_bs;
    p.mask = clamp ? mask : nullptr; p.mask_bs = mask_bs;
    p.b = b; p.a = a;
    p.C = iir_chunk_len(order);
    p.nc = (L + p.C - 1) / p.C;
    p.L = L; p.B = B; p.adjoint = adjoint ? 1 : 0; p.clamp = clamp ? 1 : 0;
    double* ws = (double*)workspace;
    p.P = ws;
    p.E = ws + IIR_MAXN * IIR_MAXN;
    p.S = p.E + (long)B * p.nc * IIR_MAXN;
    BabeProfScope prof(BABE_SLOT_SAMPLER, 8.0 * B * (double)L, 2.0 * (2 * order + 1) * B * (double)L, 0, stream);
    const hipError_t e = kIirLaunch[order - 1](p, (hipStream_t)stream);
    if (e != hipSuccess) {
        babe_set_error("iir_filter: HIP launch error: %s", hipGetErrorString(e));
        return BABE_ERR_HIP;
    }
    return BABE_OK;
}

extern "C" int babe_decimate(const float* in, long in_bs, float* out, long out_bs, int B, long L_full, long L_dec, int factor,
                             int adjoint, void* stream) {
    BABE_CHECK_ARG(in && out && B > 0 && L_full > 0 && L_dec > 0 && factor >= 1, "decimate: bad arguments");
    BABE_CHECK_ARG((L_dec - 1) * (long)factor < L_full, "decimate: %ld samples at stride %d reach beyond L = %ld", L_dec, factor,
                   L_full);
    BabeProfScope prof(BABE_SLOT_SAMPLER, 4.0 * B * (double)(L_dec + (adjoint ? L_full : L_dec)), 0, 0, stream);
    const long n_out = adjoint ? L_full : L_dec;
    long bx = (n_out + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(decimate_kernel, dim3((unsigned)bx, B), dim3(256), 0, (hipStream_t)stream, in, in_bs, out, out_bs, L_full,
                       L_dec, factor, adjoint ? 1 : 0);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" int babe_resample_sinc_adjoint(const float* g, long g_bs, float* out, long out_bs, int B, long L_in, long L_out,
                                          const float* kernel, const int* krange, int orig, int new_, int width, void* stream) {
    BABE_CHECK_ARG(g && out && kernel && krange && B > 0 && L_in > 0 && L_out > 0, "resample_sinc_adjoint: bad arguments");
    BABE_CHECK_ARG(orig > 0 && new_ > 0 && width > 0, "resample_sinc_adjoint: orig=%d new=%d width=%d", orig, new_, width);
    BABE_CHECK_ARG(L_out <= (L_in / orig + 1) * (long)new_, "resample_sinc_adjoint: L_out %ld beyond the %ld samples the transform yields",
                   L_out, (L_in / orig + 1) * (long)new_);
    const int taps = 2 * width + orig;
    BabeProfScope prof(BABE_SLOT_SAMPLER, 4.0 * B * (double)(L_in + L_out), 0, 0, stream);
    long bx = (L_in + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(resample_sinc_adjoint_kernel, dim3((unsigned)bx, B), dim3(256), 0, (hipStream_t)stream, g, g_bs, out, out_bs,
                       L_in, L_out, kernel, krange, orig, new_, width, taps);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}
