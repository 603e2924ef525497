// Observation operators of the EDM sampler's declipping and phase-retrieval tasks (the reference's testing/edm_sampler.py:308-384
// poses them to the diffusion prior; its guidance :56-94 differentiates ||y - A(x)||_2 through A):
//   clip            A(x) = clip(x, -c, c); torch.clip's gradient: 1 on the closed interval [-c, c], 0 outside
//   STFT magnitude  A(x) = |STFT(cat(x, zeros(win)))|, periodic Hamming window, center=False, frames = 1 + L / hop
// each with its vector-Jacobian product.  No atomics anywhere: repeats are bit-identical and a row never depends on the batch.
//
// STFT magnitude: one workgroup per frame, the frame's transform in LDS (fft_lds.h; the real frame enters as a complex one with
// zero imaginary part, like stft_fwd_kernel), samples at or beyond L read as zero - no padded copy of x.  The forward keeps the
// complex spectrum [B][frames][bins] for the VJP, which forms Z = G X / |X| (0 where |X| == 0: the convention of this library,
// where torch's sqrt gives NaN), applies the ADJOINT of the one-sided transform f[n] = Re sum_{k <= win/2} Z_k e^{+2 pi i k n / win}
// (the upper half of the inverse transform's input is zero: no Hermitian doubling, this is not irfft), the window, and leaves
// the frame in the workspace; a second kernel overlap-adds as a gather, every output sample summing its <= ceil(win / hop)
// frames in ascending frame order.
#include "common.h"
#include "fft_lds.h"
#include "../../include/babe_hip.h"
#include "prof.h"

namespace {

constexpr int CLIP_CHUNK = 256;                 // samples per wave and pass: 64 lanes x one float4

// r = y - clip(x), mask = |x| <= c, part[b][blk] = the sum of r^2 babe_sumsq_partial(r) gives, bit for bit: that kernel's thread
// t of block blk adds the samples (k nblk + blk) 256 + t, k ascending, then the block reduces.  Here wave w of the block takes
// chunk k0 + w of 256 consecutive samples with one 16-byte load per lane, leaves r in LDS, and thread t adds column t of the
// four chunks in the same order.  grid (nblk, B), 256 threads.  vec: rows of x, y, r 16-byte aligned and mask rows 4-byte.
__global__ __launch_bounds__(256) void clip_residual_kernel(const float* __restrict__ x, long x_bs, const float* __restrict__ y,
                                                            long y_bs, float c, float* __restrict__ r, long r_bs,
                                                            unsigned char* __restrict__ mask, long mask_bs,
                                                            double* __restrict__ part, int nblk, long L, int vec) {
    __shared__ float sr[4][CLIP_CHUNK];
    __shared__ double sh[4];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* xb = x + (long)b * x_bs;
    const float* yb = y + (long)b * y_bs;
    float* rb = r + (long)b * r_bs;
    unsigned char* mb = mask + (long)b * mask_bs;
    const long nchunks = (L + CLIP_CHUNK - 1) / CLIP_CHUNK;
    double acc = 0;
    for (long k0 = 0; k0 * nblk + blockIdx.x < nchunks; k0 += 4) {       // (block-uniform: every wave meets both barriers)
        const long chunk = (k0 + wave) * nblk + blockIdx.x;
        const long i0 = chunk * CLIP_CHUNK + 4 * lane;
        float rv[4] = {0.f, 0.f, 0.f, 0.f};
        if (chunk < nchunks) {
            if (vec && i0 + 3 < L) {
                const float4 xv = *reinterpret_cast<const float4*>(xb + i0);
                const float4 yv = *reinterpret_cast<const float4*>(yb + i0);
                const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ys[4] = {yv.x, yv.y, yv.z, yv.w};
                unsigned char ms[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    rv[j] = ys[j] - fminf(fmaxf(xs[j], -c), c);
                    ms[j] = fabsf(xs[j]) <= c ? 1 : 0;
                }
                *reinterpret_cast<float4*>(rb + i0) = make_float4(rv[0], rv[1], rv[2], rv[3]);
                *reinterpret_cast<uchar4*>(mb + i0) = make_uchar4(ms[0], ms[1], ms[2], ms[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i0 + j < L) {
                        const float xv = xb[i0 + j];
                        rv[j] = yb[i0 + j] - fminf(fmaxf(xv, -c), c);
                        rb[i0 + j] = rv[j];
                        mb[i0 + j] = fabsf(xv) <= c ? 1 : 0;
                    }
            }
        }
        *reinterpret_cast<float4*>(&sr[wave][4 * lane]) = make_float4(rv[0], rv[1], rv[2], rv[3]);   // (0 beyond L)
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const double v = sr[w][threadIdx.x];
            acc += v * v;
        }
        __syncthreads();
    }
    acc = block_sum<4>(acc, sh);
    if (threadIdx.x == 0) part[(long)b * nblk + blockIdx.x] = acc;
}

// out = clip(x, -c, c) (mask NULL) or out = x * mask (the adjoint; c unused).  One float4 per thread and pass; grid (bx, B).
__global__ __launch_bounds__(256) void clip_map_kernel(const float* __restrict__ x, long x_bs, float c,
                                                       const unsigned char* __restrict__ mask, long mask_bs,
                                                       float* __restrict__ out, long out_bs, long L, int vec) {
    const int b = blockIdx.y;
    const float* xb = x + (long)b * x_bs;
    float* ob = out + (long)b * out_bs;
    const unsigned char* mb = mask ? mask + (long)b * mask_bs : nullptr;
    for (long i0 = 4 * ((long)blockIdx.x * blockDim.x + threadIdx.x); i0 < L; i0 += 4 * (long)gridDim.x * blockDim.x) {
        if (vec && i0 + 3 < L) {
            const float4 xv = *reinterpret_cast<const float4*>(xb + i0);
            float4 o;
            if (mb) {
                const uchar4 m = *reinterpret_cast<const uchar4*>(mb + i0);
                o = make_float4(m.x ? xv.x : 0.f, m.y ? xv.y : 0.f, m.z ? xv.z : 0.f, m.w ? xv.w : 0.f);
            } else {
                o = make_float4(fminf(fmaxf(xv.x, -c), c), fminf(fmaxf(xv.y, -c), c), fminf(fmaxf(xv.z, -c), c),
                                fminf(fmaxf(xv.w, -c), c));
            }
            *reinterpret_cast<float4*>(ob + i0) = o;
        } else {
            for (int j = 0; j < 4 && i0 + j < L; ++j) {
                const float xv = xb[i0 + j];
                ob[i0 + j] = mb ? (mb[i0 + j] ? xv : 0.f) : fminf(fmaxf(xv, -c), c);
            }
        }
    }
}

// grid (frames, B), 256 threads, FFT_LDS_LEN(win) float2 of dynamic LDS
__global__ __launch_bounds__(256) void stft_mag_fwd_kernel(const float* __restrict__ x, long x_bs, long L,
                                                           const float* __restrict__ window, int log2n, int hop, int frames,
                                                           float2* __restrict__ spec, float* __restrict__ mag,
                                                           const float2* __restrict__ tw) {
    extern __shared__ float2 a[];
    const int n = 1 << log2n, nb = (n >> 1) + 1;
    const int t = blockIdx.x, b = blockIdx.y;
    const float* xb = x + (long)b * x_bs;
    const long s0 = (long)t * hop;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const long s = s0 + i;
        const float v = (s < L) ? xb[s] * window[i] : 0.f;
        a[fft_at(bitrev_n(i, log2n))] = make_float2(v, 0.f);
    }
    fft_lds_inplace(a, log2n, tw, -1);
    float2* sp = spec + ((long)b * frames + t) * nb;
    float* mg = mag + (long)b * nb * frames + t;
    for (int k = threadIdx.x; k < nb; k += blockDim.x) {
        const float2 X = a[fft_at(k)];
        sp[k] = X;
        mg[(long)k * frames] = sqrtf(X.x * X.x + X.y * X.y);
    }
}

// grid (frames, B): ws[b][t][i] = window[i] Re sum_{k <= win/2} Z_k e^{+2 pi i k i / win}, Z = G X / |X|
__global__ __launch_bounds__(256) void stft_mag_vjp_frames_kernel(const float* __restrict__ G, const float2* __restrict__ spec,
                                                                  const float* __restrict__ window, int log2n, int frames,
                                                                  float* __restrict__ ws, const float2* __restrict__ tw) {
    extern __shared__ float2 a[];
    const int n = 1 << log2n, nb = (n >> 1) + 1;
    const int t = blockIdx.x, b = blockIdx.y;
    const float2* sp = spec + ((long)b * frames + t) * nb;
    const float* g = G + (long)b * nb * frames + t;
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        float2 z = make_float2(0.f, 0.f);
        if (k < nb) {
            const float2 X = sp[k];
            const float m = sqrtf(X.x * X.x + X.y * X.y);
            if (m > 0.f) {
                const float s = g[(long)k * frames] / m;
                z = make_float2(s * X.x, s * X.y);
            }
        }
        a[fft_at(bitrev_n(k, log2n))] = z;
    }
    fft_lds_inplace(a, log2n, tw, +1);
    float* o = ws + ((long)b * frames + t) * n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) o[i] = a[fft_at(i)].x * window[i];
}

// gx[b][i] = sum over the frames t with t hop <= i < t hop + win of ws[b][t][i - t hop], t ascending; grid (bx, B)
__global__ __launch_bounds__(256) void stft_mag_vjp_ola_kernel(const float* __restrict__ ws, float* __restrict__ gx, long gx_bs,
                                                               long L, int n, int hop, int frames) {
    const int b = blockIdx.y;
    const float* f = ws + (long)b * frames * n;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < L; i += (long)gridDim.x * blockDim.x) {
        long t1 = i / hop;                                           // latest frame that holds sample i
        if (t1 > frames - 1) t1 = frames - 1;
        const long t0 = i < n ? 0 : (i - n) / hop + 1;               // earliest: t hop + win > i
        float acc = 0.f;
        for (long t = t0; t <= t1; ++t) acc += f[t * n + (i - t * hop)];
        gx[(long)b * gx_bs + i] = acc;
    }
}

// ---- gradient of the matrix 2-norm of a residual R [rows][cols] (the reference's torch.linalg.norm(y - A(x), dim=(1, 2), ord=2) on
// a 3-D observation is the largest singular value s1 of R; d s1 / dR = u1 v1^T): power iteration on R^T R, started from
// u = ones, as alternating products w = R v / |v| and z = R^T w / |w|.  Every block recomputes the norm of its (short) input
// vector in a fixed order, so there are no atomics and no pass between the products.
__device__ __forceinline__ double block_sumsq(const float* __restrict__ v, int n, double* sh) {
    double acc = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += (double)v[i] * v[i];
    const double t = block_sum<4>(acc, sh);
    __syncthreads();
    return t;
}

// w[b][k] = sum_t R[b][k][t] v[b][t] / |v[b]|: one wave per row k; grid (ceil(rows / 4), B), 256 threads
__global__ __launch_bounds__(256) void specnorm_rows_kernel(const float* __restrict__ R, long r_bs, const float* __restrict__ v,
                                                            float* __restrict__ w, int rows, int cols) {
    __shared__ double sh[4];
    const int b = blockIdx.y, lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);
    const float* vb = v + (long)b * cols;
    const double n2 = block_sumsq(vb, cols, sh);
    if (k >= rows) return;
    const float* row = R + (long)b * r_bs + (long)k * cols;
    double acc = 0;
    for (int t = lane; t < cols; t += 64) acc += (double)row[t] * vb[t];
    acc = wave_sum(acc);
    if (lane == 0) w[(long)b * rows + k] = n2 > 0 ? (float)(acc / sqrt(n2)) : 0.f;
}

// z[b][t] = sum_k R[b][k][t] u[b][k] / |u[b]| (u NULL: ones): 64 columns x 4 row groups per block; grid (ceil(cols / 64), B)
__global__ __launch_bounds__(256) void specnorm_cols_kernel(const float* __restrict__ R, long r_bs, const float* __restrict__ u,
                                                            float* __restrict__ z, int rows, int cols) {
    __shared__ double sh[4];
    __shared__ double part[4][64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, g = threadIdx.x >> 6, t = blockIdx.x * 64 + lane;
    const float* ub = u ? u + (long)b * rows : nullptr;
    const double n2 = ub ? block_sumsq(ub, rows, sh) : (double)rows;
    const float* Rb = R + (long)b * r_bs;
    double acc = 0;
    if (t < cols)
        for (int k = g; k < rows; k += 4) acc += (double)Rb[(long)k * cols + t] * (ub ? ub[k] : 1.f);
    part[g][lane] = acc;
    __syncthreads();
    if (g == 0 && t < cols) {
        const double s = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        z[(long)b * cols + t] = n2 > 0 ? (float)(s / sqrt(n2)) : 0.f;
    }
}

// out[b][k][t] = -(u[k] / |u|) (v[t] / |v|): d s1 / d(rec) at R = y - rec; 0 where R has no non-zero singular value
__global__ __launch_bounds__(256) void specnorm_seed_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                            float* __restrict__ out, long out_bs, int rows, int cols) {
    __shared__ double sh[4];
    const int b = blockIdx.y;
    const float* ub = u + (long)b * rows;
    const float* vb = v + (long)b * cols;
    const double nu = block_sumsq(ub, rows, sh), nv = block_sumsq(vb, cols, sh);
    const float sc = (nu > 0 && nv > 0) ? (float)(-1.0 / sqrt(nu * nv)) : 0.f;
    const long n = (long)rows * cols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[(long)b * out_bs + i] = sc * ub[i / cols] * vb[i % cols];
}

int ilog2_win(int n) {
    for (int l = 8; l <= 12; ++l)
        if ((1 << l) == n) return l;
    return -1;
}

inline bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

}  // namespace

extern "C" int babe_clip_residual(const float* x, long x_bs, const float* y, long y_bs, float c, float* r, long r_bs,
                                  unsigned char* mask, long mask_bs, double* part, int nblk, int B, long L, void* stream) {
    BABE_CHECK_ARG(x && y && r && mask && part && nblk > 0 && B > 0 && L > 0, "clip_residual: bad arguments");
    BABE_CHECK_ARG(c >= 0.f, "clip_residual: clip value %g below 0", (double)c);
    BABE_CHECK_ARG(x_bs >= L && y_bs >= L && r_bs >= L && mask_bs >= L, "clip_residual: a row stride below L = %ld", L);
    const int vec = aligned(x, 16) && aligned(y, 16) && aligned(r, 16) && aligned(mask, 4) &&
                    (B == 1 || (x_bs % 4 == 0 && y_bs % 4 == 0 && r_bs % 4 == 0 && mask_bs % 4 == 0));
    BabeProfScope prof(BABE_SLOT_SAMPLER, 13.0 * B * (double)L, 0, 0, stream);
    hipLaunchKernelGGL(clip_residual_kernel, dim3(nblk, B), dim3(256), 0, (hipStream_t)stream, x, x_bs, y, y_bs, c, r, r_bs, mask,
                       mask_bs, part, nblk, L, vec);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

static int clip_map(const char* what, const float* x, long x_bs, float c, const unsigned char* mask, long mask_bs, float* out,
                    long out_bs, int B, long L, void* stream) {
    BABE_CHECK_ARG(x && out && B > 0 && L > 0, "%s: bad arguments", what);
    BABE_CHECK_ARG(x_bs >= L && out_bs >= L && (!mask || mask_bs >= L), "%s: a row stride below L = %ld", what, L);
    const int vec = aligned(x, 16) && aligned(out, 16) && (!mask || aligned(mask, 4)) &&
                    (B == 1 || (x_bs % 4 == 0 && out_bs % 4 == 0 && (!mask || mask_bs % 4 == 0)));
    BabeProfScope prof(BABE_SLOT_SAMPLER, (mask ? 9.0 : 8.0) * B * (double)L, 0, 0, stream);
    long bx = (L + 1023) / 1024;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(clip_map_kernel, dim3((unsigned)bx, B), dim3(256), 0, (hipStream_t)stream, x, x_bs, c, mask, mask_bs, out,
                       out_bs, L, vec);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" int babe_clip_fwd(const float* x, long x_bs, float c, float* out, long out_bs, int B, long L, void* stream) {
    BABE_CHECK_ARG(c >= 0.f, "clip_fwd: clip value %g below 0", (double)c);
    return clip_map("clip_fwd", x, x_bs, c, nullptr, 0, out, out_bs, B, L, stream);
}

extern "C" int babe_clip_adj(const float* g, long g_bs, const unsigned char* mask, long mask_bs, float* out, long out_bs, int B,
                             long L, void* stream) {
    BABE_CHECK_ARG(mask, "clip_adj: the forward's mask is required");
    return clip_map("clip_adj", g, g_bs, 0.f, mask, mask_bs, out, out_bs, B, L, stream);
}

extern "C" long babe_stft_mag_workspace(int B, int frames, int win) {
    if (B <= 0 || frames <= 0 || ilog2_win(win) < 0) return -1;
    return 4L * B * (long)frames * win;
}

extern "C" int babe_stft_mag_fwd(const float* x, long x_bs, long L, const float* window, int win, int hop, float* spec, float* mag,
                                 int B, int frames, const float* tw4096, void* stream) {
    const int lg = ilog2_win(win);
    BABE_CHECK_ARG(x && window && spec && mag && tw4096 && B > 0 && L > 0, "stft_mag_fwd: bad arguments");
    BABE_CHECK_ARG(lg >= 0, "stft_mag_fwd: win=%d unsupported (a power of two, 256..4096)", win);
    BABE_CHECK_ARG(hop >= 1 && hop <= win, "stft_mag_fwd: hop=%d outside 1..win=%d", hop, win);
    BABE_CHECK_ARG(frames == 1 + L / hop, "stft_mag_fwd: frames=%d inconsistent with L=%ld, hop=%d", frames, L, hop);
    BABE_CHECK_ARG(x_bs >= L, "stft_mag_fwd: row stride %ld below L = %ld", x_bs, L);
    const int nb = win / 2 + 1;
    BabeProfScope prof(BABE_SLOT_STFT_FWD, (double)B * (4.0 * L + 12.0 * frames * nb), 5.0 * B * (double)frames * win * lg, 0, stream);
    hipLaunchKernelGGL(stft_mag_fwd_kernel, dim3(frames, B), dim3(256), FFT_LDS_LEN(win) * sizeof(float2), (hipStream_t)stream, x,
                       x_bs, L, window, lg, hop, frames, reinterpret_cast<float2*>(spec), mag,
                       reinterpret_cast<const float2*>(tw4096));
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" int babe_stft_mag_vjp(const float* G, const float* spec, const float* window, int win, int hop, float* gx, long gx_bs,
                                 long L, int B, int frames, const float* tw4096, void* workspace, long workspace_bytes,
                                 void* stream) {
    const int lg = ilog2_win(win);
    BABE_CHECK_ARG(G && spec && window && gx && tw4096 && workspace && B > 0 && L > 0, "stft_mag_vjp: bad arguments");
    BABE_CHECK_ARG(lg >= 0, "stft_mag_vjp: win=%d unsupported (a power of two, 256..4096)", win);
    BABE_CHECK_ARG(hop >= 1 && hop <= win, "stft_mag_vjp: hop=%d outside 1..win=%d", hop, win);
    BABE_CHECK_ARG(frames == 1 + L / hop, "stft_mag_vjp: frames=%d inconsistent with L=%ld, hop=%d", frames, L, hop);
    BABE_CHECK_ARG(gx_bs >= L, "stft_mag_vjp: row stride %ld below L = %ld", gx_bs, L);
    const long need = babe_stft_mag_workspace(B, frames, win);
    BABE_CHECK_ARG(workspace_bytes >= need, "stft_mag_vjp: workspace %ld bytes, need %ld", workspace_bytes, need);
    const int nb = win / 2 + 1;
    float* ws = (float*)workspace;
    {
        BabeProfScope prof(BABE_SLOT_ISTFT, (double)B * frames * (12.0 * nb + 4.0 * win), 5.0 * B * (double)frames * win * lg, 0,
                           stream);
        hipLaunchKernelGGL(stft_mag_vjp_frames_kernel, dim3(frames, B), dim3(256), FFT_LDS_LEN(win) * sizeof(float2),
                           (hipStream_t)stream, G, reinterpret_cast<const float2*>(spec), window, lg, frames, ws,
                           reinterpret_cast<const float2*>(tw4096));
        BABE_LAUNCH_CHECK();
    }
    BabeProfScope prof(BABE_SLOT_ISTFT, (double)B * (4.0 * frames * win + 4.0 * L), 0, 0, stream);
    long bx = (L + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(stft_mag_vjp_ola_kernel, dim3((unsigned)bx, B), dim3(256), 0, (hipStream_t)stream, ws, gx, gx_bs, L, win,
                       hop, frames);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" long babe_specnorm_workspace(int B, int rows, int cols) {
    if (B <= 0 || rows <= 0 || cols <= 0) return -1;
    return 4L * B * ((long)rows + cols);
}

extern "C" int babe_specnorm_seed(const float* r, long r_bs, int rows, int cols, int iters, float* out, long out_bs, int B,
                                  void* workspace, long workspace_bytes, void* stream) {
    BABE_CHECK_ARG(r && out && workspace && B > 0 && rows > 0 && cols > 0, "specnorm_seed: bad arguments");
    BABE_CHECK_ARG(iters >= 1 && iters <= 1024, "specnorm_seed: iters=%d outside 1..1024", iters);
    const long n = (long)rows * cols;
    BABE_CHECK_ARG(r_bs >= n && out_bs >= n, "specnorm_seed: a row stride below rows * cols = %ld", n);
    const long need = babe_specnorm_workspace(B, rows, cols);
    BABE_CHECK_ARG(workspace_bytes >= need, "specnorm_seed: workspace %ld bytes, need %ld", workspace_bytes, need);
    float* u = (float*)workspace;
    float* v = u + (long)B * rows;
    hipStream_t st = (hipStream_t)stream;
    BabeProfScope prof(BABE_SLOT_SAMPLER, 4.0 * B * (double)n * (2.0 * iters + 2.0), 4.0 * B * (double)n * iters, 0, stream);
    const dim3 gr((rows + 3) / 4, B), gc((cols + 63) / 64, B);
    hipLaunchKernelGGL(specnorm_cols_kernel, gc, dim3(256), 0, st, r, r_bs, (const float*)nullptr, v, rows, cols);
    BABE_LAUNCH_CHECK();
    for (int i = 0; i < iters; ++i) {
        hipLaunchKernelGGL(specnorm_rows_kernel, gr, dim3(256), 0, st, r, r_bs, (const float*)v, u, rows, cols);
        BABE_LAUNCH_CHECK();
        hipLaunchKernelGGL(specnorm_cols_kernel, gc, dim3(256), 0, st, r, r_bs, (const float*)u, v, rows, cols);
        BABE_LAUNCH_CHECK();
    }
    long bx = (n + 1023) / 1024;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(specnorm_seed_kernel, dim3((unsigned)bx, B), dim3(256), 0, st, (const float*)u, (const float*)v, out, out_bs,
                       rows, cols);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}
