// Objective evaluation metrics on gfx950: log-spectral distance (LSD) between a reference and an estimate, per frame and per
// clip, without a spectrogram in memory.  The definition is this project's own ("Evaluating a prior"): full
// frames only (T = 1 + (L - nfft) / hop, no centring, no padding), periodic Hann window, P = |rfft(w frame)|^2 floored at
// floor_pow, d = log10 Pref - log10 Pest, lsd[t] = sqrt(mean over bins [k_lo, k_hi) of d^2), LSD = mean over t of lsd[t].
// One workgroup per (frame, clip) like stft_fwd_kernel (stft.hip); both real signals ride ONE complex FFT in LDS
// (z = w ref + i w est) and are separated by the conjugate symmetry of a real signal's spectrum.
// The transform runs in DOUBLE.  A bandwidth-extension estimate is the worst input a packed float32 transform can get: where the
// estimate is 40 dB and more below the reference, its bins come out of the separation carrying the rounding error of the
// reference's butterflies (1.1e-7 of the spectrum's rms for radix-2 passes with float32 twiddles), and log10 turns a bin that
// happens to be small into an error of 1e-2.  Measured with fft_lds_inplace on a MI355X against the float64 statement of the
// tests: 3.5e-5 per frame over all 257 bins at nfft 512, 3.2e-4 on the Nyquist bin alone at nfft 4096, where the float32 window
// product alone already costs 5e-5 - against a bar of 2e-5.  In double the same layout is exact to 1e-11 on any signal; what is left,
// 1e-6, is the float32 log10 at the end (measured: 1.03e-6 at worst over the tests' cases).
// HBM-bound on the two inputs (each sample is read nfft / hop times, from L2 after the first); one float per frame goes out.
#include "common.h"
#include "fft_lds.h"
#include "../../include/babe_hip.h"
#include "prof.h"

namespace {

// exp(-2 pi i q / 4096), q < 2048, in double: the twiddles of every transform size (stride 4096 / n) and, through its real part,
// the Hann window.  Evaluated by the compiler: cos / sin of the first octant from their Taylor series (x <= pi / 4: the eleventh
// term is below 1e-21), the other octants by symmetry, so cos(pi / 2) is exactly 0 and the table is exactly symmetric.
struct TwTable {
    double v[2 * 2048];
};
constexpr double tw_series(double x, bool sine) {
    double term = sine ? x : 1.0, sum = term;
    for (int j = 1; j <= 10; ++j) {
        const double a = sine ? 2.0 * j : 2.0 * j - 1.0;
        term *= -x * x / (a * (a + 1.0));
        sum += term;
    }
    return sum;
}
constexpr TwTable make_tw4096() {
    TwTable t{};
    double c[513] = {}, s[513] = {};
    for (int q = 0; q <= 512; ++q) {
        const double x = 2.0 * 3.14159265358979323846 * q / 4096.0;
        c[q] = tw_series(x, false);
        s[q] = tw_series(x, true);
    }
    for (int q = 0; q < 2048; ++q) {
        const int r = q > 1024 ? 2048 - q : q;                 // angle folded into [0, pi / 2]: cos changes sign
        const double cr = r > 512 ? s[1024 - r] : c[r], sr = r > 512 ? c[1024 - r] : s[r];
        t.v[2 * q] = q > 1024 ? -cr : cr;
        t.v[2 * q + 1] = -sr;
    }
    return t;
}
__device__ constexpr TwTable kTw4096 alignas(16) = make_tw4096();

__device__ __forceinline__ double2 cmul(double2 x, double2 w) {
    return make_double2(x.x * w.x - x.y * w.y, x.x * w.y + x.y * w.x);
}

// fft_lds_inplace (fft_lds.h) on double2, forward only: in-place decimation in time on bit-reversed input, the same LDS image
// (element i at fft_at(i)), two radix-2 stages per pass, an odd log2(n) opens with a single radix-2 stage.  All threads call.
__device__ __forceinline__ void fft_lds_f64(double2* a, int log2n, const double2* __restrict__ tw) {
    const int n = 1 << log2n;
    int s = 1;
    if (log2n & 1) {
        __syncthreads();
        for (int k = threadIdx.x; k < (n >> 1); k += blockDim.x) {
            const double2 u = a[fft_at(2 * k)], x = a[fft_at(2 * k + 1)];
            a[fft_at(2 * k)] = make_double2(u.x + x.x, u.y + x.y);
            a[fft_at(2 * k + 1)] = make_double2(u.x - x.x, u.y - x.y);
        }
        s = 2;
    }
    for (; s < log2n; s += 2) {
        __syncthreads();
        const int hm = 1 << (s - 1);
        const int t1 = 4096 >> s, t2 = 4096 >> (s + 1);
        for (int k = threadIdx.x; k < (n >> 2); k += blockDim.x) {
            const int j = k & (hm - 1);
            const int base = ((k >> (s - 1)) << (s + 1)) + j;
            const double2 w1 = tw[j * t1], w2 = tw[j * t2], w3 = tw[(j + hm) * t2];
            const int i0 = fft_at(base), i1 = fft_at(base + hm), i2 = fft_at(base + 2 * hm), i3 = fft_at(base + 3 * hm);
            const double2 x0 = a[i0], x1 = a[i1], x2 = a[i2], x3 = a[i3];
            const double2 v1 = cmul(x1, w1), v3 = cmul(x3, w1);
            const double2 y0 = make_double2(x0.x + v1.x, x0.y + v1.y), y1 = make_double2(x0.x - v1.x, x0.y - v1.y);
            const double2 y2 = make_double2(x2.x + v3.x, x2.y + v3.y), y3 = make_double2(x2.x - v3.x, x2.y - v3.y);
            const double2 u2 = cmul(y2, w2), u3 = cmul(y3, w3);
            a[i0] = make_double2(y0.x + u2.x, y0.y + u2.y);
            a[i2] = make_double2(y0.x - u2.x, y0.y - u2.y);
            a[i1] = make_double2(y1.x + u3.x, y1.y + u3.y);
            a[i3] = make_double2(y1.x - u3.x, y1.y - u3.y);
        }
    }
    __syncthreads();
}

// grid (T, B), 256 threads, FFT_LDS_LEN(n) double2 of dynamic LDS.  Frame t of clip b: samples [t hop, t hop + n) of both rows -
// inside [0, L) because T counts full frames only.  Writes frame_lsd[b * T + t] and nothing else.
__global__ __launch_bounds__(256) void lsd_frames_kernel(const float* __restrict__ ref, long ref_bs,
                                                         const float* __restrict__ est, long est_bs, int log2n, int hop,
                                                         int k_lo, int k_hi, float floor_pow, float* __restrict__ frame_lsd) {
    extern __shared__ double2 a[];
    __shared__ double part[4];
    const int n = 1 << log2n;
    const int t = blockIdx.x, b = blockIdx.y, T = gridDim.x;
    const long s0 = (long)t * hop;
    const float* rb = ref + (long)b * ref_bs + s0;
    const float* eb = est + (long)b * est_bs + s0;
    const double2* tw = reinterpret_cast<const double2*>(kTw4096.v);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        // periodic Hann, 0.5 - 0.5 cos(2 pi i / n): the cosine is the real part of table entry q = i 4096 / n, its sign flipped
        // in the second half of the circle
        const int q = i << (12 - log2n);
        const double c = q < 2048 ? tw[q].x : -tw[q - 2048].x;
        const double w = 0.5 - 0.5 * c;
        a[fft_at(bitrev_n(i, log2n))] = make_double2(w * (double)rb[i], w * (double)eb[i]);
    }
    fft_lds_f64(a, log2n, tw);
    // Z = X + i Y with X, Y the spectra of two REAL signals: X[k] = (Z[k] + conj Z[n-k]) / 2, Y[k] = (Z[k] - conj Z[n-k]) / (2i).
    // k = 0 and k = n/2 are their own mirror bins (n - 0 wraps to 0): there X = Re Z and Y = Im Z, both real.
    const double fl = (double)floor_pow;
    double acc = 0.0;
    for (int k = k_lo + (int)threadIdx.x; k < k_hi; k += blockDim.x) {
        const double2 z = a[fft_at(k)];
        double pr, pe;
        if (k == 0 || k == (n >> 1)) {
            pr = z.x * z.x;
            pe = z.y * z.y;
        } else {
            const double2 m = a[fft_at(n - k)];
            const double xr = 0.5 * (z.x + m.x), xi = 0.5 * (z.y - m.y);
            const double yr = 0.5 * (z.y + m.y), yi = -0.5 * (z.x - m.x);
            pr = xr * xr + xi * xi;
            pe = yr * yr + yi * yi;
        }
        // log10 Pref - log10 Pest as ONE float32 logarithm of the double ratio, both floored first (1 ulp of a value below 30:
        // 2e-6); a ratio float32 cannot hold - floors below 1e-30 - takes the double logarithm
        const double r = fmax(pr, fl) / fmax(pe, fl);
        const float d = (r > 1e-30 && r < 1e30) ? log10f((float)r) : (float)log10(r);
        acc += (double)d * (double)d;
    }
    // fixed order: the thread's bins ascending, the wave's 64 lanes by butterfly, the four waves through LDS
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s = (part[0] + part[1]) + (part[2] + part[3]);
        frame_lsd[(long)b * T + t] = (float)sqrt(s / (double)(k_hi - k_lo));
    }
}

// grid (B), 256 threads: clip_lsd[b] = mean over t of frame_lsd[b][t], double accumulators in one fixed order
__global__ __launch_bounds__(256) void lsd_clip_mean_kernel(const float* __restrict__ frame_lsd, int T,
                                                            float* __restrict__ clip_lsd) {
    __shared__ double part[4];
    const int b = blockIdx.x;
    const float* f = frame_lsd + (long)b * T;
    double acc = 0.0;
    for (int t = threadIdx.x; t < T; t += blockDim.x) acc += (double)f[t];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) clip_lsd[b] = (float)(((part[0] + part[1]) + (part[2] + part[3])) / (double)T);
}

int lsd_log2(int n) {
    for (int l = 8; l <= 12; ++l)
        if ((1 << l) == n) return l;
    return -1;
}

}  // namespace

extern "C" long babe_lsd_num_frames(int L, int nfft, int hop) {
    if (lsd_log2(nfft) < 0 || hop < 1 || hop > nfft || L < nfft) return -1;
    return 1 + (long)(L - nfft) / hop;
}

extern "C" int babe_lsd_frames(const float* ref, long ref_bs, const float* est, long est_bs, int L, int B, int nfft, int hop,
                               int k_lo, int k_hi, float floor_pow, float* frame_lsd, float* clip_lsd, void* stream) {
    const int lg = lsd_log2(nfft);
    BABE_CHECK_ARG(ref && est && frame_lsd, "lsd_frames: null pointer");
    BABE_CHECK_ARG(lg >= 0, "lsd_frames: nfft=%d unsupported (256..4096, power of two)", nfft);
    BABE_CHECK_ARG(hop >= 1 && hop <= nfft, "lsd_frames: hop=%d (1 .. nfft=%d)", hop, nfft);
    BABE_CHECK_ARG(L >= nfft, "lsd_frames: L=%d holds no full frame of nfft=%d", L, nfft);
    BABE_CHECK_ARG(B >= 1 && B <= 65535, "lsd_frames: B=%d (1 .. 65535)", B);
    BABE_CHECK_ARG(0 <= k_lo && k_lo < k_hi && k_hi <= nfft / 2 + 1, "lsd_frames: bins [%d, %d) outside [0, %d]", k_lo, k_hi,
                   nfft / 2 + 1);
    BABE_CHECK_ARG(floor_pow > 0.f, "lsd_frames: floor_pow=%g must be positive", (double)floor_pow);      // (NaN fails too)
    const int T = (int)babe_lsd_num_frames(L, nfft, hop);
    BabeProfScope prof(BABE_SLOT_SAMPLER, 8.0 * B * (double)L + 4.0 * B * (double)T,
                       (double)B * T * (10.0 * nfft * lg + 20.0 * (k_hi - k_lo)), 0, stream);
    // nfft 4096: 67.6 KB of LDS, above the 64 KB a kernel gets without asking
    const size_t lds = (size_t)FFT_LDS_LEN(nfft) * sizeof(double2);
    static std::atomic<unsigned long long> attr_done{0};
    if (babe_lds_optin(attr_done, {reinterpret_cast<const void*>(&lsd_frames_kernel)}, (int)(FFT_LDS_LEN(4096) * sizeof(double2))) !=
        hipSuccess) {
        babe_set_error("lsd_frames: no %d bytes of LDS for the kernel", (int)(FFT_LDS_LEN(4096) * sizeof(double2)));
        return BABE_ERR_HIP;
    }
    hipLaunchKernelGGL(lsd_frames_kernel, dim3(T, B), dim3(256), lds, (hipStream_t)stream, ref, ref_bs, est, est_bs, lg, hop, k_lo,
                       k_hi, floor_pow, frame_lsd);
    BABE_LAUNCH_CHECK();
    if (clip_lsd) {
        hipLaunchKernelGGL(lsd_clip_mean_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, frame_lsd, T, clip_lsd);
        BABE_LAUNCH_CHECK();
    }
    return BABE_OK;
}
