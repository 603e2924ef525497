// One whole SAMPLING RUN of the blind bandwidth-extension sampler from plan handles - the loop BlindSampler._sample -> step ->
// _heun_first / _heun_second (babe_amd/testing/blind_bwe_sampler.py) sequences from Python, as ONE C-ABI call for a non-Python
// host: STFT of the observations, the initial state, and per step the noise injection (move_timestep :509-516), the score
// evaluation (babe_score_eval, csrc/score_eval.hip) and the Euler or second-order Heun update (:687-761), with the filter
// parameters handed from evaluation to evaluation on the device.
// Scope: that of babe_score_eval - the AR observation model of predict_bwe_AR (desc.eval.mask / dc_mask) and the known
// degradations of desc.eval.obs_kind included: the loop is the same, the descriptor goes through - and, with
// desc.skip_zero_inject and y == NULL, the loop of testing/edm_sampler.Sampler.predict_conditional: no injection on a step with
// gamma == 0, unconditional sampling.  Like babe_score_eval, the run contains no schedule formula: the caller passes one
// babe_sample_step per step (babe_edm_steps below fills the table for a host without the Python EDM class).  Same kernels, same
// order, same scalars as the Python loops, so they agree bit for bit (tests/test_gpu_sample_c.py, tests/test_gpu_obs_library.py).
// Nothing allocates, nothing synchronises.  Below the run: the host helpers babe_firwin_kaiser and babe_iir_check.
#include <cmath>
#include "common.h"
#include "eval_geom.h"
#include "workspace.h"

namespace {

// the run's workspace, stated once (babe_sample_workspace_bytes runs it dry): babe_score_eval's block of ev_bytes, then the run's
// own buffers, specY and seven [B][L] signals
struct SampleWork {
    void* ev;
    float *specY, *buf[7];
};
void carve(Carver& c, const babe_eval_desc* e, const EvalGeom& g, int B, long ev_bytes, SampleWork& w) {
    w.ev = c.take<char>((size_t)ev_bytes);
    w.specY = c.take<float>((size_t)B * 2 * g.frames * g.nbins);
    for (float*& b : w.buf) b = c.take<float>((size_t)B * e->L);
}

}  // namespace

extern "C" long babe_sample_workspace_bytes(const babe_sample_desc* d, int B) {
    if (!d || B < 1) {
        babe_set_error("sample_workspace_bytes: bad arguments");
        return -1;
    }
    const long ev = babe_eval_workspace_bytes(&d->eval, B);
    if (ev < 0) return -1;
    EvalGeom g;
    geom(&d->eval, g);                  // (it has a design: the evaluation was sized)
    Carver dry{nullptr, 0, 256};
    SampleWork w;
    carve(dry, &d->eval, g, B, ev, w);
    return (long)dry.used;
}

extern "C" int babe_sample_bwe(const babe_sample_desc* d, const float* y, float* params, float* x_out, const float* noise, long seed,
                               long clip0, float* rec_x_den, float* rec_params, void* ws, long ws_bytes, int B, void* stream) {
    // ---- host-side validation, all of it before the first launch
    BABE_CHECK_ARG(d, "sample_bwe: NULL descriptor");
    BABE_CHECK_ARG(d->T >= 1, "sample_bwe: T = %d steps", d->T);
    BABE_CHECK_ARG(d->steps, "sample_bwe: NULL step table");
    BABE_CHECK_ARG(B >= 1 && B <= 65535, "sample_bwe: B = %d", B);
    const babe_eval_desc* e = &d->eval;
    BABE_CHECK_ARG(eval_dims_ok(e), "sample_bwe: nfft = %d, L = %d", e->nfft, e->L);
    EvalGeom g;
    geom(e, g);                         // (the STFT part, all this function uses, needs no plan: the plans are looked at below)
    SampleWork w;
    Carver own{nullptr, 0, 256};
    carve(own, e, g, B, 0, w);
    BABE_CHECK_ARG(ws && ws_bytes >= (long)own.used, "sample_bwe: workspace of %ld bytes, the run's own buffers alone need %ld",
                   ws ? ws_bytes : 0L, (long)own.used);
    BABE_CHECK_ARG(y || !d->warm_start, "sample_bwe: warm_start without y");
    BABE_TRY(eval_desc_check(e, "sample_bwe", y != nullptr));
    const bool reads_params = eval_reads_params(e, y != nullptr);
    BABE_CHECK_ARG(x_out && (params || !reads_params), "sample_bwe: NULL params or x_out");
    BABE_CHECK_ARG(params || !rec_params, "sample_bwe: rec_params without params");
    const long ev_bytes = babe_eval_workspace_bytes(e, B);
    BABE_CHECK_ARG(ev_bytes >= 0, "sample_bwe: bad evaluation descriptor");
    Carver c{static_cast<char*>(ws), (size_t)ws_bytes, 256};
    carve(c, e, g, B, ev_bytes, w);
    BABE_CHECK_ARG(c.ok, "sample_bwe: workspace of %ld bytes, need %ld", ws_bytes, (long)c.used);
    BABE_TRY(sample_steps_check(d->steps, d->T, d->t0, "sample_bwe"));
    if (!noise)
        BABE_CHECK_ARG(clip0 >= 0 && clip0 + B <= 0x100000000L && d->T + 1L < 0x100000000L, "sample_bwe: clip0 = %ld outside the counter word", clip0);
    const long L = e->L, n = (long)B * L;
    const int P = e->shared ? 1 : B, frames = g.frames;
    float *x = x_out, *specY = w.specY, *x_hat = w.buf[0], *dd = w.buf[1], *x_den = w.buf[2], *x_prime = w.buf[3], *d2 = w.buf[4],
          *x_den2 = w.buf[5], *eps_ws = w.buf[6];
    hipStream_t st = (hipStream_t)stream;
#define COPY(dst, src, bytes)                                                                          \
    do {                                                                                               \
        const hipError_t e__ = hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToDevice, st);     \
        if (e__ != hipSuccess) {                                                                       \
            babe_set_error("%s:%d hipMemcpyAsync: %s", __FILE__, __LINE__, hipGetErrorString(e__));   \
            return BABE_ERR_HIP;                                                                       \
        }                                                                                              \
    } while (0)
    // draw k: rows of the caller's buffer, or the device generator into the one workspace buffer
    auto draw = [&](long k, const float** eps) -> int {
        if (noise) {
            *eps = noise + k * n;
            return BABE_OK;
        }
        *eps = eps_ws;
        return babe_randn(eps_ws, L, B, L, seed, clip0, k, stream);
    };
    const float* eps = nullptr;
    if (reads_params) BABE_TRY(babe_stft_fwd(y, L, (int)L, nullptr, specY, B, e->nfft, frames, e->tw4096, stream));
    // ---- initial state (:311 / :314): t0 eps, or y + t0 eps with a warm start
    BABE_TRY(draw(0, &eps));
    if (d->warm_start) BABE_TRY(babe_lincomb3(x, 1.f, y, d->t0, eps, 0.f, nullptr, n, stream));
    else BABE_TRY(babe_lincomb3(x, d->t0, eps, 0.f, nullptr, 0.f, nullptr, n, stream));
    for (int i = 0; i < d->T; ++i) {
        const babe_sample_step& s = d->steps[i];
        if (d->skip_zero_inject && s.inject == 0.f) {
            COPY(x_hat, x, 4L * n);                    // the state as it is: draw i + 1 is left unused
        } else {
            BABE_TRY(draw(i + 1L, &eps));
            BABE_TRY(babe_lincomb3(x_hat, 1.f, x, s.inject, eps, 0.f, nullptr, n, stream));
        }
        BABE_TRY(babe_score_eval(e, x_hat, s.t_hat, s.c1[0], s.c1[1], s.c1[2], s.c1[3], y, specY, params, dd, x_den, nullptr, w.ev, ev_bytes, B,
                                 stream));
        if (rec_x_den) COPY(rec_x_den + (long)i * n, x_den, 4L * n);
        if (rec_params) COPY(rec_params + (long)i * P * 2 * e->K, params, 4L * P * 2 * e->K);
        if (!s.heun) {
            BABE_TRY(babe_lincomb3(x, 1.f, x_hat, s.h, dd, 0.f, nullptr, n, stream));
        } else {
            BABE_TRY(babe_lincomb3(x_prime, 1.f, x_hat, s.h, dd, 0.f, nullptr, n, stream));
            BABE_TRY(babe_score_eval(e, x_prime, s.t_next, s.c2[0], s.c2[1], s.c2[2], s.c2[3], y, specY, params, d2, x_den2, nullptr, w.ev, ev_bytes,
                                     B, stream));
            BABE_TRY(babe_lincomb3(x, 1.f, x_hat, 0.5f * s.h, dd, 0.5f * s.h, d2, n, stream));
        }
    }
#undef COPY
    return BABE_OK;
}

/* The tester's schedule in double (diff_params/edm.py:38-75, :108-139; blind_bwe_sampler.py:509-516): t_i = (s0^(1/ro) +
 * i/(T-1) (sigma_min^(1/ro) - s0^(1/ro)))^ro for i < T, t_T = 0, s0 = start_sigma or sigma_max; gamma_i = min(Schurn/(T+1),
 * sqrt 2 - 1) where Stmin < t_i < Stmax (the reference divides by the T + 1 entries of the schedule). */
extern "C" int babe_edm_steps(babe_sample_step* steps, float* t0, int T, int order, double sigma_min, double sigma_max, double ro,
                              double sigma_data, double Schurn, double Stmin, double Stmax, double Snoise, double start_sigma) {
    BABE_CHECK_ARG(steps && t0 && T >= 2 && (order == 1 || order == 2), "edm_steps: bad arguments (T >= 2, order 1 or 2)");
    BABE_CHECK_ARG(sigma_min > 0 && sigma_max > sigma_min && ro > 0 && sigma_data > 0 && Schurn >= 0 && Snoise >= 0,
                   "edm_steps: sigma_min = %g, sigma_max = %g, ro = %g, sigma_data = %g, Schurn = %g, Snoise = %g", sigma_min, sigma_max, ro,
                   sigma_data, Schurn, Snoise);
    const double s0 = start_sigma > 0 ? start_sigma : sigma_max;
    const double a = std::pow(s0, 1.0 / ro), b = std::pow(sigma_min, 1.0 / ro);
    auto t_at = [&](int i) { return i >= T ? 0.0 : std::pow(a + (double)i / (T - 1) * (b - a), ro); };
    const double g = std::fmin(Schurn / (T + 1), std::sqrt(2.0) - 1.0);
    const double sd2 = sigma_data * sigma_data;
    auto precond = [&](double s, float c[4]) {
        c[0] = (float)(sd2 / (s * s + sd2));
        c[1] = (float)(s * sigma_data / std::sqrt(sd2 + s * s));
        c[2] = (float)(1.0 / std::sqrt(sd2 + s * s));
        c[3] = (float)(0.25 * std::log(s));
    };
    *t0 = (float)t_at(0);
    for (int i = 0; i < T; ++i) {
        const double t = t_at(i), tn = t_at(i + 1);
        const double gamma = (t > Stmin && t < Stmax) ? g : 0.0;
        const double t_hat = t + gamma * t;
        babe_sample_step& s = steps[i];
        memset(&s, 0, sizeof s);
        s.t_hat = (float)t_hat;
        s.inject = (float)(std::sqrt(t_hat * t_hat - t * t) * Snoise);
        s.t_next = (float)tn;
        s.h = (float)(tn - t_hat);
        s.heun = (tn != 0.0 && order == 2) ? 1 : 0;
        precond(t_hat, s.c1);
        if (s.heun) precond(tn, s.c2);
    }
    return BABE_OK;
}

// ---- host helpers for hosts without scipy (no GPU call) --------------------------------------------------------------------
namespace {

// sum of v[0..n) with the rounding errors carried along (Neumaier): correct to the last bit or two whatever the order
double compensated_sum(const double* v, int n) {
    double s = 0.0, c = 0.0;
    for (int i = 0; i < n; ++i) {
        const double t = s + v[i];
        c += std::fabs(s) >= std::fabs(v[i]) ? (s - t) + v[i] : (v[i] - t) + s;
        s = t;
    }
    return s + c;
}

// modified Bessel function I0 by its power series sum ((x/2)^2)^k / (k!)^2: positive terms only, so no cancellation
double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 1000 && term > 1e-18 * sum; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
    }
    return sum;
}

// numpy.sinc: sin(pi x) / (pi x), with x = 0 replaced by 1e-20
double np_sinc(double x) {
    const double y = M_PI * (x == 0.0 ? 1.0e-20 : x);
    return std::sin(y) / y;
}

}  // namespace

extern "C" int babe_firwin_kaiser(int numtaps, double cutoff, double width, double fs, int highpass, double* taps_out) {
    BABE_CHECK_ARG(taps_out && numtaps >= 1, "firwin_kaiser: bad arguments (numtaps = %d)", numtaps);
    BABE_CHECK_ARG(fs > 0 && width > 0 && std::isfinite(fs) && std::isfinite(width), "firwin_kaiser: fs = %g, width = %g", fs, width);
    const double nyq = 0.5 * fs, c = cutoff / nyq;
    BABE_CHECK_ARG(c > 0 && c < 1, "firwin_kaiser: cutoff = %g outside (0, fs / 2 = %g)", cutoff, nyq);
    BABE_CHECK_ARG(!highpass || (numtaps & 1), "firwin_kaiser: a high-pass with an even number of taps (%d) cannot pass the Nyquist "
                   "frequency", numtaps);
    // kaiser_atten and kaiser_beta
    const double atten = 2.285 * (numtaps - 1) * M_PI * (width / nyq) + 7.95;
    const double beta = atten > 50 ? 0.1102 * (atten - 8.7) : atten > 21 ? 0.5842 * std::pow(atten - 21, 0.4) + 0.07886 * (atten - 21) : 0.0;
    const double left = highpass ? c : 0.0, right = highpass ? 1.0 : c;
    const double alpha = 0.5 * (numtaps - 1), i0b = bessel_i0(beta);
    for (int n = 0; n < numtaps; ++n) {
        const double m = n - alpha;
        double h = 0.0;
        h += right * np_sinc(right * m);
        h -= left * np_sinc(left * m);
        double win = 1.0;                              // (one tap: the window is 1)
        if (numtaps > 1) {
            const double u = (n - alpha) / alpha;
            win = bessel_i0(beta * std::sqrt(1.0 - u * u)) / i0b;
        }
        taps_out[n] = h * win;
    }
    // unit gain at the centre of the pass band: frequency 0, or 1 (Nyquist) for the high-pass
    const double scale_frequency = highpass ? 1.0 : 0.0;
    double* hc = new double[numtaps];
    for (int n = 0; n < numtaps; ++n) hc[n] = taps_out[n] * std::cos(M_PI * (n - alpha) * scale_frequency);
    const double s = compensated_sum(hc, numtaps);
    delete[] hc;
    for (int n = 0; n < numtaps; ++n) taps_out[n] /= s;
    return BABE_OK;
}

extern "C" int babe_iir_check(const float* b, const float* a, int order) {
    BABE_CHECK_ARG(b && a, "iir_check: NULL b or a");
    BABE_CHECK_ARG(order >= 1 && order <= 16, "iir_check: order %d outside 1..16", order);
    BABE_CHECK_ARG(a[0] == 1.0f, "iir_check: a[0] = %g (the coefficients are divided by a[0] first)", (double)a[0]);
    // step-down (Schur-Cohn / Jury): z^N + a1 z^(N-1) + ... + aN has all roots inside the unit circle iff every reflection
    // coefficient k_m = a_m[m] of the recursion a_(m-1)[i] = (a_m[i] - k_m a_m[m - i]) / (1 - k_m^2) is below 1 in modulus
    double p[17], q[17];
    for (int i = 0; i <= order; ++i) {
        BABE_CHECK_ARG(std::isfinite(a[i]) && std::isfinite(b[i]), "iir_check: coefficient %d is not finite", i);
        p[i] = (double)a[i];
    }
    for (int m = order; m >= 1; --m) {
        const double k = p[m];
        BABE_CHECK_ARG(std::fabs(k) < 1.0, "iir_check: unstable at float32 coefficients (reflection coefficient %d is %g: a pole on or "
                       "outside the unit circle)", m, k);
        const double den = 1.0 - k * k;
        for (int i = 0; i < m; ++i) q[i] = (p[i] - k * p[m - i]) / den;
        for (int i = 0; i < m; ++i) p[i] = q[i];
    }
    return BABE_OK;
}
