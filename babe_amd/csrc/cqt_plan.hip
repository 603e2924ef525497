// CQT plan: the band design of the constant-Q transform (NSGT, mode "oct", Kaiser windows) in the LIBRARY, and the whole transforms
// from a plan handle - what a non-Python host needs to run cqt_nsgt_pytorch.CQT_nsgt(numocts, binsoct, "oct", ("kaiser", beta), fs,
// audio_len).fwd / .bwd / .apply_hpf_DC (constructed at networks/cqtdiff+.py:620; used at :743, :841 and
// testing/blind_bwe_sampler.py:156).  Rounds 1-5 kept the design in numpy (babe_amd/cqt.py::design_bands) and the sequencing in Python;
// this file restates both behind the C-ABI:
//   babe_cqt_design_create / _get / _destroy   host only (no GPU call): the tables, float64 / int64, the same arithmetic in the same
//                                              order as design_bands (tests/test_cqt_plan_cpu.py compares them with the numpy tables)
//   babe_cqt_plan_create / _destroy            design + float32 device tables + the mixed-radix plan of the length-L real FFT
//   babe_cqt_design_create_ex / babe_cqt_plan_create_ex     the same with the longest band transform the host takes as an argument
//                                              (4096: what the five-argument entries keep; 8192: segments up to about 754 000 samples)
//   babe_cqt_fwd / _bwd / _fwd_adjoint / _bwd_adjoint / _hpf     the transforms (rfft_L -> band kernels, band kernels -> gather -> rfft_L^T)
// The definition itself (NSGT LogScale, band lengths, Kaiser windows, painless-case dual frame with the mirrored bands, octave-wise
// power-of-two rasterisation) is stated in oracle/nsgt.py and DESIGN.md; the dependency is absent from the reference tree (parity
// unpinned, as for the Python class).
#include "common.h"
#include "workspace.h"
#include "../../include/babe_hip.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

namespace {

// ---- numpy.i0 as numpy computes it (Cephes Chebyshev expansions; numpy/lib/_function_base_impl.py: _chbevl, _i0_1, _i0_2), so that
// the Kaiser windows match the numpy design to the last bit wherever exp() does
const double kI0A[30] = {-0x1.45cb72134d0efp-58, 0x1.33362977da589p-55, -0x1.184eb721ebbb4p-52, 0x1.ee6d893f65ebap-50, -0x1.a5022c297fbebp-47,
                         0x1.59b464b262627p-44, -0x1.1164c62ee1af0p-41, 0x1.9fe2fe19bd324p-39, -0x1.2fc957a946abcp-36, 0x1.a98becc743c10p-34,
                         -0x1.1d4fe13ae9556p-31, 0x1.6d903a454cb34p-29, -0x1.beaf68c0b30abp-27, 0x1.03b769d4d6435p-24, -0x1.1ec638f227f8dp-22,
                         0x1.2bf24978cf4acp-20, -0x1.2866fcba56427p-18, 0x1.13f58be9a2859p-16, -0x1.e2b2659c41d5ap-15, 0x1.8b51b74107cabp-13,
                         -0x1.2e2fd1f15eb52p-11, 0x1.adc758a12100ep-10, -0x1.1b65e201aa849p-8, 0x1.59961f3dde3ddp-7, -0x1.84e9ef121b6f0p-6,
                         0x1.93e8acea8a32dp-5, -0x1.84b70342d06eap-4, 0x1.5f7ac77ac88c0p-3, -0x1.37febc057cd8dp-2, 0x1.5a84e9035a22ap-1};
const double kI0B[25] = {-0x1.0adb754ca8b19p-57, -0x1.646da66119130p-58, 0x1.9be1812d98421p-55, 0x1.3f3dd076041cdp-55, -0x1.4600babd21fe4p-52,
                         -0x1.8aee7d908de38p-52, 0x1.fee7da3eafb1fp-50, 0x1.12a919094e6d7p-48, -0x1.583fe7e65629ap-47, -0x1.75d99cf68bb32p-45,
                         0x1.156ff0d5fc545p-46, 0x1.b1c8c6b83c073p-42, 0x1.94347fa268cecp-41, -0x1.f904303178d66p-40, -0x1.d0fd7357e7bf2p-37,
                         -0x1.1511d08397425p-35, 0x1.a24feabe8004fp-37, 0x1.0f9ccc0f46f75p-31, 0x1.d2c64a9225b87p-29, 0x1.8569280d6d56dp-26,
                         0x1.b8007d9cd616ep-23, 0x1.8412bc101c586p-19, 0x1.20fa378999e52p-14, 0x1.b998ca2e59049p-9, 0x1.9be62aca809cbp-1};

#pragma clang fp contract(off)
double chbevl(double x, const double* vals, int n) {
    double b0 = vals[0], b1 = 0.0, b2 = 0.0;
    for (int i = 1; i < n; ++i) {
        b2 = b1;
        b1 = b0;
        b0 = x * b1 - b2 + vals[i];
    }
    return 0.5 * (b0 - b2);
}
double np_i0(double x) {
    x = std::fabs(x);
    if (x <= 8.0) return std::exp(x) * chbevl(x / 2.0 - 2.0, kI0A, 30);
    return std::exp(x) * chbevl(32.0 / x - 2.0, kI0B, 25) / std::sqrt(x);
}
// Kaiser window of Mk samples centred on the bin: m = -(Mk/2) .. Mk - Mk/2 - 1 (symmetric: .. Mk/2)
std::vector<double> kaiser(long Mk, double beta, bool symmetric) {
    const long lo = -(Mk / 2), hi = symmetric ? Mk / 2 + 1 : Mk - Mk / 2;
    std::vector<double> g((size_t)(hi - lo));
    const double i0b = np_i0(beta);
    for (long m = lo; m < hi; ++m) {
        const double x = 2.0 * (double)m / (double)Mk;
        double arg = 1.0 - x * x;
        if (arg < 0.0) arg = 0.0;
        g[(size_t)(m - lo)] = np_i0(beta * std::sqrt(arg)) / i0b;
    }
    return g;
}
long pos_mod(long a, long L) {
    const long r = a % L;
    return r < 0 ? r + L : r;
}
long next_pow2(long v) {
    if (v < 1) v = 1;
    long p = 1;
    while (p < v) p <<= 1;
    return p;
}

struct CqtDesign {
    double fs = 0, beta = 0;
    long L = 0;
    int numocts = 0, binsoct = 0, nb = 0;
    long nwin = 0, M_dc = 0;
    std::vector<long> M, c, T, woff, idx, rowptr, src;        // src: entry index, minus 2^31 when the entry is conjugated (mirror)
    std::vector<double> f, Om, g, gdual, Tw, hpf;             // hpf: bins 0 .. L/2
    // the length-L real FFT (four-step N1 x N2, csrc/fft_mixed.hip)
    long N1 = 0, N2 = 0, K2 = 0, KX = 0;
    std::vector<int> rad1, rad2;
    // workgroup table of the band kernels: 4096 points (4096 / T bands of one octave) each, an 8192-point band alone
    std::vector<int> wg_first, wg_count;
    std::vector<int> T_oct;
    int kdeg = 0;
    double kpoly[12] = {0};
    std::string error;
};

// L = N1 * N2, N1 <= N2 as balanced as possible, both multiples of 4 preferred (babe_amd/cqt.py::factor_len)
bool factor_len(long L, long& N1, long& N2) {
    long b1 = 0, b2 = 0, q1 = 0, q2 = 0;
    for (long a = 1; a * a <= L; ++a)
        if (L % a == 0) {
            b1 = a;
            b2 = L / a;
            if (a % 4 == 0 && (L / a) % 4 == 0 && 4 * (L / a) <= 5 * a) {
                q1 = a;
                q2 = L / a;
            }
        }
    N1 = q1 ? q1 : b1;
    N2 = q1 ? q2 : b2;
    return N2 <= 4096;
}
// N as a product of at most 6 radices of csrc/fft_mixed.hip (4 preferred over 2 x 2, large radices last); empty: none
std::vector<int> small_radices(long N) {
    std::vector<int> out;
    long n = N;
    const int rs[8] = {4, 2, 3, 5, 7, 11, 13, 23};
    for (int r : rs)
        while (n % r == 0 && !(r == 2 && n % 4 == 0)) {
            out.push_back(r);
            n /= r;
        }
    if (n != 1 || out.empty() || out.size() > 6) out.clear();
    return out;
}

// babe_amd/cqt.py::design_bands, operation for operation (float64; sums in the same order)
// max_band: the longest band transform the caller takes, 4096 or 8192 points
CqtDesign* design(double fs, long L, int numocts, int binsoct, double beta, int max_band) {
    CqtDesign* d = new CqtDesign;
    d->fs = fs, d->L = L, d->numocts = numocts, d->binsoct = binsoct, d->beta = beta;
    if (max_band != 4096 && max_band != 8192) {
        d->error = "cqt design: max_band must be 4096 or 8192 (got " + std::to_string(max_band) + ")";
        return d;
    }
    if (L < 16 || L % 2 != 0 || numocts < 1 || numocts > 8 || binsoct < 2 || binsoct > 255 || !(fs > 0) || !(beta >= 0)) {
        d->error = "cqt design: need an even audio length, 1..8 octaves, 2..255 bins per octave";
        return d;
    }
    const int nb = numocts * binsoct;
    d->nb = nb;
    const double fmax = fs / 2.0 - 1e-6;
    const double fmin = fmax / std::pow(2.0, (double)numocts);
    const double r = std::pow(2.0, (double)numocts / ((double)nb - 1.0));
    d->f.resize(nb), d->Om.resize(nb);
    for (int k = 0; k < nb; ++k) {
        d->f[k] = fmin * std::pow(r, (double)k);
        d->Om[k] = d->f[k] * (double)L / fs;
    }
    const double Q = std::sqrt(r) / (r - 1.0) / 2.0;
    d->M.assign(nb, 0), d->c.assign(nb, 0), d->T.assign(nb, 0), d->woff.assign(nb, 0);
    for (int k = 1; k + 1 < nb; ++k) d->M[k] = (long)std::nearbyint(d->Om[k + 1] - d->Om[k - 1]);      // (np.round: half to even)
    d->M[0] = (long)std::nearbyint(d->Om[0] / Q);
    d->M[nb - 1] = (long)std::nearbyint(d->Om[nb - 1] / Q);
    for (int k = 0; k < nb; ++k) {
        if (d->M[k] < 4) d->M[k] = 4;
        d->c[k] = (long)std::nearbyint(d->Om[k]);
    }
    d->c[nb - 1] = (long)std::nearbyint((d->Om[nb - 2] + (double)L / 2.0) / 2.0);
    d->M_dc = std::max((long)std::nearbyint(2.0 * d->Om[0]), 4L);
    const long M_ny = 4;
    d->T_oct.resize(numocts);
    for (int j = 0; j < numocts; ++j) {
        long mx = 0;
        for (int k = j * binsoct; k < (j + 1) * binsoct; ++k) mx = std::max(mx, d->M[k]);
        const long T = next_pow2(mx);
        for (int k = j * binsoct; k < (j + 1) * binsoct; ++k) d->T[k] = T;
        d->T_oct[j] = (int)T;
        if (T > max_band || T < 4) {
            d->error = max_band == 4096 ? "cqt design: a band is longer than the 4096-point band FFT supports"
                                        : "cqt design: a band is longer than the 8192-point band FFT supports";
            return d;
        }
    }
    long nwin = 0;
    for (int k = 0; k < nb; ++k) {
        d->woff[k] = nwin;
        nwin += d->M[k];
    }
    d->nwin = nwin;
    d->g.assign(nwin, 0.0), d->idx.assign(nwin, 0), d->Tw.assign(nwin, 0.0);
    std::vector<double> diag((size_t)L, 0.0), lp((size_t)L, 0.0);
    for (int k = 0; k < nb; ++k) {
        const std::vector<double> gk = kaiser(d->M[k], beta, false);
        const long Mk = d->M[k], lo = -(Mk / 2);
        for (long i = 0; i < Mk; ++i) {
            const long ii = pos_mod(d->c[k] + lo + i, L);
            d->g[d->woff[k] + i] = gk[i];
            d->idx[d->woff[k] + i] = ii;
            d->Tw[d->woff[k] + i] = (double)d->T[k];
        }
        for (long i = 0; i < Mk; ++i) diag[d->idx[d->woff[k] + i]] += (double)d->T[k] * gk[i] * gk[i];             // np.add.at, in order
        for (long i = 0; i < Mk; ++i) diag[pos_mod(-d->idx[d->woff[k] + i], L)] += (double)d->T[k] * gk[i] * gk[i];
    }
    {
        const std::vector<double> gd = kaiser(d->M_dc, beta, true);
        const long h = d->M_dc / 2;
        for (long i = 0; i < 2 * h + 1; ++i) lp[pos_mod(-h + i, L)] += (double)d->M_dc * gd[i] * gd[i];
        const std::vector<double> gn = kaiser(M_ny, beta, true);
        const long hn = M_ny / 2;
        for (long i = 0; i < 2 * hn + 1; ++i) lp[pos_mod(L / 2 - hn + i, L)] += (double)M_ny * gn[i] * gn[i];
    }
    for (long n = 0; n < L; ++n) {
        diag[n] += lp[n];
        if (!(diag[n] > 0)) {
            d->error = "cqt design: the frame has a hole (a spectral bin no window covers)";
            return d;
        }
    }
    d->gdual.resize(nwin);
    for (long e = 0; e < nwin; ++e) d->gdual[e] = d->g[e] / diag[d->idx[e]];
    d->hpf.resize(L / 2 + 1);
    for (long n = 0; n <= L / 2; ++n) d->hpf[n] = 1.0 - lp[n] / diag[n];
    // CSR over n in [0, L/2]: the window samples landing on n directly or through the mirror, stable in entry order
    std::vector<long> tgt(nwin);
    d->rowptr.assign(L / 2 + 2, 0);
    for (long e = 0; e < nwin; ++e) {
        tgt[e] = d->idx[e] <= L / 2 ? d->idx[e] : L - d->idx[e];
        d->rowptr[tgt[e] + 1] += 1;
    }
    for (long n = 0; n <= L / 2; ++n) d->rowptr[n + 1] += d->rowptr[n];
    d->src.resize(nwin);
    {
        std::vector<long> fill(d->rowptr.begin(), d->rowptr.end() - 1);
        for (long e = 0; e < nwin; ++e) d->src[fill[tgt[e]]++] = d->idx[e] > L / 2 ? e - (1L << 31) : e;
    }
    // length-L real FFT
    if (!factor_len(L, d->N1, d->N2)) {
        d->error = "cqt design: the audio length has no balanced factorisation N1 x N2 with N2 <= 4096";
        return d;
    }
    d->K2 = (L / 2) / d->N1 + 1;
    d->KX = d->K2 * d->N1;
    d->rad1 = small_radices(d->N1), d->rad2 = small_radices(d->N2);
    if (d->rad1.empty() || d->rad2.empty() || std::max(d->N1, d->N2) > 1077) {
        d->error = "cqt design: the factors of the audio length are not products of the radices 2,3,4,5,7,11,13,23 (mixed-radix FFT)";
        return d;
    }
    // band-kernel workgroup table
    for (int j = 0; j < numocts; ++j) {
        const int bpw = std::min(binsoct, std::max(1, 4096 / d->T_oct[j]));
        for (int s0 = 0; s0 < binsoct; s0 += bpw) {
            d->wg_first.push_back(j * binsoct + s0);
            d->wg_count.push_back(std::min(bpw, binsoct - s0));
        }
    }
    // analytic Kaiser window of the band kernels (babe_cqt_bands::kpoly): truncated I0 series, first dropped term < 1e-9
    {
        const double q = beta * beta / 4.0;
        std::vector<double> terms{1.0};
        double t = 1.0;
        bool ok = true;
        for (int j = 1;; ++j) {
            t = t * q / ((double)j * (double)j);
            if (t < 1e-9) break;
            terms.push_back(t);
            if (j > 11) {
                ok = false;
                break;
            }
        }
        if (ok) {
            d->kdeg = std::max((int)terms.size() - 1, 1);
            const double i0b = np_i0(beta);
            for (size_t j = 0; j < terms.size(); ++j) d->kpoly[j] = terms[j] / i0b;
        }
    }
    return d;
}

template <typename Tv>
long copy_out(const std::vector<Tv>& v, void* out, long cap) {
    const long bytes = (long)(v.size() * sizeof(Tv));
    if (out && cap >= bytes) std::memcpy(out, v.data(), (size_t)bytes);
    return bytes;
}

// ---- the plan: device tables + FFT plan
struct CqtPlan {
    CqtDesign* d = nullptr;
    int device = 0;
    // device tables (one allocation)
    char* dev = nullptr;
    size_t dev_bytes = 0;
    int *c, *M, *woff, *log2T, *oct, *binoct, *wg_first, *wg_count, *wg_rec, *band_rec, *rowptr, *src, *rec;
    float *tw4096, *win_fwd, *win_bwd, *win_bwd_adj, *hpf_irfft, *w1, *w2, *tw;
    bool has_rec = false;
    int max_wg = 0, min_l2 = 0, max_l2 = 0;
    long sum_T = 0, sum_M = 0;
    double sum_TlogT = 0;
};

void fill_bands(const CqtPlan* p, babe_cqt_bands* b, float* const* coef) {
    const CqtDesign* d = p->d;
    std::memset(b, 0, sizeof(*b));
    b->nbands = d->nb, b->L = (int)d->L, b->KX = (int)d->KX;
    b->c = p->c, b->M = p->M, b->woff = p->woff, b->log2T = p->log2T, b->oct = p->oct, b->binoct = p->binoct, b->tw4096 = p->tw4096;
    b->nocts = d->numocts, b->binsoct = d->binsoct;
    for (int j = 0; j < d->numocts; ++j) b->coef[j] = coef[j];
    b->wg_first = p->wg_first, b->wg_count = p->wg_count, b->nwg = (int)d->wg_first.size();
    b->wg_rec = p->wg_rec, b->band_rec = p->band_rec;
    b->max_wg_count = p->max_wg, b->min_log2T = p->min_l2, b->max_log2T = p->max_l2;
    b->sum_T = p->sum_T, b->sum_M = p->sum_M, b->sum_TlogT = p->sum_TlogT;
    b->kdeg = d->kdeg;
    for (int j = 0; j < 12; ++j) b->kpoly[j] = (float)d->kpoly[j];
}

int ilog2(long v) {
    int l = 0;
    while ((1L << l) < v) ++l;
    return l;
}

}  // namespace

extern "C" void* babe_cqt_design_create_ex(double fs, int audio_len, int numocts, int binsoct, double beta, int max_band) {
    CqtDesign* d = design(fs, (long)audio_len, numocts, binsoct, beta, max_band);
    if (!d->error.empty()) {
        babe_set_error("%s (fs = %g, audio_len = %d, numocts = %d, binsoct = %d, beta = %g)", d->error.c_str(), fs, audio_len, numocts,
                       binsoct, beta);
        delete d;
        return nullptr;
    }
    return d;
}
extern "C" void* babe_cqt_design_create(double fs, int audio_len, int numocts, int binsoct, double beta) {
    return babe_cqt_design_create_ex(fs, audio_len, numocts, binsoct, beta, 4096);
}
extern "C" void babe_cqt_design_destroy(void* design) { delete static_cast<CqtDesign*>(design); }

/* Copies table `name` into out (capacity cap bytes) and returns its size in bytes (call with out = NULL for the size); -1: unknown
 * name.  int64: M c T woff idx rowptr src;  float64: f Om g gdual Tw hpf kpoly;  int32: rad1 rad2 wg_first wg_count T_oct;
 * scalars as one int64: nb nwin M_dc N1 N2 K2 KX kdeg. */
extern "C" long babe_cqt_design_get(const void* design, const char* name, void* out, long cap) {
    if (!design || !name) return -1;
    const CqtDesign* d = static_cast<const CqtDesign*>(design);
    const std::string n(name);
    if (n == "M") return copy_out(d->M, out, cap);
    if (n == "c") return copy_out(d->c, out, cap);
    if (n == "T") return copy_out(d->T, out, cap);
    if (n == "woff") return copy_out(d->woff, out, cap);
    if (n == "idx") return copy_out(d->idx, out, cap);
    if (n == "rowptr") return copy_out(d->rowptr, out, cap);
    if (n == "src") return copy_out(d->src, out, cap);
    if (n == "f") return copy_out(d->f, out, cap);
    if (n == "Om") return copy_out(d->Om, out, cap);
    if (n == "g") return copy_out(d->g, out, cap);
    if (n == "gdual") return copy_out(d->gdual, out, cap);
    if (n == "Tw") return copy_out(d->Tw, out, cap);
    if (n == "hpf") return copy_out(d->hpf, out, cap);
    if (n == "rad1") return copy_out(d->rad1, out, cap);
    if (n == "rad2") return copy_out(d->rad2, out, cap);
    if (n == "wg_first") return copy_out(d->wg_first, out, cap);
    if (n == "wg_count") return copy_out(d->wg_count, out, cap);
    if (n == "T_oct") return copy_out(d->T_oct, out, cap);
    if (n == "kpoly") return copy_out(std::vector<double>(d->kpoly, d->kpoly + 12), out, cap);
    long v = -1;
    if (n == "nb") v = d->nb;
    else if (n == "nwin") v = d->nwin;
    else if (n == "M_dc") v = d->M_dc;
    else if (n == "N1") v = d->N1;
    else if (n == "N2") v = d->N2;
    else if (n == "K2") v = d->K2;
    else if (n == "KX") v = d->KX;
    else if (n == "kdeg") v = d->kdeg;
    else return -1;
    return copy_out(std::vector<long>{v}, out, cap);
}

extern "C" void* babe_cqt_plan_create(double fs, int audio_len, int numocts, int binsoct, double beta) {
    return babe_cqt_plan_create_ex(fs, audio_len, numocts, binsoct, beta, 4096);
}
extern "C" void* babe_cqt_plan_create_ex(double fs, int audio_len, int numocts, int binsoct, double beta, int max_band) {
    CqtDesign* d = static_cast<CqtDesign*>(babe_cqt_design_create_ex(fs, audio_len, numocts, binsoct, beta, max_band));
    if (!d) return nullptr;
    CqtPlan* p = new CqtPlan;
    p->d = d;
    const long L = d->L, nb = d->nb, nwin = d->nwin, N1 = d->N1, N2 = d->N2;
    const int nwg = (int)d->wg_first.size();
    // ---- host images of the device tables
    std::vector<int> hc(nb), hM(nb), hwoff(nb), hl2(nb), hoct(nb), hbin(nb), hwgrec(4 * nwg), hbrec(4 * nb), hrow(L / 2 + 2), hsrc(nwin);
    for (long k = 0; k < nb; ++k) {
        hc[k] = (int)d->c[k], hM[k] = (int)d->M[k], hwoff[k] = (int)d->woff[k], hl2[k] = ilog2(d->T[k]);
        hoct[k] = (int)(k / d->binsoct), hbin[k] = (int)(k % d->binsoct);
        hbrec[4 * k] = hc[k], hbrec[4 * k + 1] = hM[k], hbrec[4 * k + 2] = hwoff[k], hbrec[4 * k + 3] = 0;
        p->sum_T += d->T[k], p->sum_M += d->M[k], p->sum_TlogT += (double)d->T[k] * hl2[k];
    }
    p->min_l2 = *std::min_element(hl2.begin(), hl2.end()), p->max_l2 = *std::max_element(hl2.begin(), hl2.end());
    for (int w = 0; w < nwg; ++w) {
        const int f = d->wg_first[w];
        hwgrec[4 * w] = f, hwgrec[4 * w + 1] = d->wg_count[w], hwgrec[4 * w + 2] = hl2[f];
        hwgrec[4 * w + 3] = (f / d->binsoct) | ((f % d->binsoct) << 8);
        p->max_wg = std::max(p->max_wg, d->wg_count[w]);
    }
    for (long n = 0; n < L / 2 + 2; ++n) hrow[n] = (int)d->rowptr[n];
    for (long e = 0; e < nwin; ++e) hsrc[e] = (int)d->src[e];          // (e - 2^31 as int32 = e with the sign bit set: the kernel's conjugate flag)
    // fixed 16-byte records {src0, src1, src2, count} when no bin has more than three sources
    std::vector<int> hrec;
    long maxcnt = 0;
    for (long n = 0; n <= L / 2; ++n) maxcnt = std::max(maxcnt, d->rowptr[n + 1] - d->rowptr[n]);
    p->has_rec = maxcnt <= 3;
    if (p->has_rec) {
        hrec.assign(4 * (L / 2 + 1), 0);
        for (long n = 0; n <= L / 2; ++n) {
            const long cnt = d->rowptr[n + 1] - d->rowptr[n];
            for (long e = 0; e < cnt; ++e) hrec[4 * n + e] = hsrc[d->rowptr[n] + e];
            hrec[4 * n + 3] = (int)cnt;
        }
    }
    std::vector<float> htw4096(4096), hwf(nwin), hwb(nwin), hwba(nwin), hhpf(L / 2 + 1), hw1(2 * N1), hw2(2 * N2), htw(2 * N1 * N2);
    for (int q = 0; q < 2048; ++q) {
        const double a = 2.0 * M_PI * (double)q / 4096.0;
        htw4096[2 * q] = (float)std::cos(a), htw4096[2 * q + 1] = (float)(-std::sin(a));
    }
    for (long e = 0; e < nwin; ++e) {
        hwf[e] = (float)(d->g[e] / d->Tw[e]);
        hwb[e] = (float)(d->gdual[e] * d->Tw[e]);
        hwba[e] = (float)(d->gdual[e] * d->Tw[e] * (2.0 / (double)L));
    }
    for (long n = 0; n <= L / 2; ++n) hhpf[n] = (float)(d->hpf[n] * ((n == 0 || n == L / 2) ? 1.0 / (double)L : 2.0 / (double)L));
    for (long j = 0; j < N1; ++j) {
        const double a = 2.0 * M_PI * (double)j / (double)N1;
        hw1[2 * j] = (float)std::cos(a), hw1[2 * j + 1] = (float)(-std::sin(a));
    }
    for (long j = 0; j < N2; ++j) {
        const double a = 2.0 * M_PI * (double)j / (double)N2;
        hw2[2 * j] = (float)std::cos(a), hw2[2 * j + 1] = (float)(-std::sin(a));
    }
    for (long k1 = 0; k1 < N1; ++k1)
        for (long n2 = 0; n2 < N2; ++n2) {
            const double a = 2.0 * M_PI * (double)((k1 * n2) % L) / (double)L;
            htw[2 * (k1 * N2 + n2)] = (float)std::cos(a), htw[2 * (k1 * N2 + n2) + 1] = (float)(-std::sin(a));
        }
    // ---- one device allocation, each table 256-byte aligned
    struct Piece { const void* h; size_t bytes; void** dst; };
    std::vector<Piece> tables = {
        {hc.data(), hc.size() * 4, (void**)&p->c}, {hM.data(), hM.size() * 4, (void**)&p->M}, {hwoff.data(), hwoff.size() * 4, (void**)&p->woff},
        {hl2.data(), hl2.size() * 4, (void**)&p->log2T}, {hoct.data(), hoct.size() * 4, (void**)&p->oct}, {hbin.data(), hbin.size() * 4, (void**)&p->binoct},
        {d->wg_first.data(), d->wg_first.size() * 4, (void**)&p->wg_first}, {d->wg_count.data(), d->wg_count.size() * 4, (void**)&p->wg_count},
        {hwgrec.data(), hwgrec.size() * 4, (void**)&p->wg_rec}, {hbrec.data(), hbrec.size() * 4, (void**)&p->band_rec},
        {hrow.data(), hrow.size() * 4, (void**)&p->rowptr}, {hsrc.data(), hsrc.size() * 4, (void**)&p->src},
        {hrec.data(), hrec.size() * 4, (void**)&p->rec}, {htw4096.data(), htw4096.size() * 4, (void**)&p->tw4096},
        {hwf.data(), hwf.size() * 4, (void**)&p->win_fwd}, {hwb.data(), hwb.size() * 4, (void**)&p->win_bwd},
        {hwba.data(), hwba.size() * 4, (void**)&p->win_bwd_adj}, {hhpf.data(), hhpf.size() * 4, (void**)&p->hpf_irfft},
        {hw1.data(), hw1.size() * 4, (void**)&p->w1}, {hw2.data(), hw2.size() * 4, (void**)&p->w2}, {htw.data(), htw.size() * 4, (void**)&p->tw}};
    size_t total = 0;
    for (auto& pc : tables) total += (pc.bytes + 255) / 256 * 256;
    if (hipGetDevice(&p->device) != hipSuccess || hipMalloc((void**)&p->dev, total) != hipSuccess) {
        babe_set_error("cqt_plan_create: cannot allocate %zu bytes of device tables: %s", total, hipGetErrorString(hipGetLastError()));
        delete d;
        delete p;
        return nullptr;
    }
    p->dev_bytes = total;
    size_t off = 0;
    for (auto& pc : tables) {
        *pc.dst = pc.bytes ? (void*)(p->dev + off) : nullptr;
        if (pc.bytes && hipMemcpy(p->dev + off, pc.h, pc.bytes, hipMemcpyHostToDevice) != hipSuccess) {
            babe_set_error("cqt_plan_create: table upload failed: %s", hipGetErrorString(hipGetLastError()));
            (void)hipFree(p->dev);
            delete d;
            delete p;
            return nullptr;
        }
        off += (pc.bytes + 255) / 256 * 256;
    }
    return p;
}

extern "C" void babe_cqt_plan_destroy(void* plan) {
    CqtPlan* p = static_cast<CqtPlan*>(plan);
    if (!p) return;
    if (p->dev) (void)hipFree(p->dev);
    delete p->d;
    delete p;
}

extern "C" const void* babe_cqt_plan_design(const void* plan) { return plan ? static_cast<const CqtPlan*>(plan)->d : nullptr; }
// bytes of the plan's device tables, for the owner of a plan inside this library (csrc/model.hip: babe_model_info)
size_t babe_cqt_plan_table_bytes(const void* plan) { return plan ? static_cast<const CqtPlan*>(plan)->dev_bytes : 0; }

namespace {
// scratch of one transform call with B clips, whole floats: spectrum [B][2][KX], four-step intermediate [B][2][L], band spectra
// [B][nwin][2] (bwd / fwd_adjoint only; carved for all so that one buffer serves every call)
struct Work { float *spec, *four, *bs; };
Work carve(Carver& c, const CqtDesign* d, int B) {
    Work w;
    w.spec = c.take<float>((size_t)B * 2 * d->KX);
    w.four = c.take<float>((size_t)B * 2 * d->L);
    w.bs = c.take<float>((size_t)B * 2 * d->nwin);
    return w;
}
// the entry points take no size: the caller's buffer has babe_cqt_workspace_bytes(plan, B) bytes by contract
Work carve(const CqtDesign* d, float* ws, int B) {
    Carver c{reinterpret_cast<char*>(ws), (size_t)-1, 4};
    return carve(c, d, B);
}
int rfft(const CqtPlan* p, const float* x, float* spec, float* four, int B, void* stream) {
    const CqtDesign* d = p->d;
    return babe_rfft_mixed(x, spec, nullptr, nullptr, four, B, (int)d->N1, (int)d->N2, (int)d->K2, d->rad1.data(), (int)d->rad1.size(), d->rad2.data(),
                           (int)d->rad2.size(), p->w1, p->w2, p->tw, 0, stream);
}
int rfft_T(const CqtPlan* p, const float* spec, float* x, float* four, int B, void* stream) {
    const CqtDesign* d = p->d;
    return babe_rfft_mixed(nullptr, nullptr, spec, x, four, B, (int)d->N1, (int)d->N2, (int)d->K2, d->rad1.data(), (int)d->rad1.size(), d->rad2.data(),
                           (int)d->rad2.size(), p->w1, p->w2, p->tw, 1, stream);
}
int synth(const CqtPlan* p, float* const* coef, const float* win, float scale, const Work& w, int B, void* stream) {
    const CqtDesign* d = p->d;
    babe_cqt_bands b;
    fill_bands(p, &b, coef);
    BABE_TRY(babe_cqt_band_synthesis(&b, w.bs, win, d->nwin, B, stream));
    return babe_cqt_gather(w.bs, d->nwin, p->rowptr, p->src, p->has_rec ? p->rec : nullptr, w.spec, (int)d->KX, (int)d->L, scale, nullptr, B, stream);
}
bool plan_args(const void* plan, const void* a, const void* b, const void* ws, int B, const char* who) {
    if (!plan || !a || !b || !ws || B < 1) {
        babe_set_error("%s: bad arguments", who);
        return false;
    }
    return true;
}
}  // namespace

/* The carve's dry total and 1024 bytes. */
extern "C" long babe_cqt_workspace_bytes(const void* plan, int B) {
    if (!plan || B < 1) return -1;
    Carver dry{nullptr, 0, 4};
    carve(dry, static_cast<const CqtPlan*>(plan)->d, B);
    return (long)dry.used + 1024;
}

/* CQT_nsgt.fwd: x [B][L] -> planar coefficients coef[j] = [B][2][binsoct][T_oct[j]] (index 0 = lowest octave).  ws: device scratch of
 * babe_cqt_workspace_bytes(plan, B) bytes. */
extern "C" int babe_cqt_fwd(const void* plan, const float* x, float* const* coef, float* ws, int B, void* stream) {
    if (!plan_args(plan, x, coef, ws, B, "cqt_fwd")) return BABE_ERR_ARG;
    const CqtPlan* p = static_cast<const CqtPlan*>(plan);
    const Work w = carve(p->d, ws, B);
    BABE_TRY(rfft(p, x, w.spec, w.four, B, stream));
    babe_cqt_bands b;
    fill_bands(p, &b, coef);
    return babe_cqt_band_analysis(&b, w.spec, p->d->kdeg > 0 ? nullptr : p->win_fwd, B, stream);
}
/* CQT_nsgt.bwd: planar coefficients -> x [B][L] */
extern "C" int babe_cqt_bwd(const void* plan, float* const* coef, float* x, float* ws, int B, void* stream) {
    if (!plan_args(plan, coef, x, ws, B, "cqt_bwd")) return BABE_ERR_ARG;
    const CqtPlan* p = static_cast<const CqtPlan*>(plan);
    const Work w = carve(p->d, ws, B);
    BABE_TRY(synth(p, coef, p->win_bwd, (float)(2.0 / (double)p->d->L), w, B, stream));
    return rfft_T(p, w.spec, x, w.four, B, stream);
}
/* transpose of babe_cqt_fwd: gradients w.r.t. the coefficients -> gradient w.r.t. x */
extern "C" int babe_cqt_fwd_adjoint(const void* plan, float* const* gcoef, float* gx, float* ws, int B, void* stream) {
    if (!plan_args(plan, gcoef, gx, ws, B, "cqt_fwd_adjoint")) return BABE_ERR_ARG;
    const CqtPlan* p = static_cast<const CqtPlan*>(plan);
    const Work w = carve(p->d, ws, B);
    BABE_TRY(synth(p, gcoef, p->d->kdeg > 0 ? nullptr : p->win_fwd, 1.0f, w, B, stream));
    return rfft_T(p, w.spec, gx, w.four, B, stream);
}
/* transpose of babe_cqt_bwd: gradient w.r.t. x -> gradients w.r.t. the coefficients */
extern "C" int babe_cqt_bwd_adjoint(const void* plan, const float* gx, float* const* gcoef, float* ws, int B, void* stream) {
    if (!plan_args(plan, gx, gcoef, ws, B, "cqt_bwd_adjoint")) return BABE_ERR_ARG;
    const CqtPlan* p = static_cast<const CqtPlan*>(plan);
    const Work w = carve(p->d, ws, B);
    BABE_TRY(rfft(p, gx, w.spec, w.four, B, stream));
    babe_cqt_bands b;
    fill_bands(p, &b, gcoef);
    return babe_cqt_band_analysis(&b, w.spec, p->win_bwd_adj, B, stream);
}
/* CQT_nsgt.apply_hpf_DC: zero-phase removal of the DC and Nyquist bands (self-adjoint), x [B][L] -> out [B][L] (may alias x) */
extern "C" int babe_cqt_hpf(const void* plan, const float* x, float* out, float* ws, int B, void* stream) {
    if (!plan_args(plan, x, out, ws, B, "cqt_hpf")) return BABE_ERR_ARG;
    const CqtPlan* p = static_cast<const CqtPlan*>(plan);
    const CqtDesign* d = p->d;
    const Work w = carve(d, ws, B);
    BABE_TRY(rfft(p, x, w.spec, w.four, B, stream));
    BABE_TRY(babe_spec_scale(w.spec, nullptr, w.spec, p->hpf_irfft, (int)d->KX, (int)d->L, 1.0f, 0.0f, B, stream));
    return rfft_T(p, w.spec, out, w.four, B, stream);
}
