// Host-only parts of the file-level flow with the denoiser pre-pass (csrc/dn_engine.hip wraps them as C-ABI entries): the sinc
// table of babe_amd/resample.py, the walk of DenoiserPrepass.apply_denoiser, the rate plan of long_file.rate_plan, and what a
// denoiser weights file (babe_amd/model_file.py::export_denoiser) must hold.  Plain C++17, no HIP: tools/dn_host_check.cpp
// compiles it with a host compiler under the sanitizers.
#pragma once
#include <cmath>
#include <numeric>
#include "model_file.h"

namespace babe_dn {

// ------------------------------------------------------------------------------------------------------------ the sinc table
// resample.py::sinc_resample_kernel is float32 arithmetic on tensors, one rounding per operation; the functions below restate
// it operation by operation.  A fused multiply-add would skip a rounding, so contraction is off for them.
#if defined(__clang__)
#define BABE_DN_NO_CONTRACT _Pragma("clang fp contract(off)")
#define BABE_DN_NO_CONTRACT_ATTR
#elif defined(__GNUC__)
#define BABE_DN_NO_CONTRACT
#define BABE_DN_NO_CONTRACT_ATTR __attribute__((optimize("fp-contract=off")))
#else
#define BABE_DN_NO_CONTRACT
#define BABE_DN_NO_CONTRACT_ATTR
#endif

constexpr int LOWPASS_WIDTH = 6;
constexpr double ROLLOFF = 0.99;
constexpr long MAX_RATE = 1 << 20;

struct SincDims {
    int width, orig, new_;
    double base_freq;
};
// the two rates divided by their gcd and the table's half width; false: a rate that is not positive or too large
inline bool sinc_dims(long orig_freq, long new_freq, SincDims& d) {
    if (orig_freq < 1 || new_freq < 1 || orig_freq > MAX_RATE || new_freq > MAX_RATE) return false;
    const long g = std::gcd(orig_freq, new_freq);
    d.orig = (int)(orig_freq / g), d.new_ = (int)(new_freq / g);
    d.base_freq = (double)(d.orig < d.new_ ? d.orig : d.new_) * ROLLOFF;
    d.width = (int)std::ceil((double)(LOWPASS_WIDTH * (long)d.orig) / d.base_freq);
    return true;
}

// kernel [new_][2 width + orig], krange [new_][2] (first and one-past-last tap with |t| < 6; 0, 0 for a phase without one)
BABE_DN_NO_CONTRACT_ATTR inline void sinc_table(const SincDims& d, float* kernel, int* krange) {
    BABE_DN_NO_CONTRACT
    const int taps = 2 * d.width + d.orig;
    const float forig = (float)d.orig, fnew = (float)d.new_, base = (float)d.base_freq, lim = (float)LOWPASS_WIDTH;
    const float pi = (float)M_PI, scale = (float)(d.base_freq / (double)d.orig);
    for (int j = 0; j < d.new_; ++j) {
        const float phase = (float)(-j) / fnew;
        int first = 0, last = 0;
        bool any = false;
        for (int k = 0; k < taps; ++k) {
            const float idx = (float)(k - d.width) / forig;
            float t = phase + idx;
            t = t * base;
            if (std::fabs(t) < lim) {
                if (!any) first = k;
                any = true, last = k + 1;
            }
            t = t < -lim ? -lim : (t > lim ? lim : t);
            float a = t * pi;
            a = a / lim;
            a = a / 2.0f;
            const float c = cosf(a);
            const float window = c * c;
            t = t * pi;
            const float s = t == 0.0f ? 1.0f : sinf(t) / t;
            const float ws = window * scale;
            kernel[(size_t)j * taps + k] = s * ws;
        }
        krange[2 * j] = first, krange[2 * j + 1] = last;
    }
}

// resample.py::resampled_length: the quotient is rounded to double, then to float32, then taken to the next integer
inline long resampled_length(long L, long orig_freq, long new_freq) {
    const long g = std::gcd(orig_freq, new_freq);
    const long orig = orig_freq / g, new_ = new_freq / g;
    return (long)std::ceil((float)((double)(new_ * L) / (double)orig));
}

// ------------------------------------------------------------------------------------------------------------------- the walks
// DenoiserPrepass.apply_denoiser: full segments while start + segment < n, hopping by segment - overlap, then one padded
// remainder.  Returns the number of segments (starts filled up to max), -1 where the Python walk raises: a remainder longer
// than segment - overlap after a first full segment - and for arguments it has no walk for.
inline long denoise_plan(long n, long segment, long overlap, long* starts, long max) {
    if (n < 1 || overlap < 1 || segment < 2 * overlap || max < 0) return -1;
    long count = 0, p = 0;
    while (p + segment < n) {
        if (starts && count < max) starts[count] = p;
        ++count;
        p += segment - overlap;
    }
    if (p != 0 && n - p > segment - overlap) return -1;
    if (starts && count < max) starts[count] = p;
    return count + 1;
}

// long_file.rate_plan: lengths = {the file, the signal the denoiser sees, the signal handed to the model}.  Returns bit 0: the
// conversion before the denoiser (without one: file rate -> model rate) takes place, bit 1: the one after it; -1: bad arguments.
// With a denoiser BOTH conversions hang on fs_file != fs_denoiser (a file at the denoiser's rate reaches the model unconverted).
inline int file_plan(long Lfile, long fs_file, long fs_denoiser, long fs_model, long* lengths) {
    if (Lfile < 1 || fs_file < 1 || fs_model < 1 || fs_denoiser < 0 || fs_file > MAX_RATE || fs_model > MAX_RATE || fs_denoiser > MAX_RATE ||
        Lfile > (1L << 40))
        return -1;
    int mask = 0;
    long a = Lfile, b = Lfile;
    if (fs_denoiser == 0) {
        if (fs_file != fs_model) mask = 1, a = b = resampled_length(Lfile, fs_file, fs_model);
    } else if (fs_file != fs_denoiser) {
        mask = 1, a = b = resampled_length(Lfile, fs_file, fs_denoiser);
        if (fs_denoiser != fs_model) mask |= 2, b = resampled_length(a, fs_denoiser, fs_model);
    }
    if (lengths) lengths[0] = Lfile, lengths[1] = a, lengths[2] = b;
    return mask;
}

// The split-K rule of the denoiser's convolutions (networks/denoiser.py::_split_k): planes too small to fill the GPU split the
// input channels over several workgroups per tile.  Returns the number of splits, 1: none.
inline int ksplit(int B, int Cin, int Cout, int OH, int OW, int KH, int KW) {
    const long tiles = (long)((OH + 3) / 4) * ((OW + 63) / 64) * ((Cout + 63) / 64) * B;
    const long chunks = (KH != 1 || KW != 1) ? (long)((Cin + 31) / 32) * 4 : (Cin + 31) / 32;
    long ks = 512 / tiles;
    if (ks < 1) ks = 1;
    if (ks > chunks) ks = chunks;
    if (ks > 32) ks = 32;
    return (ks <= 1 || chunks < 8) ? 1 : (int)ks;
}

// ------------------------------------------------------------------------------------------------------------ the weights file
constexpr int NS[7] = {64, 64, 64, 128, 128, 256, 512};         // networks/denoiser.py
constexpr int FADE = 1024;                                       // the cross-fade of apply_denoiser, samples

struct DnCfg {
    int depth = 0, num_tfc = 0, num_stages = 0, use_sam = 0, fenc = 0, f_dim = 0;
    int rate = 0, win = 0, hop = 0;
    double segment_s = 0;
    long segment = 0;             // int(sample_rate_denoiser * segment_size)
};

inline bool dn_config(const babe_model::File& f, DnCfg& c, std::string& err) {
    using namespace babe_model;
    const std::string dn = "tester.denoiser.";
    auto kind = f.settings.find("kind");
    if (kind == f.settings.end() || !kind->second.is_string || kind->second.str != "denoiser")
        return err = "not a denoiser file (the setting kind = \"denoiser\" is missing: a UNet file is loaded by babe_model_load)", false;
    for (const char* flag : {"use_csff", "use_cam", "use_fam", "use_tdf", "use_alttdfs"}) {
        auto it = f.settings.find(dn + flag);
        if (it != f.settings.end() && (it->second.is_string || it->second.num != 0))
            return err = fmt("denoiser option %s is set (unused by the reference network, not implemented)", flag), false;
    }
    double d;
    if (!number(f, dn + "depth", d, err)) return false;
    if (d != std::floor(d) || d < 1 || d > 6) return err = fmt("tester.denoiser.depth = %g: a depth in 1..6 is expected", d), false;
    c.depth = (int)d;
    if (!number(f, dn + "num_stages", d, err)) return false;
    if (d != 1 && d != 2) return err = fmt("tester.denoiser.num_stages = %g: 1 or 2 stages are expected", d), false;
    c.num_stages = (int)d;
    if (!integer(f, dn + "num_tfc", 1, 8, c.num_tfc, err) || !integer(f, dn + "use_SAM", 0, 1, c.use_sam, err) ||
        !integer(f, dn + "use_fencoding", 0, 1, c.fenc, err) || !integer(f, dn + "f_dim", 2, 1 << 16, c.f_dim, err) ||
        !integer(f, dn + "sample_rate_denoiser", 1, MAX_RATE, c.rate, err) || !integer(f, dn + "stft_win_size", 64, 1024, c.win, err) ||
        !integer(f, dn + "stft_hop_size", 1, 1024, c.hop, err) || !number(f, dn + "segment_size", c.segment_s, err))
        return false;
    if (c.win & (c.win - 1)) return err = fmt("tester.denoiser.stft_win_size = %d is not a power of two", c.win), false;
    if (c.hop > c.win) return err = fmt("tester.denoiser.stft_hop_size = %d exceeds the window of %d", c.hop, c.win), false;
    if (c.fenc && c.f_dim != c.win / 2 + 1)
        return err = fmt("tester.denoiser.f_dim = %d, but use_fencoding needs stft_win_size / 2 + 1 = %d", c.f_dim, c.win / 2 + 1), false;
    const double seg = (double)c.rate * c.segment_s;
    if (!(seg >= 2 * FADE) || seg > (double)(1 << 28))
        return err = fmt("tester.denoiser.segment_size = %g s: a segment of %d .. 2^28 samples is expected", c.segment_s, 2 * FADE), false;
    c.segment = (long)seg;
    return true;
}

// networks/denoiser.py::param_shapes, in its order
inline std::vector<babe_model::Expected> dn_expected_tensors(const DnCfg& c) {
    using babe_model::Expected;
    std::vector<Expected> out;
    auto add = [&](const std::string& name, std::initializer_list<long> d) {
        Expected e{name, (int)d.size(), {1, 1, 1, 1}};
        std::copy(d.begin(), d.end(), e.dims);
        out.push_back(e);
    };
    auto conv = [&](const std::string& name, long co, long ci, long kh, long kw) {
        add(name + ".weight", {co, ci, kh, kw});
        add(name + ".bias", {co});
    };
    const int depth = c.depth, n = c.num_tfc, nin = c.fenc ? 12 : 2;
    auto iblock = [&](const std::string& pre, long n0, long width) {
        for (int i = 0; i < n; ++i) conv(pre + ".tfc.H." + std::to_string(i) + ".0", width, n0 + i * width, 3, 3);
        conv(pre + ".conv2d_res", width, n0, 1, 1);
    };
    auto encoder = [&](const std::string& pre, long n0) {
        for (int i = 0; i < depth; ++i) {
            const std::string e = pre + ".eblocks." + std::to_string(i);
            iblock(e + ".i_block", i == 0 ? n0 : NS[i], NS[i]);
            conv(e + ".conv2d_2.0", NS[i + 1], NS[i], 4, 4);
        }
        iblock(pre + ".i_block", NS[depth], NS[depth]);
    };
    auto decoder = [&](const std::string& pre) {
        for (int i = 0; i < depth; ++i) {
            const std::string d = pre + ".dblocks." + std::to_string(i);
            add(d + ".tconv_1.0.weight", {NS[i + 1], NS[i], 4, 4});          // [in, out, kh, kw]
            add(d + ".tconv_1.0.bias", {NS[i]});
            conv(d + ".projection", NS[i], NS[i + 1], 1, 1);
            iblock(d + ".i_block", 2 * NS[i], NS[i]);
        }
    };
    if (c.fenc) add("freq_encoding.fembeddings", {c.f_dim, 10});
    conv("conv2d_1.0", NS[0], nin, 7, 7);
    encoder("encoder_s1", NS[0]);
    decoder("decoder_s1");
    conv("finalblock.conv2", 2, NS[0], 3, 3);
    if (c.num_stages > 1) {
        conv("sam_1.conv1", NS[0], NS[0], 3, 3);
        conv("sam_1.conv2", 2, NS[0], 3, 3);
        conv("sam_1.conv3", NS[0], 2, 3, 3);
        conv("conv2d_2.0", NS[0], nin, 7, 7);
        encoder("encoder_s2", 2 * NS[0]);
        decoder("decoder_s2");
    }
    return out;
}

inline bool dn_check_tensors(const babe_model::File& f, const DnCfg& c, std::string& err) {
    using namespace babe_model;
    std::vector<Expected> want = dn_expected_tensors(c);
    want.push_back({"aux.tw4096", 2, {2048, 2, 1, 1}});
    want.push_back({"aux.fade", 1, {2 * FADE, 1, 1, 1}});
    std::map<std::string, const Expected*> by_name;
    for (const Expected& e : want) by_name[e.name] = &e;
    for (const Expected& e : want) {
        const Tensor* t = f.find(e.name);
        if (!t) return err = "missing tensor " + e.name, false;
        bool same = t->ndim == e.ndim;
        for (int k = 0; same && k < e.ndim; ++k) same = t->dims[k] == e.dims[k];
        if (!same) {
            std::string got, exp;
            for (int k = 0; k < t->ndim; ++k) got += (k ? "," : "") + std::to_string(t->dims[k]);
            for (int k = 0; k < e.ndim; ++k) exp += (k ? "," : "") + std::to_string(e.dims[k]);
            return err = "wrong shape for " + e.name + ": [" + got + "], the settings give [" + exp + "]", false;
        }
    }
    for (const Tensor& t : f.tensors)
        if (!by_name.count(t.name)) return err = "tensor " + t.name + " does not belong to a denoiser of these settings", false;
    return true;
}

// Everything babe_denoiser_load / _create check before they touch a device.
inline bool dn_validate(const babe_model::File& f, DnCfg& c, std::string& err) { return dn_config(f, c, err) && dn_check_tensors(f, c, err); }

}  // namespace babe_dn
