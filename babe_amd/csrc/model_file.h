// The model file (babe_amd/model_file.py writes it, INTEGRATION.md section 2 documents it): parser, settings and the table of
// tensors a CQTDiff+ network of those settings must hold.  Plain C++17, no HIP: csrc/model.hip includes it for babe_model_load /
// babe_model_create, tools/model_file_check.cpp compiles it with a host compiler under the sanitizers.
//
// Layout, little-endian, every offset absolute:
//   header, 64 bytes: magic "BABEMODL" | u32 version (1) | u32 header bytes (64) | u64 file bytes | u32 settings | u32 tensors |
//                     u64 settings offset | u64 index offset | u64 data offset | u64 0
//   settings [settings offset, index offset): records  u16 key length | u8 kind (0 number, 1 string) | u8 0 | u32 value bytes |
//                     key | value (kind 0: one float64; kind 1: the characters)
//   index    [index offset, data offset):     records  u16 name length | u16 ndim (1..4) | u32 0 | u64 dims[4] (unused: 1) |
//                     u64 data offset | u64 data bytes | name; then zeros up to the data section's boundary
//   data     [data offset, file bytes):       float32, each tensor on a 64-byte boundary, no two overlapping
// Nothing is read before its range has been checked against the buffer; every refusal has a message.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

namespace babe_model {

constexpr uint32_t VERSION = 1;
constexpr size_t HEADER_BYTES = 64, ALIGN = 64, MAX_NAME = 255, MAX_STRING = 255;
constexpr uint64_t MAX_RECORDS = 1u << 20;

struct Setting {
    bool is_string = false;
    double num = 0;
    std::string str;
};
struct Tensor {
    std::string name;
    int ndim = 0;
    long dims[4] = {1, 1, 1, 1};
    size_t numel = 0;
    const float* data = nullptr;      // host memory: inside the parsed buffer, or the caller's (babe_model_create)
};
struct File {
    std::map<std::string, Setting> settings;
    std::vector<Tensor> tensors;
    std::map<std::string, size_t> index;      // name -> position in tensors
    const Tensor* find(const std::string& name) const {
        auto it = index.find(name);
        return it == index.end() ? nullptr : &tensors[it->second];
    }
};

inline std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
inline std::string fmt(const char* f, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// a key or tensor name: 1..255 printable ASCII characters without blanks
inline bool name_ok(const char* p, size_t n) {
    if (n < 1 || n > MAX_NAME) return false;
    for (size_t i = 0; i < n; ++i)
        if (p[i] <= 0x20 || p[i] >= 0x7f) return false;
    return true;
}

// numel of dims[0..ndim), false on a non-positive dimension or a product (times 4 bytes) that does not fit 2^62
inline bool dim_product(const long* dims, int ndim, size_t& numel) {
    uint64_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (dims[i] < 1) return false;
        if ((uint64_t)dims[i] > (1ull << 60) / n) return false;
        n *= (uint64_t)dims[i];
    }
    numel = (size_t)n;
    return true;
}

// Adds a tensor to the table (both loaders): name, rank, dimensions and duplicates are checked here.
inline bool add_tensor(File& f, const std::string& name, int ndim, const long* dims, const float* data, std::string& err) {
    if (!name_ok(name.data(), name.size())) return err = "tensor name is empty, too long or not printable", false;
    if (ndim < 1 || ndim > 4) return err = fmt("tensor %s: rank %d (1..4)", name.c_str(), ndim), false;
    Tensor t;
    t.name = name, t.ndim = ndim, t.data = data;
    for (int i = 0; i < ndim; ++i) t.dims[i] = dims[i];
    if (!dim_product(t.dims, ndim, t.numel)) return err = fmt("tensor %s: dimension product overflows or is not positive", name.c_str()), false;
    if (!data) return err = fmt("tensor %s: no data", name.c_str()), false;
    if (!f.index.emplace(name, f.tensors.size()).second) return err = fmt("duplicate tensor name %s", name.c_str()), false;
    f.tensors.push_back(t);
    return true;
}
inline bool add_setting(File& f, const std::string& key, const Setting& s, std::string& err) {
    if (!name_ok(key.data(), key.size())) return err = "setting key is empty, too long or not printable", false;
    if (s.is_string && s.str.size() > MAX_STRING) return err = fmt("setting %s: string longer than %zu", key.c_str(), MAX_STRING), false;
    if (!s.is_string && !std::isfinite(s.num)) return err = fmt("setting %s: not a finite number", key.c_str()), false;
    if (!f.settings.emplace(key, s).second) return err = fmt("duplicate setting %s", key.c_str()), false;
    return true;
}

namespace detail {
struct Reader {                         // a cursor over [pos, end) of buf; every get checks its range first
    const unsigned char* buf;
    size_t pos, end;
    bool take(void* out, size_t n) {
        if (n > end - pos) return false;
        memcpy(out, buf + pos, n);
        pos += n;
        return true;
    }
    template <typename T>
    bool get(T& v) { return take(&v, sizeof v); }
    bool str(std::string& s, size_t n) {
        if (n > end - pos) return false;
        s.assign(reinterpret_cast<const char*>(buf + pos), n);
        pos += n;
        return true;
    }
};
}  // namespace detail

// buf[0..n) -> f (tensor data stays in buf: keep it alive as long as f).  false: err says why.
inline bool parse(const unsigned char* buf, size_t n, File& f, std::string& err) {
    using detail::Reader;
    if (!buf || n == 0) return err = "empty file", false;
    if (n < HEADER_BYTES) return err = fmt("truncated file: %zu bytes, the header alone has %zu", n, HEADER_BYTES), false;
    if (memcmp(buf, "BABEMODL", 8) != 0) return err = "wrong magic: not a babe model file", false;
    Reader h{buf, 8, HEADER_BYTES};
    uint32_t version, hbytes, nset, nten;
    uint64_t fbytes, soff, ioff, doff, zero;
    h.get(version), h.get(hbytes), h.get(fbytes), h.get(nset), h.get(nten), h.get(soff), h.get(ioff), h.get(doff), h.get(zero);
    if (version != VERSION) return err = fmt("unknown version %u (this library reads version %u)", version, VERSION), false;
    if (hbytes != HEADER_BYTES) return err = fmt("bad header: header size %u", hbytes), false;
    if (fbytes > n) return err = fmt("truncated file: the header says %llu bytes, the file has %zu", (unsigned long long)fbytes, n), false;
    if (fbytes < n) return err = fmt("bad header: the header says %llu bytes, the file has %zu", (unsigned long long)fbytes, n), false;
    if (!(soff == HEADER_BYTES && soff <= ioff && ioff <= doff && doff <= fbytes))
        return err = "bad header: section offsets out of order or out of range", false;
    if (nset > MAX_RECORDS || nten > MAX_RECORDS) return err = "bad header: record count out of range", false;
    if (doff % ALIGN) return err = "bad header: data section not 64-byte aligned", false;
    Reader s{buf, (size_t)soff, (size_t)ioff};
    for (uint32_t i = 0; i < nset; ++i) {
        uint16_t klen;
        uint8_t kind, pad;
        uint32_t vlen;
        std::string key;
        if (!s.get(klen) || !s.get(kind) || !s.get(pad) || !s.get(vlen) || !s.str(key, klen))
            return err = fmt("settings section: record %u leaves the section", i), false;
        Setting v;
        if (kind == 0) {
            if (vlen != 8 || !s.get(v.num)) return err = fmt("settings section: record %u (%s) is not one float64", i, key.c_str()), false;
        } else if (kind == 1) {
            v.is_string = true;
            if (vlen > MAX_STRING || !s.str(v.str, vlen)) return err = fmt("settings section: record %u leaves the section", i), false;
        } else {
            return err = fmt("settings section: record %u has unknown kind %u", i, kind), false;
        }
        if (!add_setting(f, key, v, err)) return false;
    }
    if (s.pos != s.end) return err = "settings section: bytes left after the last record", false;
    Reader t{buf, (size_t)ioff, (size_t)doff};
    std::vector<std::pair<uint64_t, uint64_t>> ranges;
    for (uint32_t i = 0; i < nten; ++i) {
        uint16_t nlen, ndim;
        uint32_t pad;
        uint64_t dims[4], off, nbytes;
        std::string name;
        if (!t.get(nlen) || !t.get(ndim) || !t.get(pad) || !t.take(dims, sizeof dims) || !t.get(off) || !t.get(nbytes) || !t.str(name, nlen))
            return err = fmt("tensor index: record %u leaves the section", i), false;
        if (!name_ok(name.data(), name.size())) return err = fmt("tensor index: record %u has a bad name", i), false;
        if (ndim < 1 || ndim > 4) return err = fmt("tensor %s: rank %u (1..4)", name.c_str(), ndim), false;
        long d[4];
        for (int k = 0; k < 4; ++k) {
            if (dims[k] < 1 || dims[k] > (1ull << 60) || (k >= ndim && dims[k] != 1))
                return err = fmt("tensor %s: dimension %d is not positive or overflows", name.c_str(), k), false;
            d[k] = (long)dims[k];
        }
        size_t numel;
        if (!dim_product(d, ndim, numel)) return err = fmt("tensor %s: dimension product overflows", name.c_str()), false;
        if (nbytes != (uint64_t)numel * 4) return err = fmt("tensor %s: %llu data bytes for %zu elements", name.c_str(), (unsigned long long)nbytes, numel), false;
        if (off % ALIGN) return err = fmt("tensor %s: data offset not 64-byte aligned", name.c_str()), false;
        if (off < doff || off > fbytes || nbytes > fbytes - off)
            return err = fmt("tensor %s: data range [%llu, +%llu) leaves the file's data section", name.c_str(), (unsigned long long)off, (unsigned long long)nbytes), false;
        if (!add_tensor(f, name, ndim, d, reinterpret_cast<const float*>(buf + off), err)) return false;
        ranges.emplace_back(off, off + nbytes);
    }
    if (t.end - t.pos >= ALIGN) return err = "tensor index: bytes left after the last record", false;
    for (size_t i = t.pos; i < t.end; ++i)              // the padding up to the data section's 64-byte boundary
        if (buf[i] != 0) return err = "tensor index: bytes left after the last record", false;
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); ++i)
        if (ranges[i].first < ranges[i - 1].second) return err = "overlapping tensor data", false;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- the network
// What the settings say about the network and the sampler (babe_amd/config.py::default_args names, flattened with dots).
struct NetCfg {
    double fs = 0, beta = 0;
    int L = 0, nocts = 0, bpo = 0, emb_dim = 0, fenc = 0;
    int Ns[8] = {}, dils[8] = {};
    // time attention (all zero without it): the core the host chose (1 fp32, 2 bf16), one flag per octave + the bottleneck, and
    // attention_options' leaves of network.attention_dict
    int attention = 0, att[8] = {}, heads = 0, bias_qkv = 0, rel_pos = 0, nbk = 0, maxd = 0;
    bool has_attention() const { return std::any_of(att, att + 8, [](int v) { return v != 0; }); }
    // sampler defaults
    int T = 0, order = 0, hpf = 0, nfft = 0, K = 0, has_start_sigma = 0, weighting = 0;
    double xi = 0, start_sigma = 0;
    double sigma_data = 0, sigma_min = 0, sigma_max = 0, ro = 0, Schurn = 0, Snoise = 0, Stmin = 0, Stmax = 0;
    double fcmin = 0, fcmax = 0, Amin = 0, Amax = 0, mu[2] = {}, tol[2] = {};
    int max_iter = 0, clamp_fc = 0, clamp_A = 0, only_negative_A = 0;
    float fc0[8] = {}, A0[8] = {};
};

inline bool number(const File& f, const std::string& key, double& v, std::string& err) {
    auto it = f.settings.find(key);
    if (it == f.settings.end()) return err = "missing setting " + key, false;
    if (it->second.is_string) return err = "setting " + key + " is a string, a number is expected", false;
    v = it->second.num;
    return true;
}
inline bool integer(const File& f, const std::string& key, long lo, long hi, int& v, std::string& err) {
    double d;
    if (!number(f, key, d, err)) return false;
    if (d != std::floor(d) || d < (double)lo || d > (double)hi)
        return err = fmt("setting %s = %g: an integer in %ld..%ld is expected", key.c_str(), d, lo, hi), false;
    v = (int)d;
    return true;
}

// an optional integer leaf: absent (or, under network.attention_dict, the whole node "None") leaves v at its default
inline bool integer_or(const File& f, const std::string& key, long lo, long hi, int& v, std::string& err) {
    return f.settings.count(key) ? integer(f, key, lo, hi, v, err) : true;
}

// settings -> cfg; refuses what the kernels do not cover.  attention: the host's choice of the attention core (0: a file with
// attention layers is refused, 1 fp32, 2 bf16 - babe_model_options::attention)
inline bool net_config(const File& f, NetCfg& c, std::string& err, int attention = 0) {
    const std::string nw = "network.", cq = "network.cqt.", te = "tester.", ps = "tester.posterior_sampling.", dp = "tester.diff_params.",
                      bb = "tester.blind_bwe.", op = "tester.blind_bwe.optimization.", ic = "tester.blind_bwe.initial_conditions.";
    if (attention < 0 || attention > 2) return err = fmt("attention = %d is none of 0 (refuse), 1 (fp32 core), 2 (bf16 core)", attention), false;
    for (int i = 0; i < 8; ++i) {                           // absent flags mean no attention
        auto it = f.settings.find(nw + "attention_layers." + std::to_string(i));
        if (it == f.settings.end()) continue;
        if (!attention && (it->second.is_string || it->second.num != 0))
            return err = fmt("attention layers are not supported by the library-side sequencers (network.attention_layers.%d is set)", i), false;
        if (!integer(f, it->first, 0, 1, c.att[i], err)) return false;
    }
    if (f.settings.count(nw + "attention_layers.8")) return err = "network.attention_layers has more entries than octaves plus the bottleneck", false;
    if (c.has_attention()) {                                // cqtdiff_plus.attention_options: the reference's defaults where absent
        const std::string ad = nw + "attention_dict.";
        c.attention = attention, c.heads = 8, c.bias_qkv = 0, c.rel_pos = 1, c.nbk = 32, c.maxd = 64;
        if (!integer_or(f, ad + "num_heads", 1, 64, c.heads, err) || !integer_or(f, ad + "bias_qkv", 0, 1, c.bias_qkv, err) ||
            !integer_or(f, ad + "use_rel_pos", 0, 1, c.rel_pos, err))
            return false;
        if (c.rel_pos) {                                    // what babe_attn_bucket_thresholds and the kernels' 64-bucket tables take
            if (!integer_or(f, ad + "rel_pos_num_buckets", 4, 64, c.nbk, err) || !integer_or(f, ad + "rel_pos_max_distance", 2, 65536, c.maxd, err))
                return false;
            if (c.nbk % 2) return err = fmt("%srel_pos_num_buckets = %d: an even count is expected", ad.c_str(), c.nbk), false;
            if (c.maxd <= c.nbk / 4)
                return err = fmt("%srel_pos_max_distance = %d: more than a quarter of the %d buckets is expected", ad.c_str(), c.maxd, c.nbk), false;
        }
    }
    auto prec = f.settings.find(nw + "precision");
    if (prec != f.settings.end() && !(prec->second.is_string && prec->second.str == "f32"))
        return err = "network.precision: the library-side sequencers run the fp32 network only", false;
    auto un = f.settings.find(nw + "use_norm");
    if (un != f.settings.end() && (un->second.is_string || un->second.num == 0)) return err = "network.use_norm = False is not implemented", false;
    auto win = f.settings.find(cq + "window");
    if (win != f.settings.end() && !(win->second.is_string && win->second.str == "kaiser"))
        return err = "network.cqt.window: only the kaiser window is planned by the library", false;
    if (!number(f, "exp.sample_rate", c.fs, err) || !integer(f, "exp.audio_len", 1, 1 << 30, c.L, err)) return false;
    if (!(c.fs > 0)) return err = "exp.sample_rate must be positive", false;
    if (!integer(f, cq + "num_octs", 1, 8, c.nocts, err) || !integer(f, cq + "bins_per_oct", 1, 4096, c.bpo, err) || !number(f, cq + "beta", c.beta, err))
        return false;
    if (c.nocts != 7) return err = fmt("network.cqt.num_octs = %d: the network has 7 octaves", c.nocts), false;
    if (!integer(f, nw + "emb_dim", 1, 1 << 16, c.emb_dim, err) || !integer(f, nw + "use_fencoding", 0, 1, c.fenc, err)) return false;
    if (c.fenc && c.bpo != 64) return err = fmt("use_fencoding needs 64 bins per octave (got %d)", c.bpo), false;
    // (the head dimension of level i is (i + 1) * bins_per_oct: a multiple of 64 up to 448 for the attention kernels)
    if (c.has_attention() && c.bpo != 64) return err = fmt("attention layers need 64 bins per octave (got %d)", c.bpo), false;
    for (int i = 0; i < c.nocts; ++i) {
        if (!integer(f, nw + "Ns." + std::to_string(i), 8, 512, c.Ns[i], err) || !integer(f, nw + "num_dils." + std::to_string(i), 1, 8, c.dils[i], err))
            return false;
        if (c.Ns[i] % 8) return err = fmt("network.Ns.%d = %d: channels are a multiple of the 8 GroupNorm groups", i, c.Ns[i]), false;
    }
    if (f.settings.count(nw + "Ns." + std::to_string(c.nocts)) || f.settings.count(nw + "num_dils." + std::to_string(c.nocts)))
        return err = "network.Ns / network.num_dils have more entries than octaves", false;
    // sampler defaults
    if (!integer(f, te + "T", 2, 100000, c.T, err) || !integer(f, te + "order", 1, 2, c.order, err) || !integer(f, te + "filter_out_cqt_DC_Nyq", 0, 1, c.hpf, err) ||
        !number(f, ps + "xi", c.xi, err))
        return false;
    auto ss = f.settings.find(ps + "start_sigma");
    if (ss == f.settings.end()) return err = "missing setting " + ps + "start_sigma", false;
    if (ss->second.is_string) {
        if (ss->second.str != "None") return err = ps + "start_sigma: a number or None is expected", false;
    } else {
        c.has_start_sigma = 1, c.start_sigma = ss->second.num;
    }
    auto fw = f.settings.find(ps + "freq_weighting_filter");
    if (fw == f.settings.end() || !fw->second.is_string) return err = "missing setting " + ps + "freq_weighting_filter (a string)", false;
    static const char* const W[] = {"None", "sqrt", "linear", "log"};
    c.weighting = -1;
    for (int i = 0; i < 4; ++i)
        if (fw->second.str == W[i]) c.weighting = i;
    if (c.weighting < 0) return err = ps + "freq_weighting_filter = " + fw->second.str + " is not implemented (None, sqrt, linear, log)", false;
    if (!number(f, dp + "sigma_data", c.sigma_data, err) || !number(f, dp + "sigma_min", c.sigma_min, err) || !number(f, dp + "sigma_max", c.sigma_max, err) ||
        !number(f, dp + "ro", c.ro, err) || !number(f, dp + "Schurn", c.Schurn, err) || !number(f, dp + "Snoise", c.Snoise, err) ||
        !number(f, dp + "Stmin", c.Stmin, err) || !number(f, dp + "Stmax", c.Stmax, err))
        return false;
    if (!integer(f, bb + "NFFT", 256, 4096, c.nfft, err)) return false;
    if (c.nfft & (c.nfft - 1)) return err = fmt("tester.blind_bwe.NFFT = %d is not a power of two", c.nfft), false;
    if (!number(f, bb + "fcmin", c.fcmin, err) || !number(f, bb + "fcmax", c.fcmax, err) || !number(f, bb + "Amin", c.Amin, err) || !number(f, bb + "Amax", c.Amax, err) ||
        !integer(f, op + "max_iter", 0, 1 << 20, c.max_iter, err) || !integer(f, op + "clamp_fc", 0, 1, c.clamp_fc, err) || !integer(f, op + "clamp_A", 0, 1, c.clamp_A, err) ||
        !integer(f, op + "only_negative_A", 0, 1, c.only_negative_A, err))
        return false;
    for (int i = 0; i < 2; ++i)
        if (!number(f, op + "mu." + std::to_string(i), c.mu[i], err) || !number(f, op + "tol." + std::to_string(i), c.tol[i], err)) return false;
    for (c.K = 0; c.K < 8 && f.settings.count(ic + "fc." + std::to_string(c.K)); ++c.K) {
        double fc, A;
        if (!number(f, ic + "fc." + std::to_string(c.K), fc, err) || !number(f, ic + "A." + std::to_string(c.K), A, err)) return false;
        c.fc0[c.K] = (float)fc, c.A0[c.K] = (float)A;
    }
    if (c.K < 1 || f.settings.count(ic + "fc.8")) return err = "tester.blind_bwe.initial_conditions: 1..8 break points are expected", false;
    return true;
}

// One ResnetBlock as babe_amd/networks/cqtdiff_plus.py::param_specs lays it out.
struct BlockSpec {
    std::string p;          // state_dict prefix, with the trailing dot
    int dim, dim_out, N, nd, KH, KW;
    bool proj_out, res_conv, proj_in;
    int attnF = 0;          // the head dimension of the block's time-attention branch (its frequency rows); 0: none
};
inline BlockSpec block_spec(const std::string& p, int dim, int dim_out, int nd, int KH, int KW, bool after) {
    BlockSpec b{p, dim, dim_out, after ? dim : dim_out, nd, KH, KW, false, false, false, 0};
    b.proj_out = after && b.N != dim_out;
    b.res_conv = dim != dim_out;
    b.proj_in = dim != b.N;
    return b;
}
// The network's blocks in the order of UnetEngine.blocks(): init, main, mid_blk, mid_out, up_out, up_blk.
struct NetBlocks {
    BlockSpec init[8], main[8], mid_blk, mid_out, up_out[8], up_blk[8];
};
inline NetBlocks net_blocks(const NetCfg& c) {
    NetBlocks nb;
    const int n = c.nocts, nin = c.fenc ? 66 : 2;
    for (int i = 0; i < n; ++i) {
        const int din = i == 0 ? c.Ns[0] : c.Ns[i - 1], dout = c.Ns[i];
        nb.init[i] = block_spec("downs." + std::to_string(i) + ".0.", nin, din, 1, 1, 1, false);
        nb.main[i] = block_spec("downs." + std::to_string(i) + ".2.", din, dout, c.dils[i], 5, 3, false);
        nb.main[i].attnF = c.att[i] ? (i + 1) * c.bpo : 0;
    }
    nb.mid_out = block_spec("middle.0.0.", c.Ns[n - 1], 2, 1, 1, 1, true);
    nb.mid_blk = block_spec("middle.0.1.", c.Ns[n - 1], c.Ns[n - 1], c.dils[n - 1], 5, 3, false);
    nb.mid_blk.attnF = c.att[n] ? n * c.bpo : 0;           // (the flag after the octaves': the bottleneck)
    for (int ii = 0; ii < n; ++ii) {
        const int i = n - 1 - ii;
        const int din = 2 * c.Ns[i], dout = i == 0 ? c.Ns[0] : c.Ns[i - 1];
        nb.up_out[ii] = block_spec("ups." + std::to_string(ii) + ".0.", dout, 2, 1, 1, 1, true);
        nb.up_blk[ii] = block_spec("ups." + std::to_string(ii) + ".1.", din, dout, c.dils[i], 5, 3, false);
        nb.up_blk[ii].attnF = c.att[i] ? (i + 1) * c.bpo : 0;
    }
    return nb;
}

struct Expected {
    std::string name;
    int ndim;
    long dims[4];
};
// Every tensor a state_dict of this network holds, with its shape.
inline std::vector<Expected> expected_tensors(const NetCfg& c) {
    std::vector<Expected> out;
    auto add = [&](const std::string& name, std::initializer_list<long> d) {
        Expected e{name, (int)d.size(), {1, 1, 1, 1}};
        std::copy(d.begin(), d.end(), e.dims);
        out.push_back(e);
    };
    add("embedding.RFF_freq", {1, 32});
    const long mlp[3][2] = {{128, 64}, {256, 128}, {c.emb_dim, 256}};
    for (int i = 0; i < 3; ++i) {
        add("embedding.MLP." + std::to_string(i) + ".weight", {mlp[i][0], mlp[i][1]});
        add("embedding.MLP." + std::to_string(i) + ".bias", {mlp[i][0]});
    }
    if (c.fenc)
        for (int i = 0; i < c.nocts; ++i) {
            add("freq_encodings." + std::to_string(i) + ".RFF_freq", {1, 32});
            add("freq_encodings." + std::to_string(i) + ".embeddings", {1, 64, c.bpo});
        }
    add("downsamplerT.kernel", {8});
    add("upsamplerT.kernel", {8});
    auto block = [&](const BlockSpec& b) {
        if (b.proj_out) add(b.p + "proj_out.weight", {b.dim_out, b.N, 1, 1});
        if (b.res_conv) add(b.p + "res_conv.weight", {b.dim_out, b.dim, 1, 1});
        if (b.proj_in) add(b.p + "proj_in.weight", {b.N, b.dim, 1, 1});
        for (int d = 0; d < b.nd; ++d) {
            const std::string k = std::to_string(d);
            add(b.p + "norm." + k + ".gamma", {1, b.N, 1, 1});
            add(b.p + "affine." + k + ".weight", {b.N, c.emb_dim});
            add(b.p + "affine." + k + ".bias", {b.N});
            add(b.p + "gate." + k + ".weight", {b.N, c.emb_dim});
            add(b.p + "gate." + k + ".bias", {b.N});
            add(b.p + "H." + k + ".weight", {b.N, b.N, b.KH, b.KW});
        }
        if (b.attnF) {                                       // the time-attention branch (param_specs: after the block's other keys)
            const long hF = (long)c.heads * b.attnF;
            add(b.p + "norm2.gamma", {1, b.N, 1, 1});
            for (const char* lin : {"affine2", "gate2"}) {
                add(b.p + lin + ".weight", {b.N, c.emb_dim});
                add(b.p + lin + ".bias", {b.N});
            }
            add(b.p + "attn_block.qk.weight", {2 * hF, hF, 1});
            if (c.bias_qkv) add(b.p + "attn_block.qk.bias", {2 * hF});
            add(b.p + "attn_block.proj_in.weight", {c.heads, b.N, 1, 1});
            add(b.p + "attn_block.proj_out.weight", {b.N, c.heads, 1, 1});
            if (c.rel_pos) add(b.p + "attn_block.rel_pos.relative_attention_bias.weight", {c.nbk, c.heads});
        }
    };
    const NetBlocks nb = net_blocks(c);
    for (int i = 0; i < c.nocts; ++i) {
        block(nb.init[i]);
        add("downs." + std::to_string(i) + ".1.weight", {c.Ns[i], 2, 5, 3});
        block(nb.main[i]);
    }
    block(nb.mid_out);
    block(nb.mid_blk);
    for (int i = 0; i < c.nocts; ++i) block(nb.up_out[i]), block(nb.up_blk[i]);
    return out;
}

// frames and envelope length of the STFT-domain degradation model for (nfft, L): babe_amd/stft.py::STFTOps
inline long env_len(const NetCfg& c) { return c.nfft + (long)(c.nfft / 2) * (c.L / (c.nfft / 2)); }

// The table against the settings: every expected tensor present with its shape, nothing else but the two aux tables.
inline bool check_tensors(const File& f, const NetCfg& c, std::string& err) {
    std::vector<Expected> want = expected_tensors(c);
    want.push_back({"aux.env_inv", 1, {env_len(c), 1, 1, 1}});
    want.push_back({"aux.tw4096", 2, {2048, 2, 1, 1}});
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
        if (!by_name.count(t.name)) return err = "tensor " + t.name + " does not belong to a network of these settings", false;
    return true;
}

// Everything a loader checks before it touches a device.
inline bool validate(const File& f, NetCfg& c, std::string& err, int attention = 0) {
    return net_config(f, c, err, attention) && check_tensors(f, c, err);
}

}  // namespace babe_model
