// The denoiser pre-pass and the rate conversions of a recording FILE, behind the C ABI - what networks/denoiser.py::DenoiserEngine,
// testing/denoise.py::DenoiserPrepass, resample.py's table builder and long_file.restore_recording_complete(fs=..., denoiser=...)
// sequence from Python, for a host without it:
//   babe_resample_sinc_table / babe_resampled_length   the resampler's table and output length, host only (csrc/dn_host.h)
//   babe_denoiser_load / _create                        one arena from a weights file, packed with babe_dn_pack_weights
//   babe_denoiser_fwd                                   DenoiserEngine.forward: the same launches in the same order
//   babe_denoise_signal                                 DenoiserPrepass.apply_denoiser: cut, pad, STFT, network, inverse STFT, cross-fade
//   babe_restore_file                                   conversion -> denoiser -> conversion -> babe_restore_recording
// The arithmetic is that of csrc/denoiser.hip and csrc/resample_sinc.hip, unchanged; new here are the sequencers and the two
// element-wise kernels that replace torch's slicing and in-place products.  Ownership of the handle is babe_model_load's
// (csrc/model.hip): create allocates one arena and waits on the stream once; nothing else allocates or synchronises.
#include "common.h"
#include "workspace.h"
#include "dn_host.h"
#include "eval_geom.h"
#include "../../include/babe_hip.h"
#include <cerrno>
#include <chrono>
#include <memory>

namespace {
using namespace babe_model;
using namespace babe_dn;

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ------------------------------------------------------------------------------------------------------- element-wise kernels
__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// dst[b][i] = i < n ? x[b][i] : 0 for i in [0, len); one row per blockIdx.y
__global__ __launch_bounds__(256) void pad_kernel(const float* __restrict__ x, long x_bs, long n, float* __restrict__ dst, long dst_bs,
                                                  long len) {
    const float* src = x + (long)blockIdx.y * x_bs;
    float* d = dst + (long)blockIdx.y * dst_bs;
    const long step = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (aligned16(src) && aligned16(d)) {
        const long lv = len / 4;
        for (long q = t0; q < lv; q += step) {
            const long i = 4 * q;
            float4 f;
            if (i + 3 < n) f = reinterpret_cast<const float4*>(src)[q];
            else f = make_float4(i < n ? src[i] : 0.f, i + 1 < n ? src[i + 1] : 0.f, i + 2 < n ? src[i + 2] : 0.f, 0.f);
            reinterpret_cast<float4*>(d)[q] = f;
        }
        for (long i = 4 * lv + t0; i < len; i += step) d[i] = i < n ? src[i] : 0.f;
    } else {
        for (long i = t0; i < len; i += step) d[i] = i < n ? src[i] : 0.f;
    }
}

// the cross-fade weight of sample i of a segment: the rising half on [0, size), the falling half on [seg - size, seg), else 1
__device__ __forceinline__ float fade_at(long i, long seg, const float* __restrict__ fade, int size, int fade_in, int fade_out) {
    if (fade_in && i < size) return fade[i];
    if (fade_out && i >= seg - size) return fade[size + (i - (seg - size))];
    return 1.f;
}
// out[b][i] = out[b][i] + y[b][i] * w(i): the product is rounded, then the sum (torch's `y *= w; out += y`); y * 1 is exact
__global__ __launch_bounds__(256) void fade_add_kernel(const float* __restrict__ y, long y_bs, float* __restrict__ out, long out_bs, long n,
                                                       long seg, const float* __restrict__ fade, int size, int fade_in, int fade_out) {
#pragma clang fp contract(off)
    const float* yr = y + (long)blockIdx.y * y_bs;
    float* o = out + (long)blockIdx.y * out_bs;
    const long step = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long done = 0;
    if (aligned16(yr) && aligned16(o)) {
        const long nv = n / 4;
        for (long q = t0; q < nv; q += step) {
            const long i = 4 * q;
            const float4 v = reinterpret_cast<const float4*>(yr)[q];
            float4 a = reinterpret_cast<const float4*>(o)[q];
            const float p0 = v.x * fade_at(i, seg, fade, size, fade_in, fade_out), p1 = v.y * fade_at(i + 1, seg, fade, size, fade_in, fade_out);
            const float p2 = v.z * fade_at(i + 2, seg, fade, size, fade_in, fade_out), p3 = v.w * fade_at(i + 3, seg, fade, size, fade_in, fade_out);
            a.x = a.x + p0, a.y = a.y + p1, a.z = a.z + p2, a.w = a.w + p3;
            reinterpret_cast<float4*>(o)[q] = a;
        }
        done = 4 * nv;
    }
    for (long i = done + t0; i < n; i += step) {
        const float p = yr[i] * fade_at(i, seg, fade, size, fade_in, fade_out);
        o[i] = o[i] + p;
    }
}

int grid_for(long n) {
    const int g = cdiv(n, 1024);
    return g < 1 ? 1 : (g > 2048 ? 2048 : g);
}

// ------------------------------------------------------------------------------------------------------------------ the handle
struct PC {                         // one convolution in the kernel's layout: networks/denoiser.py::_Packed
    const float* w[4] = {};         // mode 0: w[0]; transposed: parity (ph, pw) at 2 ph + pw
    const float* bias = nullptr;
    int Cout = 0, Cin = 0, KH = 0, KW = 0;
    bool tconv = false;
};

struct Denoiser {
    DnCfg cfg;
    int device = -1;
    char* arena = nullptr;
    size_t arena_bytes = 0, upload_bytes = 0;
    long params = 0;
    std::map<std::string, PC> pc;
    const float *femb = nullptr, *tw4096 = nullptr, *fade = nullptr;
    double ms[3] = {0, 0, 0};
};

// One pass over the arena's layout, dry (counting) or live (staging image, upload, pack kernels): csrc/model.hip's Builder.
struct Builder {
    const File& f;
    Denoiser& m;
    Carver& c;
    char* staging;
    void* stream;
    bool dry() const { return c.base == nullptr; }

    int run() {
        std::map<std::string, const float*> dev;
        for (const Tensor& t : f.tensors) {
            float* d = c.take<float>(t.numel);
            if (!dry() && d) memcpy(staging + (reinterpret_cast<char*>(d) - c.base), t.data, t.numel * sizeof(float));
            dev[t.name] = d;
        }
        m.upload_bytes = c.used;
        if (!dry()) {
            hipStream_t s = static_cast<hipStream_t>(stream);
            if (hipMemsetAsync(c.base + m.upload_bytes, 0, m.arena_bytes - m.upload_bytes, s) != hipSuccess ||
                hipMemcpyAsync(c.base, staging, m.upload_bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
                babe_set_error("denoiser: upload of %zu bytes failed: %s", m.upload_bytes, hipGetErrorString(hipGetLastError()));
                return BABE_ERR_HIP;
            }
            m.ms[1] = now_ms();
        }
        m.pc.clear();
        for (const Expected& e : dn_expected_tensors(m.cfg)) {
            const size_t len = e.name.size();
            if (len < 7 || e.name.compare(len - 7, 7, ".weight") != 0) continue;
            const std::string base = e.name.substr(0, len - 7);
            PC p;
            p.bias = dev[base + ".bias"];
            p.tconv = base.find(".tconv_1.") != std::string::npos;
            const float* w = dev[e.name];
            if (!p.tconv) {
                p.Cout = (int)e.dims[0], p.Cin = (int)e.dims[1], p.KH = (int)e.dims[2], p.KW = (int)e.dims[3];
                float* img = c.take<float>((size_t)babe_dn_packed_size(p.Cout, p.Cin, p.KH, p.KW));
                p.w[0] = img;
                if (!dry()) BABE_TRY(babe_dn_pack_weights(w, img, p.Cout, p.Cin, p.KH, p.KW, 0, 0, 0, stream));
            } else {
                p.Cin = (int)e.dims[0], p.Cout = (int)e.dims[1], p.KH = p.KW = 2;
                for (int ph = 0; ph < 2; ++ph)
                    for (int pw = 0; pw < 2; ++pw) {
                        float* img = c.take<float>((size_t)babe_dn_packed_size(p.Cout, p.Cin, 2, 2));
                        p.w[2 * ph + pw] = img;
                        if (!dry()) BABE_TRY(babe_dn_pack_weights(w, img, p.Cout, p.Cin, 2, 2, 1, ph, pw, stream));
                    }
            }
            m.pc[base] = p;
        }
        m.femb = m.cfg.fenc ? dev["freq_encoding.fembeddings"] : nullptr;
        m.tw4096 = dev["aux.tw4096"], m.fade = dev["aux.fade"];
        return BABE_OK;
    }
};

void destroy(Denoiser* m) {
    if (!m) return;
    if (m->arena) (void)hipFree(m->arena);
    delete m;
}

void* create(File& f, void* stream, double t0) {
    std::unique_ptr<Denoiser> guard(new Denoiser);
    Denoiser& m = *guard;
    std::string err;
    if (!dn_validate(f, m.cfg, err)) return babe_set_error("denoiser: %s", err.c_str()), nullptr;
    for (const Expected& e : dn_expected_tensors(m.cfg)) m.params += (long)f.find(e.name)->numel;
    m.ms[0] = now_ms();
    Carver dry{nullptr, 0, 256};
    {
        Builder b{f, m, dry, nullptr, stream};
        if (b.run() != BABE_OK) return nullptr;
    }
    m.arena_bytes = dry.used;
    if (hipGetDevice(&m.device) != hipSuccess || hipMalloc((void**)&m.arena, m.arena_bytes) != hipSuccess) {
        babe_set_error("denoiser: cannot allocate the %zu-byte arena on the current device: %s", m.arena_bytes, hipGetErrorString(hipGetLastError()));
        m.arena = nullptr;
        return nullptr;
    }
    Denoiser* pm = guard.release();                 // from here on destroy() releases it
    char* staging = static_cast<char*>(malloc(pm->upload_bytes ? pm->upload_bytes : 1));
    int rc = staging ? BABE_OK : BABE_ERR_ARG;
    if (!staging) babe_set_error("denoiser: cannot allocate %zu bytes of host staging", pm->upload_bytes);
    if (rc == BABE_OK) {
        memset(staging, 0, pm->upload_bytes);
        Carver live{pm->arena, pm->arena_bytes, 256};
        Builder b{f, *pm, live, staging, stream};
        rc = b.run();
        if (rc == BABE_OK && !live.ok) rc = (babe_set_error("denoiser: the arena's two layout passes disagree"), BABE_ERR_ARG);
    }
    if (staging) {                                  // the one wait: the upload has read the staging, the pack kernels have run
        const hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
        if (e != hipSuccess && rc == BABE_OK) rc = (babe_set_error("denoiser: upload / pack failed: %s", hipGetErrorString(e)), BABE_ERR_HIP);
        free(staging);
    }
    if (rc != BABE_OK) return destroy(pm), nullptr;
    const double t3 = now_ms();
    pm->ms[2] = t3 - pm->ms[1], pm->ms[1] -= pm->ms[0], pm->ms[0] -= t0;
    return pm;
}

const Denoiser* use(const void* h, const char* who) {
    const Denoiser* m = static_cast<const Denoiser*>(h);
    if (!m) return babe_set_error("%s: null denoiser", who), nullptr;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != m->device) {
        babe_set_error("%s: the denoiser lives on device %d, the current device is %d", who, m->device, dev);
        return nullptr;
    }
    return m;
}

// --------------------------------------------------------------------------------------------------------------- the forward
struct View {                       // a [B][C][H][W] view with contiguous planes (networks/denoiser.py::_planes)
    float* p = nullptr;
    long bs = 0, cs = 0;
    int C = 0, H = 0, W = 0;
};
View chan(const View& v, int c0, int n) {            // v[:, c0:c0 + n]
    View o = v;
    o.p = v.p ? v.p + (long)c0 * v.cs : nullptr;
    o.C = n;
    return o;
}
View tail(const View& v, int n) { return chan(v, v.C - n, n); }

struct StageBufs {
    View enc[6], dec[6], dec_out[6], low[6], bottom, bottom_out;
};
struct Bufs {                       // DenoiserEngine._alloc
    int H[7], W[7];
    View xin, pred1, sam_x1, sam_m;
    StageBufs st[2];
    float* ksws = nullptr;
};

// The launch sequence of DenoiserEngine.forward.  launch = false walks it without a launch and records what the split-K
// convolutions need of the shared partial-sum buffer.
struct Run {
    const Denoiser& m;
    int B;
    bool launch;
    void* stream;
    float* ksws;
    size_t ks_need = 0;

    const PC& pc(const std::string& name) const { return m.pc.at(name); }

    void split(babe_dnconv_args& a) {
        const int ks = babe_dn_ksplit(&a);
        if (ks <= 1) return;
        const size_t n = (size_t)ks * a.B * a.Cout * a.OH * a.OW;
        if (n > ks_need) ks_need = n;
        a.ksplit = ks, a.ws = ksws;
    }
    // networks/denoiser.py::_conv
    int conv(const View& x, const PC& p, const View& out, bool act = false, const View* res = nullptr, int stride = 1, int pt = -1, int pl = -1) {
        babe_dnconv_args a;
        memset(&a, 0, sizeof a);
        a.in = x.p, a.in_bs = x.bs, a.in_cs = x.cs, a.IH = x.H, a.IW = x.W;
        a.bias = p.bias;
        a.out = out.p, a.out_bs = out.bs, a.out_cs = out.cs, a.out_H = out.H, a.out_W = out.W;
        a.out_hstep = a.out_wstep = 1;
        if (res) a.res = res->p, a.res_bs = res->bs, a.res_cs = res->cs;
        a.B = B, a.Cin = x.C, a.Cout = p.Cout, a.OH = out.H, a.OW = out.W;
        a.KH = p.KH, a.KW = p.KW, a.stride = stride, a.pad_t = pt >= 0 ? pt : (p.KH - 1) / 2, a.pad_l = pl >= 0 ? pl : (p.KW - 1) / 2;
        a.pad_mode = 1, a.act = act ? 1 : 0;
        if (x.C != p.Cin || out.C != p.Cout) return babe_set_error("denoiser_fwd: a view of %d -> %d channels meets a %d -> %d convolution", x.C, out.C, p.Cin, p.Cout), BABE_ERR_ARG;
        split(a);
        return launch ? babe_dn_conv2d(&a, p.w[0], stream) : BABE_OK;
    }
    // networks/denoiser.py::_tconv: the four parities of the 4x4 stride-2 transposed convolution, cropped
    int tconv(const View& x, const PC& p, const View& out, int crop_h, int crop_w) {
        for (int ph = 0; ph < 2; ++ph)
            for (int pw = 0; pw < 2; ++pw) {
                babe_dnconv_args a;
                memset(&a, 0, sizeof a);
                a.in = x.p, a.in_bs = x.bs, a.in_cs = x.cs, a.IH = x.H, a.IW = x.W;
                a.bias = p.bias;
                a.out = out.p, a.out_bs = out.bs, a.out_cs = out.cs, a.out_H = out.H, a.out_W = out.W;
                a.out_hstep = 2, a.out_h0 = ph - crop_h, a.out_wstep = 2, a.out_w0 = pw - crop_w;
                a.B = B, a.Cin = x.C, a.Cout = p.Cout, a.OH = x.H + 1, a.OW = x.W + 1;
                a.KH = 2, a.KW = 2, a.stride = 1, a.pad_t = 1, a.pad_l = 1, a.pad_mode = 0, a.act = 1;
                split(a);
                if (launch) BABE_TRY(babe_dn_conv2d(&a, p.w[2 * ph + pw], stream));
            }
        return BABE_OK;
    }
    // I_Block on a dense buffer whose last n0 channels hold the input
    int iblock(const std::string& pre, const View& buf, int n0, int width, const View& out) {
        const int n = m.cfg.num_tfc, ctot = buf.C;
        BABE_TRY(conv(chan(buf, ctot - n0, n0), pc(pre + ".conv2d_res"), out));
        for (int i = 0; i < n; ++i) {
            const View src = chan(buf, ctot - n0 - i * width, n0 + i * width);
            const PC& p = pc(pre + ".tfc.H." + std::to_string(i) + ".0");
            if (i == n - 1) BABE_TRY(conv(src, p, out, true, &out));
            else BABE_TRY(conv(src, p, chan(buf, ctot - n0 - (i + 1) * width, width), true));
        }
        return BABE_OK;
    }
    int stage(int s, Bufs& bf, int first_n0, View& result) {
        StageBufs& st = bf.st[s - 1];
        const int depth = m.cfg.depth;
        const std::string enc = "encoder_s" + std::to_string(s), dec = "decoder_s" + std::to_string(s);
        for (int i = 0; i < depth; ++i) {
            const int n0 = i == 0 ? first_n0 : NS[i];
            const View bridge = tail(st.dec[i], NS[i]);
            const std::string e = enc + ".eblocks." + std::to_string(i);
            BABE_TRY(iblock(e + ".i_block", st.enc[i], n0, NS[i], bridge));
            const View& nxt = i + 1 < depth ? st.enc[i + 1] : st.bottom;
            BABE_TRY(conv(bridge, pc(e + ".conv2d_2.0"), tail(nxt, NS[i + 1]), true, nullptr, 2, 2, 2));
        }
        BABE_TRY(iblock(enc + ".i_block", st.bottom, NS[depth], NS[depth], st.bottom_out));
        View x = st.bottom_out;
        for (int i = depth - 1; i >= 0; --i) {
            const View& buf = st.dec[i];
            const View y = chan(buf, buf.C - 2 * NS[i], NS[i]);
            const int H = bf.H[i], W = bf.W[i], h = x.H, w = x.W;
            const int d2h = (2 * h - H) / 2, d2w = (2 * w - W) / 2;
            const std::string d = dec + ".dblocks." + std::to_string(i);
            BABE_TRY(tconv(x, pc(d + ".tconv_1.0"), y, 1 + d2h, 1 + d2w));
            BABE_TRY(conv(x, pc(d + ".projection"), st.low[i]));
            if (launch)
                BABE_TRY(babe_dn_upsample_add(y.p, y.bs, y.cs, st.low[i].p, st.low[i].bs, st.low[i].cs, B, NS[i], H, W, h, w, d2h, d2w, stream));
            BABE_TRY(iblock(d + ".i_block", buf, 2 * NS[i], NS[i], st.dec_out[i]));
            x = st.dec_out[i];
        }
        result = x;
        return BABE_OK;
    }
    int forward(const float* X, float* pred2, float* pred1, Bufs& bf) {
        const DnCfg& cfg = m.cfg;
        const int T = bf.H[0], F = bf.W[0];
        if (launch) BABE_TRY(babe_dn_fill_input(X, m.femb, bf.xin.p, B, T, F, cfg.fenc ? 10 : 0, stream));
        BABE_TRY(conv(bf.xin, pc("conv2d_1.0"), tail(bf.st[0].enc[0], NS[0]), true));
        View feats1, feats2;
        BABE_TRY(stage(1, bf, NS[0], feats1));
        View p1 = bf.pred1, p2 = bf.pred1, Xv = bf.pred1;
        if (pred1) p1.p = pred1;
        p2.p = pred2, Xv.p = const_cast<float*>(X);
        if (cfg.num_stages <= 1) return conv(feats1, pc("finalblock.conv2"), p1);
        // SAM (denoiser.py:117-132)
        BABE_TRY(conv(feats1, pc("sam_1.conv1"), bf.sam_x1));
        BABE_TRY(conv(feats1, pc("sam_1.conv2"), p1, false, &Xv));
        BABE_TRY(conv(p1, pc("sam_1.conv3"), bf.sam_m));
        const View tail2 = tail(bf.st[1].enc[0], 2 * NS[0]);
        BABE_TRY(conv(bf.xin, pc("conv2d_2.0"), chan(tail2, 0, NS[0]), true));
        const View second = chan(tail2, NS[0], NS[0]);
        if (launch) {
            if (cfg.use_sam) {
                BABE_TRY(babe_dn_sam_gate(bf.sam_x1.p, bf.sam_m.p, feats1.p, feats1.bs, feats1.cs, second.p, second.bs, second.cs, B, NS[0], (long)T * F,
                                          stream));
            } else {                                 // second.copy_(feats1): per batch item one dense block of NS[0] planes
                for (int b = 0; b < B; ++b)
                    if (hipMemcpyAsync(second.p + (long)b * second.bs, feats1.p + (long)b * feats1.bs, sizeof(float) * (size_t)NS[0] * T * F,
                                       hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)) != hipSuccess)
                        return babe_set_error("denoiser_fwd: copy failed: %s", hipGetErrorString(hipGetLastError())), BABE_ERR_HIP;
            }
        }
        BABE_TRY(stage(2, bf, 2 * NS[0], feats2));
        return conv(feats2, pc("finalblock.conv2"), p2);
    }
};

// every buffer of one forward, then the split-K buffer sized by a launch-free walk of the sequence over those very views
int carve_fwd(Carver& c, const Denoiser& m, int B, int T, int F, Bufs& bf) {
    const DnCfg& cfg = m.cfg;
    const int depth = cfg.depth, n = cfg.num_tfc;
    bf.H[0] = T, bf.W[0] = F;
    for (int i = 0; i < depth; ++i) bf.H[i + 1] = bf.H[i] / 2 + 1, bf.W[i + 1] = bf.W[i] / 2 + 1;      // 4x4 stride 2 on a 2-sample reflect pad
    auto mk = [&](int C, int lvl) {
        View v;
        v.C = C, v.H = bf.H[lvl], v.W = bf.W[lvl];
        v.cs = (long)v.H * v.W, v.bs = v.cs * C;
        v.p = c.take<float>((size_t)B * v.bs);
        return v;
    };
    bf.xin = mk(cfg.fenc ? 12 : 2, 0);
    for (int s = 1; s <= cfg.num_stages; ++s) {
        StageBufs& st = bf.st[s - 1];
        const int n0 = s == 1 ? NS[0] : 2 * NS[0];
        for (int i = 0; i < depth; ++i) {
            st.enc[i] = mk((i == 0 ? n0 : NS[i]) + (n - 1) * NS[i], i);
            st.dec[i] = mk(2 * NS[i] + (n - 1) * NS[i], i);
            st.dec_out[i] = mk(NS[i], i);
            st.low[i] = mk(NS[i], i + 1);
        }
        st.bottom = mk(NS[depth] + (n - 1) * NS[depth], depth);
        st.bottom_out = mk(NS[depth], depth);
    }
    bf.pred1 = mk(2, 0);
    if (cfg.num_stages > 1) bf.sam_x1 = mk(NS[0], 0), bf.sam_m = mk(NS[0], 0);
    Run measure{m, B, false, nullptr, nullptr};
    BABE_TRY(measure.forward(nullptr, nullptr, nullptr, bf));
    bf.ksws = c.take<float>(measure.ks_need ? measure.ks_need : 1);
    return BABE_OK;
}

int fwd_args_check(const Denoiser& m, int B, int T, int F, const char* who) {
    BABE_CHECK_ARG(B >= 1 && B <= 64, "%s: B = %d outside 1..64", who, B);
    // every level keeps a plane the reflect padding of its convolutions fits in (3 samples for the 7x7, 2 for the down conv)
    int h = T, w = F;
    for (int i = 0; i < m.cfg.depth; ++i) h = h / 2 + 1, w = w / 2 + 1;
    BABE_CHECK_ARG(T >= 4 && F >= 4 && T <= 1 << 16 && F <= 1 << 16 && h >= 2 && w >= 2, "%s: planes of %d x %d are not covered", who, T, F);
    BABE_CHECK_ARG(!m.cfg.fenc || F == m.cfg.f_dim, "%s: F = %d but the frequency encoding was built for f_dim = %d", who, F, m.cfg.f_dim);
    BABE_CHECK_ARG((double)B * (3 + m.cfg.num_tfc) * NS[0] * T * F < 2.0e9, "%s: B = %d planes of %d x %d exceed the 32-bit plane index", who, B, T, F);
    return BABE_OK;
}

// -------------------------------------------------------------------------------------------------- the segmented application
struct SigWork {
    float *seg, *X, *pred2, *pred1, *frames, *y;
    void* fwd;
    long fwd_bytes, Lp, Lout;
    int frames_n, nb;
};
int carve_signal(Carver& c, const Denoiser& m, int B, SigWork& w) {
    const DnCfg& cfg = m.cfg;
    w.Lp = cfg.segment + cfg.win;                                  // one window of zeros appended
    w.frames_n = (int)(1 + (w.Lp - cfg.win) / cfg.hop), w.nb = cfg.win / 2 + 1;
    const long synth = cfg.win + (long)cfg.hop * (w.frames_n - 1);
    w.Lout = synth < w.Lp ? synth : w.Lp;
    BABE_TRY(fwd_args_check(m, B, w.frames_n, w.nb, "denoise_signal"));
    const size_t plane = (size_t)B * 2 * w.frames_n * w.nb;
    w.seg = c.take<float>((size_t)B * w.Lp);
    w.X = c.take<float>(plane), w.pred2 = c.take<float>(plane), w.pred1 = c.take<float>(plane);
    w.frames = c.take<float>((size_t)B * w.frames_n * cfg.win);
    w.y = c.take<float>((size_t)B * w.Lout);
    Carver inner{nullptr, 0, 256};
    Bufs bf;
    BABE_TRY(carve_fwd(inner, m, B, w.frames_n, w.nb, bf));
    w.fwd_bytes = (long)inner.used;
    w.fwd = c.take<char>(inner.used);
    return BABE_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------- host-only entries
extern "C" long babe_resample_sinc_table_size(long orig_freq, long new_freq, int* width, int* orig, int* new_) {
    SincDims d;
    if (!sinc_dims(orig_freq, new_freq, d)) return babe_set_error("resample_sinc_table: rates %ld -> %ld outside 1..2^20", orig_freq, new_freq), -1;
    if (width) *width = d.width;
    if (orig) *orig = d.orig;
    if (new_) *new_ = d.new_;
    return (long)d.new_ * (2 * d.width + d.orig);
}
extern "C" int babe_resample_sinc_table(long orig_freq, long new_freq, float* kernel, int* krange) {
    SincDims d;
    BABE_CHECK_ARG(sinc_dims(orig_freq, new_freq, d), "resample_sinc_table: rates %ld -> %ld outside 1..2^20", orig_freq, new_freq);
    BABE_CHECK_ARG(kernel && krange, "resample_sinc_table: NULL kernel or krange");
    sinc_table(d, kernel, krange);
    return BABE_OK;
}
extern "C" long babe_resampled_length(long L, long orig_freq, long new_freq) {
    if (L < 0 || L > (1L << 40) || orig_freq < 1 || new_freq < 1 || orig_freq > MAX_RATE || new_freq > MAX_RATE)
        return babe_set_error("resampled_length: L = %ld, rates %ld -> %ld", L, orig_freq, new_freq), -1;
    return resampled_length(L, orig_freq, new_freq);
}
extern "C" long babe_denoise_signal_plan(long n, long segment, long overlap, long* starts, long max) {
    const long count = denoise_plan(n, segment, overlap, starts, max);
    if (count < 0)
        babe_set_error("denoise_signal_plan: n = %ld, segment = %ld, overlap = %ld: no walk (n >= 1, overlap >= 1, segment >= 2 overlap, and a "
                       "last remainder of at most segment - overlap after a first full segment)", n, segment, overlap);
    return count;
}
extern "C" int babe_restore_file_plan(long Lfile, long fs_file, long fs_denoiser, long fs_model, long* lengths) {
    const int mask = file_plan(Lfile, fs_file, fs_denoiser, fs_model, lengths);
    if (mask < 0) babe_set_error("restore_file_plan: Lfile = %ld, rates %ld / %ld / %ld", Lfile, fs_file, fs_denoiser, fs_model);
    return mask;
}
extern "C" int babe_dn_ksplit(const babe_dnconv_args* a) {
    if (!a || a->B < 1 || a->Cin < 1 || a->Cout < 1 || a->OH < 1 || a->OW < 1) return babe_set_error("dn_ksplit: bad shapes"), BABE_ERR_ARG;
    return ksplit(a->B, a->Cin, a->Cout, a->OH, a->OW, a->KH, a->KW);
}

// ------------------------------------------------------------------------------------------------------------------ the handle
extern "C" void* babe_denoiser_load(const char* path, void* stream) {
    const double t0 = now_ms();
    if (!path) return babe_set_error("denoiser_load: null path"), nullptr;
    FILE* fh = fopen(path, "rb");
    if (!fh) return babe_set_error("denoiser_load: cannot open %s: %s", path, strerror(errno)), nullptr;
    std::vector<unsigned char> buf;
    long size = -1;
    if (fseek(fh, 0, SEEK_END) == 0) size = ftell(fh);
    if (size < 0 || fseek(fh, 0, SEEK_SET) != 0) {
        fclose(fh);
        return babe_set_error("denoiser_load: cannot read %s", path), nullptr;
    }
    buf.resize((size_t)size);
    const size_t got = size ? fread(buf.data(), 1, (size_t)size, fh) : 0;
    fclose(fh);
    if (got != (size_t)size) return babe_set_error("denoiser_load: short read of %s (%zu of %ld bytes)", path, got, size), nullptr;
    File f;
    std::string err;
    if (!parse(buf.data(), buf.size(), f, err)) return babe_set_error("denoiser_load: %s: %s", path, err.c_str()), nullptr;
    return create(f, stream, t0);
}

extern "C" void* babe_denoiser_create(const babe_model_entry* entries, int n, const babe_model_kv* settings, int nsettings, void* stream) {
    const double t0 = now_ms();
    if (!entries || !settings || n < 1 || nsettings < 1) return babe_set_error("denoiser_create: null or empty tables"), nullptr;
    File f;
    std::string err;
    for (int i = 0; i < nsettings; ++i) {
        Setting s;
        if (!settings[i].key) return babe_set_error("denoiser_create: setting %d has no key", i), nullptr;
        if (settings[i].str) s.is_string = true, s.str = settings[i].str;
        else s.num = settings[i].num;
        if (!add_setting(f, settings[i].key, s, err)) return babe_set_error("denoiser_create: %s", err.c_str()), nullptr;
    }
    for (int i = 0; i < n; ++i) {
        if (!entries[i].name) return babe_set_error("denoiser_create: entry %d has no name", i), nullptr;
        if (!add_tensor(f, entries[i].name, entries[i].ndim, entries[i].shape, entries[i].data, err))
            return babe_set_error("denoiser_create: %s", err.c_str()), nullptr;
    }
    return create(f, stream, t0);
}

extern "C" void babe_denoiser_destroy(void* denoiser) { destroy(static_cast<Denoiser*>(denoiser)); }

extern "C" int babe_denoiser_info(const void* denoiser, babe_denoiser_summary* info) {
    const Denoiser* m = static_cast<const Denoiser*>(denoiser);
    BABE_CHECK_ARG(m && info, "denoiser_info: null arguments");
    const DnCfg& c = m->cfg;
    memset(info, 0, sizeof *info);
    info->depth = c.depth, info->num_tfc = c.num_tfc, info->num_stages = c.num_stages, info->use_SAM = c.use_sam, info->use_fencoding = c.fenc;
    info->f_dim = c.f_dim, info->sample_rate = c.rate, info->win = c.win, info->hop = c.hop, info->segment = c.segment;
    info->params = m->params, info->device_bytes = (long)m->arena_bytes, info->device = m->device;
    for (int i = 0; i < 3; ++i) info->load_ms[i] = m->ms[i];
    return BABE_OK;
}

// ----------------------------------------------------------------------------------------------------------------- the forward
extern "C" long babe_denoiser_workspace_bytes(const void* denoiser, int B, int T, int F) {
    const Denoiser* m = static_cast<const Denoiser*>(denoiser);
    if (!m) return babe_set_error("denoiser_workspace_bytes: null denoiser"), -1;
    if (fwd_args_check(*m, B, T, F, "denoiser_workspace_bytes") != BABE_OK) return -1;
    Carver dry{nullptr, 0, 256};
    Bufs bf;
    if (carve_fwd(dry, *m, B, T, F, bf) != BABE_OK) return -1;
    return (long)dry.used;
}

extern "C" int babe_denoiser_fwd(const void* denoiser, const float* X, float* pred2, float* pred1, void* ws, long ws_bytes, int B, int T, int F,
                                 void* stream) {
    const Denoiser* m = use(denoiser, "denoiser_fwd");
    if (!m) return BABE_ERR_ARG;
    BABE_TRY(fwd_args_check(*m, B, T, F, "denoiser_fwd"));
    BABE_CHECK_ARG(X && ws && (m->cfg.num_stages > 1 ? pred2 != nullptr : pred1 != nullptr), "denoiser_fwd: NULL X, ws or result");
    Carver c{static_cast<char*>(ws), ws_bytes > 0 ? (size_t)ws_bytes : 0, 256};
    Bufs bf;
    BABE_TRY(carve_fwd(c, *m, B, T, F, bf));
    BABE_CHECK_ARG(c.ok, "denoiser_fwd: workspace of %ld bytes, need %ld", ws_bytes, (long)c.used);
    Run run{*m, B, true, stream, bf.ksws};
    return run.forward(X, pred2, pred1, bf);
}

// ------------------------------------------------------------------------------------------------- the segmented application
extern "C" int babe_dn_segment_pad(const float* x, long x_bs, long n, float* dst, long dst_bs, long len, int B, void* stream) {
    BABE_CHECK_ARG(x && dst && B >= 1 && B <= 65535 && n >= 0 && len >= 1 && n <= len, "dn_segment_pad: B = %d, n = %ld, len = %ld", B, n, len);
    hipLaunchKernelGGL(pad_kernel, dim3(grid_for(len), B), dim3(256), 0, (hipStream_t)stream, x, x_bs, n, dst, dst_bs, len);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" int babe_dn_fade_add(const float* y, long y_bs, float* out, long out_bs, int B, long n, long seg, const float* fade, int size,
                                int fade_in, int fade_out, void* stream) {
    BABE_CHECK_ARG(y && out && B >= 1 && B <= 65535 && n >= 1 && n <= seg, "dn_fade_add: B = %d, n = %ld, seg = %ld", B, n, seg);
    BABE_CHECK_ARG(!(fade_in || fade_out) || (fade && size >= 1 && seg >= 2L * size), "dn_fade_add: a fade of %d samples on a segment of %ld", size, seg);
    hipLaunchKernelGGL(fade_add_kernel, dim3(grid_for(n), B), dim3(256), 0, (hipStream_t)stream, y, y_bs, out, out_bs, n, seg, fade, size,
                       fade_in ? 1 : 0, fade_out ? 1 : 0);
    BABE_LAUNCH_CHECK();
    return BABE_OK;
}

extern "C" long babe_denoise_signal_workspace_bytes(const void* denoiser, int B, long n) {
    const Denoiser* m = static_cast<const Denoiser*>(denoiser);
    if (!m) return babe_set_error("denoise_signal_workspace_bytes: null denoiser"), -1;
    if (n < 1) return babe_set_error("denoise_signal_workspace_bytes: n = %ld", n), -1;
    Carver dry{nullptr, 0, 256};
    SigWork w;
    if (carve_signal(dry, *m, B, w) != BABE_OK) return -1;
    return (long)dry.used;
}

extern "C" int babe_denoise_signal(const void* denoiser, const float* x, long x_bs, float* out, long out_bs, int B, long n, void* ws,
                                   long ws_bytes, void* stream) {
    const Denoiser* m = use(denoiser, "denoise_signal");
    if (!m) return BABE_ERR_ARG;
    const DnCfg& cfg = m->cfg;
    BABE_CHECK_ARG(x && out && ws && n >= 1, "denoise_signal: NULL x, out or ws, or n = %ld", n);
    BABE_CHECK_ARG(B == 1 || (x_bs >= n && out_bs >= n), "denoise_signal: row strides %ld / %ld below n = %ld", x_bs, out_bs, n);
    const long segment = cfg.segment, count = denoise_plan(n, segment, FADE, nullptr, 0);
    BABE_CHECK_ARG(count >= 1, "denoise_signal: n = %ld: the last segment would be longer than segment - %d = %ld samples (the reference fails here too)",
                   n, FADE, segment - FADE);
    Carver c{static_cast<char*>(ws), ws_bytes > 0 ? (size_t)ws_bytes : 0, 256};
    SigWork w;
    BABE_TRY(carve_signal(c, *m, B, w));
    BABE_CHECK_ARG(c.ok, "denoise_signal: workspace of %ld bytes, need %ld", ws_bytes, (long)c.used);
    hipStream_t st = (hipStream_t)stream;
    for (int b = 0; b < B; ++b)
        if (hipMemsetAsync(out + (long)b * out_bs, 0, sizeof(float) * (size_t)n, st) != hipSuccess)
            return babe_set_error("denoise_signal: clearing out failed: %s", hipGetErrorString(hipGetLastError())), BABE_ERR_HIP;
    const float* pred = cfg.num_stages > 1 ? w.pred2 : w.pred1;
    for (long s = 0, p = 0; s < count; ++s, p += segment - FADE) {
        const bool last = s == count - 1;
        const long nl = last ? n - p : segment;
        BABE_TRY(babe_dn_segment_pad(x + p, x_bs, nl, w.seg, w.Lp, w.Lp, B, stream));
        BABE_TRY(babe_dn_stft(w.seg, w.Lp, (int)w.Lp, w.X, B, cfg.win, cfg.hop, w.frames_n, m->tw4096, stream));
        BABE_TRY(babe_denoiser_fwd(m, w.X, w.pred2, w.pred1, w.fwd, w.fwd_bytes, B, w.frames_n, w.nb, stream));
        BABE_TRY(babe_dn_istft(pred, w.frames, w.y, w.Lout, (int)w.Lout, B, cfg.win, cfg.hop, w.frames_n, m->tw4096, stream));
        BABE_TRY(babe_dn_fade_add(w.y, w.Lout, out + p, out_bs, B, nl, segment, m->fade, FADE, p != 0, !last, stream));
    }
    return BABE_OK;
}

// -------------------------------------------------------------------------------------------------------------- the whole flow
namespace {
struct FileWork {
    float *a, *b, *c;              // after conv[0], after the denoiser, after conv[1] (each only where that step runs)
    void* run;                     // the denoiser's and the recording's workspaces, one after the other in one block
    long dn_bytes, rec_bytes, run_bytes;
};
int file_check(const babe_file_desc* d, const char* who) {
    BABE_CHECK_ARG(d, "%s: NULL descriptor", who);
    const long* len = d->lengths;
    BABE_CHECK_ARG(len[0] >= 2 && len[1] >= 2 && len[2] >= 2 && len[0] <= (1L << 40), "%s: lengths %ld / %ld / %ld", who, len[0], len[1], len[2]);
    for (int k = 0; k < 2; ++k) {
        const babe_sinc_table& t = d->conv[k];
        const long from = len[k], to = len[k + 1];
        if (!t.kernel) {
            BABE_CHECK_ARG(from == to, "%s: lengths[%d] = %ld and lengths[%d] = %ld differ without a conversion", who, k, from, k + 1, to);
            continue;
        }
        BABE_CHECK_ARG(t.krange && t.width >= 1 && t.orig >= 1 && t.new_ >= 1 && t.orig <= MAX_RATE && t.new_ <= MAX_RATE, "%s: conv[%d] is incomplete", who, k);
        BABE_CHECK_ARG(to == resampled_length(from, t.orig, t.new_), "%s: conv[%d] (%d -> %d) turns %ld samples into %ld, lengths[%d] = %ld", who, k,
                       t.orig, t.new_, from, resampled_length(from, t.orig, t.new_), k + 1, to);
    }
    BABE_CHECK_ARG(d->conv[1].kernel == nullptr || d->denoiser, "%s: conv[1] without a denoiser (one conversion goes to conv[0])", who);
    return BABE_OK;
}
int carve_file(Carver& c, const babe_file_desc* d, FileWork& w) {
    w.a = d->conv[0].kernel ? c.take<float>((size_t)d->lengths[1]) : nullptr;
    w.b = d->denoiser ? c.take<float>((size_t)d->lengths[1]) : nullptr;
    w.c = d->conv[1].kernel ? c.take<float>((size_t)d->lengths[2]) : nullptr;
    w.dn_bytes = d->denoiser ? babe_denoise_signal_workspace_bytes(d->denoiser, 1, d->lengths[1]) : 0;
    w.rec_bytes = babe_recording_workspace_bytes(&d->rec);
    if (w.dn_bytes < 0 || w.rec_bytes < 0) return BABE_ERR_ARG;
    w.run_bytes = w.dn_bytes > w.rec_bytes ? w.dn_bytes : w.rec_bytes;
    w.run = c.take<char>((size_t)w.run_bytes);
    return BABE_OK;
}
}  // namespace

extern "C" long babe_restore_file_workspace_bytes(const babe_file_desc* d) {
    if (file_check(d, "restore_file_workspace_bytes") != BABE_OK) return -1;
    Carver dry{nullptr, 0, 256};
    FileWork w;
    if (carve_file(dry, d, w) != BABE_OK) return -1;
    return (long)dry.used;
}

extern "C" int babe_restore_file(const babe_file_desc* d, const float* rec, long Lfile, float* out, float* filter_out, float* blind_pred,
                                 float* pre_out, long seed, long clip0, void* ws, long ws_bytes, void* stream) {
    // ---- host-side validation, all of it before the first device call
    BABE_TRY(file_check(d, "restore_file"));
    BABE_CHECK_ARG(rec && out && ws, "restore_file: NULL rec, out or ws");
    BABE_CHECK_ARG(Lfile == d->lengths[0], "restore_file: Lfile = %ld, lengths[0] = %ld", Lfile, d->lengths[0]);
    const Denoiser* m = d->denoiser ? use(d->denoiser, "restore_file") : nullptr;
    if (d->denoiser && !m) return BABE_ERR_ARG;
    if (m) BABE_CHECK_ARG(denoise_plan(d->lengths[1], m->cfg.segment, FADE, nullptr, 0) >= 1,
                          "restore_file: %ld samples at the denoiser's rate: the last segment would be longer than segment - %d = %ld samples", d->lengths[1],
                          FADE, m->cfg.segment - FADE);
    Carver c{static_cast<char*>(ws), ws_bytes > 0 ? (size_t)ws_bytes : 0, 256};
    FileWork w;
    BABE_TRY(carve_file(c, d, w));                      // (babe_recording_workspace_bytes checks the recording descriptor)
    BABE_CHECK_ARG(c.ok, "restore_file: workspace of %ld bytes, need %ld", ws_bytes, (long)c.used);
    const long Lrec = d->lengths[2], segL = d->rec.eval.L;
    for (int j = 0; j < d->rec.n_blind; ++j)
        BABE_CHECK_ARG(d->rec.blind_starts[j] >= 0 && d->rec.blind_starts[j] <= (Lrec > segL ? Lrec - segL : 0),
                       "restore_file: blind_starts[%d] = %ld past lengths[2] - segL = %ld", j, d->rec.blind_starts[j], Lrec - segL);
    babe_eval_desc probe = d->rec.eval;
    probe.blind = 1;
    BABE_TRY(eval_desc_check(&probe, "restore_file"));
    BABE_TRY(sample_steps_check(d->rec.steps_blind, d->rec.T, d->rec.t0, "restore_file: steps_blind"));
    BABE_TRY(sample_steps_check(d->rec.steps_known, d->rec.T, d->rec.t0, "restore_file: steps_known"));
    // ---- conversion, denoiser, conversion
    const float* cur = rec;
    if (d->conv[0].kernel) {
        const babe_sinc_table& t = d->conv[0];
        BABE_TRY(babe_resample_sinc(cur, d->lengths[0], w.a, d->lengths[1], 1, d->lengths[0], d->lengths[1], t.kernel, t.krange, t.orig, t.new_, t.width, stream));
        cur = w.a;
    }
    if (m) {
        BABE_TRY(babe_denoise_signal(m, cur, d->lengths[1], w.b, d->lengths[1], 1, d->lengths[1], w.run, w.dn_bytes, stream));
        cur = w.b;
    }
    if (d->conv[1].kernel) {
        const babe_sinc_table& t = d->conv[1];
        BABE_TRY(babe_resample_sinc(cur, d->lengths[1], w.c, d->lengths[2], 1, d->lengths[1], d->lengths[2], t.kernel, t.krange, t.orig, t.new_, t.width, stream));
        cur = w.c;
    }
    if (pre_out && hipMemcpyAsync(pre_out, cur, sizeof(float) * (size_t)Lrec, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
        return babe_set_error("restore_file: copy to pre_out failed: %s", hipGetErrorString(hipGetLastError())), BABE_ERR_HIP;
    // ---- normalise, blind estimate, AR pass: exactly babe_restore_recording
    return babe_restore_recording(&d->rec, cur, Lrec, out, filter_out, blind_pred, seed, clip0, w.run, w.rec_bytes, stream);
}
