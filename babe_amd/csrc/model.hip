// babe_model_*: a complete, ready-to-run network from one weights file (csrc/model_file.h; babe_amd/model_file.py writes it) - what
// a host without Python calls instead of restating UnetEngine.__init__, _Block, _FilmIndex, ops.PackedConv, STFTOps and CEval.
// The loader does what the Python engine does, with the same pack kernels on the same raw weights, so every image, table and
// descriptor field is bit-identical to the Python-built one (tests/test_gpu_model_c.py):
//   images       babe_packed_conv_plan (csrc/conv_auto.hip) with the default forms, as ops.PackedConv asks it; each conv's splits
//                from babe_conv_splits_for under the precision the HOST asked for at load time (the file holds the fp32 masters)
//   block order  UnetEngine.blocks(): init, main, mid_blk, mid_out, up_out, up_blk
//   FiLM         _FilmIndex: blocks in CONSTRUCTION order (init i, main i per octave; mid_blk, mid_out; up_out i, up_blk i), per
//                dilation layer the affine rows, then the gate rows
//   encodings    the init blocks' 66 -> 2 column convs and their babe_fenc_bias tables
//   attention    _Attn: per block with a time-attention layer the three (1,1) convs proj_in / proj_out / qk, packed under the same
//                rule at the load precision, norm2's gamma, the qk bias and the relative-position table as uploaded, and affine2 /
//                gate2 in the FiLM matrix after the block's dilation layers; only when the host chose an attention core
//                (babe_model_options::attention), which becomes the plan's attn_core
//   CQT          babe_cqt_plan_create_ex(fs, L, octaves, bins, beta, 8192)
// The documented exception to "the library never allocates / never synchronises": create allocates ONE arena on the current
// device (sized by a dry pass of the same layout function) plus the CQT plan's tables, and waits on `stream` once before it
// releases its host staging; destroy frees.  Nothing else here allocates, and no later call synchronises.  Every refusal happens
// before the first HIP call where the fault is in the file or the settings; a failure later frees what was made.
#include "common.h"
#include "workspace.h"
#include "model_file.h"
#include "../../include/babe_hip.h"
#include <cerrno>
#include <chrono>
#include <memory>

size_t babe_cqt_plan_table_bytes(const void* plan);      // csrc/cqt_plan.hip

namespace {
using namespace babe_model;

struct Model {
    NetCfg cfg;
    std::map<std::string, Setting> settings;
    int device = -1, precision = 0, attention = 0;
    babe_unet_attn attn[17];         // the attention branches desc's blocks point to (the plan keeps copies of its own)
    int nattn = 0;
    char* arena = nullptr;
    size_t arena_bytes = 0, upload_bytes = 0;
    long params = 0;
    babe_unet_plan_desc desc;
    void* unet_plan = nullptr;
    void* cqt_plan = nullptr;
    const float *rff = nullptr, *emb_W[3] = {}, *emb_b[3] = {}, *film_W = nullptr, *film_b = nullptr, *env_inv = nullptr, *tw4096 = nullptr;
    int film_J = 0;
    double ms[3] = {0, 0, 0};        // read + parse + validate, staging + upload, pack + CQT plan + the one wait
};

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One pass over the arena's layout: dry (c.base == nullptr) it only counts; live it fills the staging image of the upload region,
// enqueues the upload and every pack kernel.  Both passes take the same pieces in the same order.
struct Builder {
    const File& f;
    Model& m;
    Carver& c;
    char* staging;                   // host image of arena[0, upload_bytes); nullptr dry
    void* stream;
    std::map<std::string, const float*> dev;      // tensor name -> its device copy
    bool dry() const { return c.base == nullptr; }

    float* upload(const float* src, size_t n) {
        float* d = c.take<float>(n);
        if (!dry() && d) memcpy(staging + (reinterpret_cast<char*>(d) - c.base), src, n * sizeof(float));
        return d;
    }
    float* staged(float* d) const { return reinterpret_cast<float*>(staging + (reinterpret_cast<char*>(d) - c.base)); }
    const Tensor& T(const std::string& name) const { return *f.find(name); }       // (check_tensors found every name)

    // every image of one conv, as babe_packed_conv_plan lays them out (default forms; nt 2 where the (1,1) rule allows it), carved
    // direction by direction and packed from the device copy of the raw weights.  splits: the library's rule for the model's
    // precision with bf16_hbm_f32 on, as the Python engine has it by default; bf16 images are 2-byte elements, carved by their byte
    // count on the same 256-byte granules
    int conv(babe_packed_conv& pc, const float* w, int Cout, int Cin, int KH, int KW) {
        babe_packed_conv_layout lay;
        const int splits = babe_conv_splits_for(Cout, Cin, KH, KW, m.precision, 1);
        if (splits < 0) return BABE_ERR_ARG;
        BABE_TRY(babe_packed_conv_plan(Cout, Cin, KH, KW, splits, 0, 2, BABE_CONV_FORMS_ALL, &lay));
        memset(&pc, 0, sizeof pc);
        pc.Cout = Cout, pc.Cin = Cin, pc.KH = KH, pc.KW = KW, pc.nt = lay.nt, pc.splits = lay.splits;
        if (lay.raw) pc.w_raw = w;
        const float** family[8] = {&pc.fwd_wino, &pc.bwd_wino, &pc.fwd_wino4, &pc.bwd_wino4, &pc.fwd_wino45, &pc.bwd_wino45, &pc.fwd_wino85, &pc.bwd_wino85};
        for (int tf = 0; tf < 2; ++tf)
            for (int i = tf; i < 10; i += 2) {
                if (!lay.bytes[i]) continue;
                char* img = c.take<char>((size_t)lay.bytes[i]);
                if (i < 2) (tf ? pc.bwd : pc.fwd) = img;
                else *family[i - 2] = reinterpret_cast<float*>(img);
            }
        return dry() ? BABE_OK : babe_packed_conv_pack(&pc, w, stream);
    }
    int conv(babe_packed_conv& pc, const std::string& name) {
        const Tensor& t = T(name);
        return conv(pc, dev[name], (int)t.dims[0], (int)t.dims[1], (int)t.dims[2], (int)t.dims[3]);
    }

    // phase A of one block: its FiLM rows (affine, gate per layer) appended to the concatenated matrix, its folded column weights
    struct Folded { float *proj_in = nullptr, *res_conv = nullptr; };
    void film_rows(const BlockSpec& b, babe_unet_block& blk, float* W, float* bias, int& J) {
        const int E = m.cfg.emb_dim;
        for (int d = 0; d < b.nd; ++d)
            for (int gate = 0; gate < 2; ++gate) {
                const std::string k = b.p + (gate ? "gate." : "affine.") + std::to_string(d);
                (gate ? blk.film_gate : blk.film_aff)[d] = J;
                if (!dry()) {
                    memcpy(staged(W) + (size_t)J * E, T(k + ".weight").data, (size_t)b.N * E * sizeof(float));
                    memcpy(staged(bias) + J, T(k + ".bias").data, (size_t)b.N * sizeof(float));
                }
                J += b.N;
            }
        if (b.attnF) {                                       // _Attn: affine2, then gate2, after all of the block's layers
            babe_unet_attn& at = m.attn[m.nattn++];
            memset(&at, 0, sizeof at);
            blk.attn = &at;
            for (int gate = 0; gate < 2; ++gate) {
                const std::string k = b.p + (gate ? "gate2" : "affine2");
                (gate ? at.film_gate : at.film_aff) = J;
                if (!dry()) {
                    memcpy(staged(W) + (size_t)J * E, T(k + ".weight").data, (size_t)b.N * E * sizeof(float));
                    memcpy(staged(bias) + J, T(k + ".bias").data, (size_t)b.N * sizeof(float));
                }
                J += b.N;
            }
        }
    }
    float* fold(const std::string& name, int N) {          // w[:, :2] of a [N, 66, 1, 1] weight, contiguous
        float* d = c.take<float>((size_t)N * 2);
        if (!dry()) {
            const float* w = T(name).data;
            float* s = staged(d);
            for (int r = 0; r < N; ++r) s[2 * r] = w[66 * r], s[2 * r + 1] = w[66 * r + 1];
        }
        return d;
    }

    // phase B of one block: the packed convs, gammas and bias tables
    int block(const BlockSpec& b, babe_unet_block& blk, const Folded* fo, int oct) {
        blk.N = b.N, blk.nd = b.nd, blk.k53 = b.KH > 1;
        if (fo) {                                            // an init block with frequency encodings
            const float* emb = dev["freq_encodings." + std::to_string(oct) + ".embeddings"];
            const struct { const char* name; float* w2; babe_packed_conv* pc; const float** fb; } folded[2] = {
                {"proj_in.weight", fo->proj_in, &blk.proj_in, &blk.fb_proj_in}, {"res_conv.weight", fo->res_conv, &blk.res_conv, &blk.fb_res_conv}};
            for (const auto& fd : folded) {
                BABE_TRY(conv(*fd.pc, fd.w2, b.N, 2, 1, 1));
                float* fb = c.take<float>((size_t)b.N * 64);
                *fd.fb = fb;
                if (!dry()) BABE_TRY(babe_fenc_bias(dev[b.p + fd.name], emb, fb, b.N, 66, stream));
            }
        } else {
            if (b.proj_in) BABE_TRY(conv(blk.proj_in, b.p + "proj_in.weight"));
            if (b.res_conv) BABE_TRY(conv(blk.res_conv, b.p + "res_conv.weight"));
        }
        if (b.proj_out) BABE_TRY(conv(blk.proj_out, b.p + "proj_out.weight"));
        for (int d = 0; d < b.nd; ++d) {
            BABE_TRY(conv(blk.H[d], b.p + "H." + std::to_string(d) + ".weight"));
            blk.gamma[d] = dev[b.p + "norm." + std::to_string(d) + ".gamma"];
        }
        if (b.attnF) {                                       // (film_rows made the branch and set its FiLM offsets)
            const NetCfg& cfg = m.cfg;
            babe_unet_attn& at = const_cast<babe_unet_attn&>(*blk.attn);
            const std::string ab = b.p + "attn_block.";
            at.H = cfg.heads, at.F = b.attnF, at.scale = (float)std::pow((double)b.attnF, -0.5);
            BABE_TRY(conv(at.proj_in, ab + "proj_in.weight"));
            BABE_TRY(conv(at.proj_out, ab + "proj_out.weight"));
            BABE_TRY(conv(at.qk, dev[ab + "qk.weight"], 2 * cfg.heads * b.attnF, cfg.heads * b.attnF, 1, 1));      // Conv1d: [2HF, HF, 1]
            at.gamma = dev[b.p + "norm2.gamma"];
            if (cfg.bias_qkv) at.qk_bias = dev[ab + "qk.bias"];
            if (cfg.rel_pos) at.emb = dev[ab + "rel_pos.relative_attention_bias.weight"], at.num_buckets = cfg.nbk, at.max_distance = cfg.maxd;
        }
        return BABE_OK;
    }

    int run() {
        const NetCfg& cfg = m.cfg;
        const int n = cfg.nocts, E = cfg.emb_dim;
        const NetBlocks nb = net_blocks(cfg);
        babe_unet_plan_desc& D = m.desc;
        memset(&D, 0, sizeof D);
        m.nattn = 0;
        D.nocts = n, D.bpo = cfg.bpo, D.attn_core = cfg.has_attention() ? m.attention : 0;
        for (int i = 0; i < n; ++i) D.Ns[i] = cfg.Ns[i];
        // ---- phase A: what is uploaded.  Every tensor of the file as it is ...
        for (const Tensor& t : f.tensors) dev[t.name] = upload(t.data, t.numel);
        // ... the FiLM Linears stacked in the engine's order ...
        int J = 0;
        for (int i = 0; i < n; ++i) J += 2 * (nb.init[i].N * nb.init[i].nd + nb.main[i].N * nb.main[i].nd + nb.up_out[i].N * nb.up_out[i].nd + nb.up_blk[i].N * nb.up_blk[i].nd);
        J += 2 * (nb.mid_blk.N * nb.mid_blk.nd + nb.mid_out.N * nb.mid_out.nd);
        for (int i = 0; i < n; ++i) J += 2 * ((nb.main[i].attnF ? nb.main[i].N : 0) + (nb.up_blk[i].attnF ? nb.up_blk[i].N : 0));
        J += 2 * (nb.mid_blk.attnF ? nb.mid_blk.N : 0);
        float* W = c.take<float>((size_t)J * E);
        float* bias = c.take<float>((size_t)J);
        int at = 0;
        for (int i = 0; i < n; ++i) film_rows(nb.init[i], D.init_blk[i], W, bias, at), film_rows(nb.main[i], D.main_blk[i], W, bias, at);
        film_rows(nb.mid_blk, D.mid_blk, W, bias, at), film_rows(nb.mid_out, D.mid_out, W, bias, at);
        for (int i = 0; i < n; ++i) film_rows(nb.up_out[i], D.up_out[i], W, bias, at), film_rows(nb.up_blk[i], D.up_blk[i], W, bias, at);
        if (at != J) return babe_set_error("model: FiLM rows %d != %d", at, J), BABE_ERR_ARG;
        m.film_W = W, m.film_b = bias, m.film_J = J;
        // ... and the signal columns of the folded init-block convs
        Folded fo[8];
        if (cfg.fenc)
            for (int i = 0; i < n; ++i) {
                fo[i].proj_in = fold(nb.init[i].p + "proj_in.weight", nb.init[i].N);
                fo[i].res_conv = fold(nb.init[i].p + "res_conv.weight", nb.init[i].N);
            }
        m.upload_bytes = c.used;
        if (!dry()) {
            hipStream_t s = static_cast<hipStream_t>(stream);
            if (hipMemsetAsync(c.base + m.upload_bytes, 0, m.arena_bytes - m.upload_bytes, s) != hipSuccess ||
                hipMemcpyAsync(c.base, staging, m.upload_bytes, hipMemcpyHostToDevice, s) != hipSuccess) {
                babe_set_error("model: upload of %zu bytes failed: %s", m.upload_bytes, hipGetErrorString(hipGetLastError()));
                return BABE_ERR_HIP;
            }
            m.ms[1] = now_ms();
        }
        // ---- phase B: the images, packed on the device from the uploaded raw weights
        for (int i = 0; i < n; ++i) {
            BABE_TRY(block(nb.init[i], D.init_blk[i], cfg.fenc ? &fo[i] : nullptr, i));
            BABE_TRY(conv(D.pyr_conv[i], "downs." + std::to_string(i) + ".1.weight"));
            BABE_TRY(block(nb.main[i], D.main_blk[i], nullptr, i));
        }
        BABE_TRY(block(nb.mid_blk, D.mid_blk, nullptr, 0));
        BABE_TRY(block(nb.mid_out, D.mid_out, nullptr, 0));
        for (int i = 0; i < n; ++i) {
            BABE_TRY(block(nb.up_out[i], D.up_out[i], nullptr, 0));
            BABE_TRY(block(nb.up_blk[i], D.up_blk[i], nullptr, 0));
        }
        m.rff = dev["embedding.RFF_freq"];
        for (int i = 0; i < 3; ++i) {
            m.emb_W[i] = dev["embedding.MLP." + std::to_string(i) + ".weight"];
            m.emb_b[i] = dev["embedding.MLP." + std::to_string(i) + ".bias"];
        }
        m.env_inv = dev["aux.env_inv"], m.tw4096 = dev["aux.tw4096"];
        return BABE_OK;
    }
};

void destroy(Model* m) {
    if (!m) return;
    if (m->unet_plan) babe_unet_plan_destroy(m->unet_plan);
    if (m->cqt_plan) babe_cqt_plan_destroy(m->cqt_plan);
    if (m->arena) (void)hipFree(m->arena);
    delete m;
}

// f (validated here) -> a model on the current device, or nullptr with the message set.  t0: when the caller began (load: before
// it read the file).
void* create(File& f, int precision, int attention, void* stream, double t0) {
    std::unique_ptr<Model> guard(new Model);
    Model& m = *guard;
    m.precision = precision, m.attention = attention;
    std::string err;
    if (!validate(f, m.cfg, err, attention)) return babe_set_error("model: %s", err.c_str()), nullptr;
    const NetCfg& cfg = m.cfg;
    if (cfg.has_attention() && cfg.rel_pos) {       // what babe_unet_plan_create would refuse of the bucket table, asked before any device call
        babe_attn_bucket_thr thr;
        if (babe_attn_bucket_thresholds(&thr, cfg.nbk, cfg.maxd) != BABE_OK) {
            const std::string why = babe_last_error();
            return babe_set_error("model: network.attention_dict: %s", why.c_str()), nullptr;
        }
    }
    // the CQT design is host-only: a length the plan does not cover is refused before any device call (its message is set)
    void* design = babe_cqt_design_create_ex(cfg.fs, cfg.L, cfg.nocts, cfg.bpo, cfg.beta, 8192);
    if (!design) {
        const std::string why = babe_last_error();
        return babe_set_error("model: %s", why.c_str()), nullptr;
    }
    babe_cqt_design_destroy(design);
    m.settings = f.settings;
    for (const Expected& e : expected_tensors(cfg)) m.params += (long)f.find(e.name)->numel;
    m.ms[0] = now_ms();
    Carver dry{nullptr, 0, 256};
    {
        Builder b{f, m, dry, nullptr, stream, {}};
        if (b.run() != BABE_OK) return nullptr;
    }
    m.arena_bytes = dry.used;
    if (hipGetDevice(&m.device) != hipSuccess || hipMalloc((void**)&m.arena, m.arena_bytes) != hipSuccess) {
        babe_set_error("model: cannot allocate the %zu-byte arena on the current device: %s", m.arena_bytes, hipGetErrorString(hipGetLastError()));
        m.arena = nullptr;
        return nullptr;
    }
    Model* pm = guard.release();                    // from here on destroy() releases it
    char* staging = static_cast<char*>(malloc(pm->upload_bytes ? pm->upload_bytes : 1));
    int rc = staging ? BABE_OK : BABE_ERR_ARG;
    if (!staging) babe_set_error("model: cannot allocate %zu bytes of host staging", pm->upload_bytes);
    if (rc == BABE_OK) {
        memset(staging, 0, pm->upload_bytes);
        Carver live{pm->arena, pm->arena_bytes, 256};
        Builder b{f, *pm, live, staging, stream, {}};
        rc = b.run();
        if (rc == BABE_OK && !live.ok) rc = (babe_set_error("model: the arena's two layout passes disagree"), BABE_ERR_ARG);
    }
    if (rc == BABE_OK) {
        pm->cqt_plan = babe_cqt_plan_create_ex(cfg.fs, cfg.L, cfg.nocts, cfg.bpo, cfg.beta, 8192);
        if (!pm->cqt_plan) rc = BABE_ERR_HIP;
    }
    // the one wait: the upload has read the staging and the pack kernels have run (their failures surface here)
    if (staging) {
        const hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
        if (e != hipSuccess && rc == BABE_OK) rc = (babe_set_error("model: upload / pack failed: %s", hipGetErrorString(e)), BABE_ERR_HIP);
        free(staging);
    }
    if (rc == BABE_OK) {
        pm->unet_plan = babe_unet_plan_create(&pm->desc);
        if (!pm->unet_plan) rc = BABE_ERR_ARG;
    }
    if (rc != BABE_OK) return destroy(pm), nullptr;
    const double t3 = now_ms();
    pm->ms[2] = t3 - pm->ms[1], pm->ms[1] -= pm->ms[0], pm->ms[0] -= t0;
    return pm;
}

const Model* use(const void* model, const char* who) {
    const Model* m = static_cast<const Model*>(model);
    if (!m) return babe_set_error("%s: null model", who), nullptr;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != m->device) {
        babe_set_error("%s: the model lives on device %d, the current device is %d", who, m->device, dev);
        return nullptr;
    }
    return m;
}
}  // namespace

// (asked first: a host's own mistake, whatever the file holds)
static bool precision_ok(int precision, const char* who) {
    if (precision >= BABE_PRECISION_F32 && precision <= BABE_PRECISION_BF16X3) return true;
    babe_set_error("%s: precision %d is none of BABE_PRECISION_F32 (0), _BF16 (1), _BF16X3 (2)", who, precision);
    return false;
}

static bool attention_ok(int attention, const char* who) {
    if (attention >= BABE_ATTENTION_REFUSE && attention <= BABE_ATTENTION_BF16) return true;
    babe_set_error("%s: attention %d is none of BABE_ATTENTION_REFUSE (0), _F32 (1), _BF16 (2)", who, attention);
    return false;
}
static bool options_ok(const babe_model_options* o, const char* who) {
    if (!o) return babe_set_error("%s: null options", who), false;
    return precision_ok(o->precision, who) && attention_ok(o->attention, who);
}

static void* model_load(const char* path, int precision, int attention, void* stream) {
    const double t0 = now_ms();
    if (!path) return babe_set_error("model_load: null path"), nullptr;
    FILE* fh = fopen(path, "rb");
    if (!fh) return babe_set_error("model_load: cannot open %s: %s", path, strerror(errno)), nullptr;
    std::vector<unsigned char> buf;
    long size = -1;
    if (fseek(fh, 0, SEEK_END) == 0) size = ftell(fh);
    if (size < 0 || fseek(fh, 0, SEEK_SET) != 0) {
        fclose(fh);
        return babe_set_error("model_load: cannot read %s", path), nullptr;
    }
    buf.resize((size_t)size);
    const size_t got = size ? fread(buf.data(), 1, (size_t)size, fh) : 0;
    fclose(fh);
    if (got != (size_t)size) return babe_set_error("model_load: short read of %s (%zu of %ld bytes)", path, got, size), nullptr;
    File f;
    std::string err;
    if (!parse(buf.data(), buf.size(), f, err)) return babe_set_error("model_load: %s: %s", path, err.c_str()), nullptr;
    return create(f, precision, attention, stream, t0);
}
extern "C" void* babe_model_load_opt(const char* path, const babe_model_options* options, void* stream) {
    return options_ok(options, "model_load") ? model_load(path, options->precision, options->attention, stream) : nullptr;
}
extern "C" void* babe_model_load_ex(const char* path, int precision, void* stream) {
    return precision_ok(precision, "model_load") ? model_load(path, precision, BABE_ATTENTION_REFUSE, stream) : nullptr;
}
extern "C" void* babe_model_load(const char* path, void* stream) { return babe_model_load_ex(path, BABE_PRECISION_F32, stream); }

static void* model_create(const babe_model_entry* entries, int n, const babe_model_kv* settings, int nsettings, int precision, int attention,
                          void* stream) {
    const double t0 = now_ms();
    if (!entries || !settings || n < 1 || nsettings < 1) return babe_set_error("model_create: null or empty tables"), nullptr;
    File f;
    std::string err;
    for (int i = 0; i < nsettings; ++i) {
        Setting s;
        if (!settings[i].key) return babe_set_error("model_create: setting %d has no key", i), nullptr;
        if (settings[i].str) s.is_string = true, s.str = settings[i].str;
        else s.num = settings[i].num;
        if (!add_setting(f, settings[i].key, s, err)) return babe_set_error("model_create: %s", err.c_str()), nullptr;
    }
    for (int i = 0; i < n; ++i) {
        if (!entries[i].name) return babe_set_error("model_create: entry %d has no name", i), nullptr;
        if (!add_tensor(f, entries[i].name, entries[i].ndim, entries[i].shape, entries[i].data, err))
            return babe_set_error("model_create: %s", err.c_str()), nullptr;
    }
    return create(f, precision, attention, stream, t0);
}
extern "C" void* babe_model_create_opt(const babe_model_entry* entries, int n, const babe_model_kv* settings, int nsettings,
                                       const babe_model_options* options, void* stream) {
    return options_ok(options, "model_create") ? model_create(entries, n, settings, nsettings, options->precision, options->attention, stream)
                                               : nullptr;
}
extern "C" void* babe_model_create_ex(const babe_model_entry* entries, int n, const babe_model_kv* settings, int nsettings, int precision,
                                      void* stream) {
    return precision_ok(precision, "model_create") ? model_create(entries, n, settings, nsettings, precision, BABE_ATTENTION_REFUSE, stream)
                                                   : nullptr;
}
extern "C" void* babe_model_create(const babe_model_entry* entries, int n, const babe_model_kv* settings, int nsettings, void* stream) {
    return babe_model_create_ex(entries, n, settings, nsettings, BABE_PRECISION_F32, stream);
}

extern "C" int babe_model_precision(const void* model) {
    const Model* m = static_cast<const Model*>(model);
    if (!m) return babe_set_error("model_precision: null model"), -1;
    return m->precision;
}

extern "C" int babe_model_attention(const void* model) {
    const Model* m = static_cast<const Model*>(model);
    if (!m) return babe_set_error("model_attention: null model"), -1;
    return m->attention;
}

extern "C" void babe_model_destroy(void* model) { destroy(static_cast<Model*>(model)); }

extern "C" int babe_model_info(const void* model, babe_model_summary* info) {
    const Model* m = static_cast<const Model*>(model);
    BABE_CHECK_ARG(m && info, "model_info: null arguments");
    memset(info, 0, sizeof *info);
    info->L = m->cfg.L, info->fs = (float)m->cfg.fs, info->nocts = m->cfg.nocts, info->bpo = m->cfg.bpo;
    for (int i = 0; i < m->cfg.nocts; ++i) info->Ns[i] = m->cfg.Ns[i];
    info->params = m->params, info->device_bytes = (long)m->arena_bytes, info->cqt_device_bytes = (long)babe_cqt_plan_table_bytes(m->cqt_plan);
    info->device = m->device;
    for (int i = 0; i < 3; ++i) info->load_ms[i] = m->ms[i];
    return BABE_OK;
}

extern "C" int babe_model_setting(const void* model, const char* key, double* value) {
    const Model* m = static_cast<const Model*>(model);
    BABE_CHECK_ARG(m && key && value, "model_setting: null arguments");
    auto it = m->settings.find(key);
    BABE_CHECK_ARG(it != m->settings.end(), "model_setting: no setting %s", key);
    BABE_CHECK_ARG(!it->second.is_string, "model_setting: %s is the string %s", key, it->second.str.c_str());
    *value = it->second.num;
    return BABE_OK;
}

extern "C" const void* babe_model_unet_plan(const void* model) {
    const Model* m = use(model, "model_unet_plan");
    return m ? m->unet_plan : nullptr;
}
extern "C" const void* babe_model_cqt_plan(const void* model) {
    const Model* m = use(model, "model_cqt_plan");
    return m ? m->cqt_plan : nullptr;
}

extern "C" int babe_model_eval_desc(const void* model, void* unet_state, babe_eval_desc* d) {
    BABE_CHECK_ARG(d, "model_eval_desc: null descriptor");
    const Model* m = use(model, "model_eval_desc");
    if (!m) return BABE_ERR_ARG;
    const NetCfg& c = m->cfg;
    memset(d, 0, sizeof *d);
    d->unet_plan = m->unet_plan, d->unet_state = unet_state, d->cqt_plan = m->cqt_plan, d->L = c.L;
    d->rff_freq = m->rff, d->rff_n = 32;
    const int dims[4] = {64, 128, 256, c.emb_dim};
    for (int i = 0; i < 3; ++i) d->emb_W[i] = m->emb_W[i], d->emb_b[i] = m->emb_b[i];
    for (int i = 0; i < 4; ++i) d->emb_dim[i] = dims[i];
    d->film_W = m->film_W, d->film_b = m->film_b, d->film_J = m->film_J;
    d->nfft = c.nfft, d->fs = (float)c.fs, d->env_inv = m->env_inv, d->tw4096 = m->tw4096;
    // the sampler's defaults of the file: predict_blind_bwe with per-clip filters (the host overrides what it wants)
    d->K = c.K;
    babe_fit_cfg& fit = d->fit;
    fit.mu_fc = (float)c.mu[0], fit.mu_A = (float)c.mu[1], fit.tol_fc = (float)c.tol[0], fit.tol_A = (float)c.tol[1];
    fit.fcmin = (float)c.fcmin, fit.fcmax = (float)c.fcmax, fit.Amin = (float)c.Amin, fit.Amax = (float)c.Amax;
    fit.max_iter = c.max_iter, fit.clamp_fc = c.clamp_fc, fit.clamp_A = c.clamp_A, fit.only_negative_A = c.only_negative_A;
    fit.weighting = c.weighting, fit.kernel = 0;
    d->blind = 1, d->shared = 0, d->hpf = c.hpf;
    d->xi = (float)c.xi, d->score_mode = 0, d->audio_len_norm = (float)c.L;
    return BABE_OK;
}
