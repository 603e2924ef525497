// CQTDiff+ UNet body, forward and hand-wired input-VJP, sequenced INSIDE the library from a plan handle: one C call per direction
// (babe_unet_fwd / babe_unet_vjp) instead of ~1100 op-level calls from the host language.  Same wiring, same kernels, same order
// as the Python engine (babe_amd/networks/unet_engine.py; /root/reference/networks/cqtdiff+.py:746-839 forward, ResnetBlock :452-493;
// the VJP replaces torch.autograd through the network, testing/blind_bwe_sampler.py:120) - the two are bit-identical
// (tests/test_gpu_unet_c.py) - so a non-Python host gets the whole network through the C-ABI, and the Python host sheds its
// per-evaluation enqueue time.  The images decide the arithmetic: fp32, or bf16 / bf16x3 images (babe_packed_conv::splits) that
// babe_conv2d_auto runs over the same fp32 activations; under bf16 the wide (5,3) layers take their input as bf16 units, as the
// Python engine's block_fwd does (tests/test_gpu_bf16_library.py).
//
// Memory: the caller owns everything.  Activations, saved tensors and scratch are carved from ONE workspace by a bump allocator
// (256-byte granules) that is reset by babe_unet_fwd; what the VJP needs (one tensor per dilation layer + per-layer statistics)
// stays where the forward pass put it, the VJP's own buffers are carved after it.  babe_unet_workspace_bytes runs both passes
// dry.  A state (babe_unet_state_*) holds one evaluation's bookkeeping: two clips on two streams = two states + two workspaces
// over one plan.  Host code only: every tensor operation is one of this library's extern "C" functions.
#include "common.h"
#include "../../include/babe_hip.h"
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

/* The two forms BOTH sequencers of the UNet layer path act on (this file's and babe_amd/networks/unet_engine.py's), one value
 * per process: the environment is read here, once, and nowhere else; babe_unet_form_set changes a form at run time and
 * babe_amd/forms.py (FORMS.fuse_gn_fwd / FORMS.fuse_gn) is a view of these values.
 *   BABE_FORM_FUSE_GN_FWD  the next layer's GroupNorm sums from the forward F(4,5) conv's epilogue (babe_conv_args::stat_mode 1);
 *                          on by default, BABE_FUSE_GN_FWD=0: babe_gn_partial's own pass
 *   BABE_FORM_FUSE_GN      the GroupNorm-VJP partial sums from the transposed F(4,5) conv's epilogue (stat_mode 2); off by default
 *                          (measured slower, profiles/r06_gn_fusion_experiment.txt), BABE_FUSE_GN=1 turns it on */
static std::atomic<int>& unet_form(int which) {
    static std::atomic<int> fwd{[] { const char* e = getenv("BABE_FUSE_GN_FWD"); return (e && atoi(e) == 0) ? 0 : 1; }()};
    static std::atomic<int> vjp{[] { const char* e = getenv("BABE_FUSE_GN"); return (e && atoi(e) != 0) ? 1 : 0; }()};
    return which == BABE_FORM_FUSE_GN ? vjp : fwd;
}
extern "C" int babe_unet_form_get(int which) {
    if (which != BABE_FORM_FUSE_GN_FWD && which != BABE_FORM_FUSE_GN) return -1;
    return unet_form(which).load(std::memory_order_relaxed);
}
extern "C" int babe_unet_form_set(int which, int on) {
    BABE_CHECK_ARG(which == BABE_FORM_FUSE_GN_FWD || which == BABE_FORM_FUSE_GN, "unet_form_set: no form %d", which);
    unet_form(which).store(on ? 1 : 0, std::memory_order_relaxed);
    return BABE_OK;
}

namespace {

constexpr float RS2 = 0.70710678118654752440f;
const double RS2D = 1.0 / std::sqrt(2.0);       // the Python sequencer's RS2, for scalars it multiplies before rounding
constexpr int G_GROUPS = 8;
constexpr float GN_EPS = 1e-7f;

struct View {                     // [B][C][F][T] fp32, rows contiguous (a frequency sub-range is a view)
    float* p = nullptr;
    long bs = 0, cs = 0;
    int C = 0, F = 0, T = 0;
    bool dense() const { return cs == (long)F * T && bs == (long)C * F * T; }
};
View sub_f(const View& v, int f0, int nf) { View r = v; r.p = v.p + (long)f0 * v.T; r.F = nf; return r; }
View sub_c(const View& v, int c0, int nc) { View r = v; r.p = v.p + (long)c0 * v.cs; r.C = nc; return r; }

struct Saved { View z; float* stats; float* scale; float* gate; };
// what an attention branch's forward leaves for its VJP (unet_engine.py: _State.attn); bucket: the table of this time length
struct SavedAttn { View z; float* stats; float* scale; float* gate; float* a1; float* qk; float* o; float* lse; const int* bucket; };

// The plan: the caller's descriptor, with every attention branch copied next to it (babe_unet_block::attn points into `at`) and
// the host data of its bucket-table kernel.  A plan handle is read as its descriptor (the first member).
struct AttnPlan { babe_unet_attn a; babe_attn_bucket_thr thr; };
struct UnetPlan {
    babe_unet_plan_desc d;
    AttnPlan at[17];              // main_blk[8], mid_blk, up_blk[8]
    int nat = 0;
};

}  // namespace

struct babe_unet_state_s {
    int B = 0, Ts[8] = {};
    float* ws = nullptr;
    size_t cap = 0, off = 0, high = 0;
    bool dry = false;
    float* scr_a = nullptr;
    size_t scr_a_n = 0;
    void* units = nullptr;         // the bf16 units of the layer being run (babe_scale_gelu_units), grown like scr_a
    size_t units_n = 0;            // in floats
    Saved saved[6][8][8];          // [kind][index][layer]: kinds 0 init, 1 main, 2 up_out, 3 up_blk, 4 mid_blk, 5 mid_out
    SavedAttn attn[6 * 8];         // [kind * 8 + index]: the attention branch of that block
    struct { int T; babe_attn_bucket_thr thr; int* tab; } buckets[17];      // the bucket tables this forward has built ...
    int nbuckets = 0;              // ... one per distinct (time length, thresholds)
    View hs[8];
    const float* film = nullptr;
    long film_bs = 0;
    bool have_fwd = false;
};

namespace {

struct Ctx {
    const babe_unet_plan_desc* P;
    babe_unet_state_s* S;
    hipStream_t st;
    int err = 0;
    int B() const { return S->B; }
    bool dry() const { return S->dry; }
    float* alloc(size_t nfloat) {
        // (+ an odd number of 256-byte granules: tensor sizes here are large powers of two times small integers, and operands
        // that start at multiples of the same power of two walk the HBM channels in lockstep)
        // (BABE_UNET_SKEW overrides the 4352 bytes; rounded to a multiple of 256 so that every carved buffer keeps the alignment the
        // float4 / LDS-DMA kernels need, negative values read as 0)
        static const size_t skew = [] {
            const char* e = getenv("BABE_UNET_SKEW");
            long v = e ? atol(e) : 4352L;
            if (v < 0) v = 0;
            return (size_t)((v + 255) / 256 * 256);
        }();
        const size_t bytes = ((nfloat * 4 + 255) & ~(size_t)255) + skew;
        float* p = S->ws ? reinterpret_cast<float*>(reinterpret_cast<char*>(S->ws) + S->off) : nullptr;
        S->off += bytes;
        if (S->off > S->high) S->high = S->off;
        if (!S->dry && S->off > S->cap && !err) {
            babe_set_error("unet: workspace too small (%zu bytes needed so far, %zu given; ask babe_unet_workspace_bytes)", S->off, S->cap);
            err = BABE_ERR_ARG;
        }
        return p;
    }
    View buf(int C, int F, int T) {
        View v;
        v.p = alloc((size_t)B() * C * F * T);
        v.C = C; v.F = F; v.T = T; v.cs = (long)F * T; v.bs = (long)C * F * T;
        return v;
    }
    // stack discipline for the VJP's temporaries: what a level needs only while it runs is carved after a mark and given back, so
    // the next level reuses the same (cache-warm) bytes - what the caching allocator did for the Python-sequenced engine
    size_t mark() const { return S->off; }
    void release(size_t m) { S->off = m; }
    float* scratch_a(size_t n) {
        if (n > S->scr_a_n) { S->scr_a = alloc(n); S->scr_a_n = n; }
        return S->scr_a;
    }
    // B * nu 16-byte units (nu = babe_units_size) = B * nu * 8 int16
    void* scratch_units(size_t nu) {
        const size_t n = (size_t)B() * nu * 4;
        if (n > S->units_n) { S->units = alloc(n); S->units_n = n; }
        return S->units;
    }
    void ck(int e) { if (e && !err) err = e; }

    // ---- ops (each = one extern "C" call of this library; nothing runs in a dry pass or after an error)
    // stat_cg / stat_part: also form the GroupNorm sums of the output in the conv's epilogue (babe_conv_args::stat_mode 1); returns
    // true if the kernel that ran the conv produced them (only the F(4,5) kernels do)
    // the argument block of out = alpha * conv(x[, x2]) * oscale + rbeta * res (babe_conv2d_auto fills in the weight's shape)
    babe_conv_args conv_args(const View& x, const View& out, int dil, const View* x2, const View* res, const float* in_scale,
                             const float* oscale, float alpha, float rbeta, const float* fbias = nullptr) const {
        babe_conv_args a;
        memset(&a, 0, sizeof a);
        a.in = x.p; a.in_bs = x.bs; a.in_cs = x.cs;
        if (x2) { a.in2 = x2->p; a.in2_bs = x2->bs; a.in2_cs = x2->cs; a.cin_split = x.C; }
        a.out = out.p; a.out_bs = out.bs; a.out_cs = out.cs;
        if (res) { a.res = res->p; a.res_bs = res->bs; a.res_cs = res->cs; }
        a.in_scale = in_scale; a.oscale = oscale; a.alpha = alpha; a.rbeta = rbeta; a.fbias = fbias;
        a.B = B(); a.F = x.F; a.T = x.T; a.dil = dil;
        return a;
    }
    bool conv(const View& x, const babe_packed_conv& pc, const View& out, int dil, bool transpose, const View* x2, const View* res,
              const float* in_scale, const float* oscale, float alpha, float rbeta, int stat_cg = 0, double* stat_part = nullptr,
              const float* fbias = nullptr) {
        if (dry() || err) return false;
        babe_conv_args a = conv_args(x, out, dil, x2, res, in_scale, oscale, alpha, rbeta, fbias);
        if (stat_part) { a.stat_mode = 1; a.stat_cg = stat_cg; a.stat_part = stat_part; }
        ck(babe_conv2d_auto(&a, &pc, transpose ? 1 : 0, st));
        return a.stat_mode == 1;
    }
    // slots per group of the fused reduction for a [C][F][T] output at this dilation (babe_conv2d_wino85_stat_slots)
    static int stat_slots(int cg, int F, int T, int dil) {
        babe_conv_args a;
        memset(&a, 0, sizeof a);
        a.stat_cg = cg; a.F = F; a.T = T; a.dil = dil;
        return babe_conv2d_wino85_stat_slots(&a);
    }
    void axpby(const View& x, const View& out, float alpha = 1.f, float beta = 0.f) {
        if (dry() || err) return;
        ck(babe_axpby4d(x.p, x.bs, x.cs, out.p, out.bs, out.cs, B(), x.C, x.F, x.T, alpha, beta, st));
    }
    static bool al16(const View& v) { return ((uintptr_t)v.p & 15) == 0 && v.bs % 4 == 0 && v.cs % 4 == 0; }
    void axpby2(const View& x, const View& y, const View& out, float alpha, float beta) {
        if (dry() || err) return;
        if (((long)x.F * x.T) % 4 == 0 && al16(x) && al16(y) && al16(out))
            ck(babe_axpby2_4d(x.p, x.bs, x.cs, y.p, y.bs, y.cs, out.p, out.bs, out.cs, B(), x.C, x.F, x.T, alpha, beta, st));
        else {
            axpby(x, out, alpha);
            axpby(y, out, beta, 1.f);
        }
    }
    // mode 0 down, 1 up, 2 down^T, 3 up^T; T argument of the C function = the forward op's input length
    void resample(const View& x, const View& out, int mode, float alpha = 1.f, float beta = 0.f, const View* res = nullptr) {
        if (dry() || err) return;
        const int T = mode == 0 || mode == 1 ? x.T : (mode == 2 ? x.T * 2 : x.T / 2);
        if (res) {
            if (al16(*res) && al16(out)) {
                ck(babe_resample_res(x.p, x.bs, x.cs, res->p, res->bs, res->cs, out.p, out.bs, out.cs, B(), x.C, x.F, T, mode, alpha, beta, st));
                return;
            }
            axpby(*res, out);
        }
        ck(babe_resample(x.p, x.bs, x.cs, out.p, out.bs, out.cs, B(), x.C, x.F, T, mode, alpha, beta, st));
    }
    static int splits(long n) { return (int)babe_gn_splits(n); }      // split count of a GroupNorm group of n elements
    const float* film_at(int off) const { return S->film + off; }

    // ---- the time-attention branch of a ResnetBlock (unet_engine.py attn_fwd / attn_vjp, launch for launch)
    SavedAttn& attn_rec(const Saved* saved) const { return S->attn[(saved - &S->saved[0][0][0]) / 8]; }
    static View view(float* p, int C, int F, int T) {
        View v;
        v.p = p; v.C = C; v.F = F; v.T = T; v.cs = (long)F * T; v.bs = (long)C * F * T;
        return v;
    }
    // the [2T-1] relative-position bucket table of this time length, built in the workspace once per forward
    const int* bucket_table(const babe_unet_attn& at, int T) {
        const babe_attn_bucket_thr& thr = reinterpret_cast<const AttnPlan&>(at).thr;       // (the plan's copy: UnetPlan::at)
        for (int i = 0; i < S->nbuckets; ++i)
            if (S->buckets[i].T == T && !memcmp(&S->buckets[i].thr, &thr, sizeof thr)) return S->buckets[i].tab;
        int* tab = reinterpret_cast<int*>(alloc((size_t)2 * T - 1));
        if (!dry() && !err) ck(babe_attn_bucket_table(&thr, T, tab, st));
        auto& e = S->buckets[S->nbuckets++];                 // (at most one per attention branch: 17)
        e.T = T; e.thr = thr; e.tab = tab;
        return tab;
    }
    // z' = (gate2 * proj_out(attention(...)) + z) / sqrt2; what attn_vjp needs stays in the workspace (rec)
    View attn_fwd(const babe_unet_block& blk, SavedAttn& rec, const View& z) {
        const babe_unet_attn& at = *blk.attn;
        const int N = blk.N, H = at.H, Fq = z.F, T = z.T;
        if (Fq != at.F && !err) {
            babe_set_error("unet: an attention branch built for F=%d runs at F=%d", at.F, Fq);
            err = BABE_ERR_ARG;
        }
        const long n = (long)(N / G_GROUPS) * Fq * T;
        const int Sp = splits(n);
        double* part = reinterpret_cast<double*>(alloc((size_t)B() * G_GROUPS * Sp * 2 * 2));
        float* stats = alloc((size_t)B() * G_GROUPS * 3);
        float* scale = alloc((size_t)B() * N);
        View a1 = buf(H, Fq, T);
        View qk = view(alloc((size_t)B() * 2 * H * Fq * T), 2 * H * Fq, 1, T);
        View o = buf(H, Fq, T);
        float* lse = alloc((size_t)B() * H * T);
        const int* bucket = at.emb ? bucket_table(at, T) : nullptr;
        float* gate;
        if (B() == 1) gate = const_cast<float*>(film_at(at.film_gate));
        else gate = alloc((size_t)B() * N);
        View zn = buf(N, Fq, T);
        rec = SavedAttn{z, stats, scale, gate, a1.p, qk.p, o.p, lse, bucket};
        if (dry() || err) return zn;
        ck(babe_gn_partial(z.p, part, B(), G_GROUPS, n, Sp, st));
        ck(babe_gn_finalize(part, at.gamma, film_at(at.film_aff), S->film_bs, stats, scale, B(), N, G_GROUPS, n, Sp, GN_EPS, st));
        conv(z, at.proj_in, a1, 1, false, nullptr, nullptr, scale, nullptr, 1.f, 0.f);
        conv(view(a1.p, H * Fq, 1, T), at.qk, qk, 1, false, nullptr, nullptr, nullptr, nullptr, 1.f, 0.f);
        if (!err)
            ck((P->attn_core == 2 ? babe_attn_fwd_bf16 : babe_attn_fwd)(qk.p, at.qk_bias, a1.p, bucket, at.emb, at.emb ? at.num_buckets : 0, o.p,
                                                                        lse, B(), H, Fq, T, at.scale, st));
        if (B() > 1 && !err) ck(babe_axpby4d(film_at(at.film_gate), S->film_bs, 0, gate, N, 0, B(), 1, 1, N, 1.f, 0.f, st));
        conv(o, at.proj_out, zn, 1, false, nullptr, &z, nullptr, gate, RS2, RS2);
        return zn;
    }
    // gz <- gradient w.r.t. the branch's input z, given cd * gz = gradient w.r.t. its output z' (in place).  The scalars are formed
    // in double and rounded once, as the Python sequencer's RS2 * c is
    void attn_vjp(const babe_unet_block& blk, const SavedAttn& rec, const View& gz, double cd) {
        const babe_unet_attn& at = *blk.attn;
        const View& z = rec.z;
        const int N = blk.N, H = at.H, Fq = z.F, T = z.T;
        const float rc = (float)(RS2D * cd);
        const size_t m = mark();
        View dout = buf(H, Fq, T);
        View dqk = view(alloc((size_t)B() * 2 * H * Fq * T), 2 * H * Fq, 1, T);
        View dv = buf(H, Fq, T);
        float* D = alloc((size_t)B() * H * T);
        View da1 = view(alloc((size_t)B() * H * Fq * T), H * Fq, 1, T);
        View da0 = buf(N, Fq, T);
        const int Sp = splits((long)(N / G_GROUPS) * Fq * T);
        double* part = reinterpret_cast<double*>(alloc((size_t)B() * G_GROUPS * Sp * 2));
        release(m);
        if (dry() || err) return;
        conv(gz, at.proj_out, dout, 1, true, nullptr, nullptr, rec.gate, nullptr, rc, 0.f);
        if (!err)
            ck((P->attn_core == 2 ? babe_attn_vjp_bf16 : babe_attn_vjp)(rec.qk, at.qk_bias, rec.a1, rec.bucket, at.emb, at.emb ? at.num_buckets : 0,
                                                                        rec.o, rec.lse, dout.p, D, dqk.p, dv.p, B(), H, Fq, T, at.scale, st));
        const View dvf = view(dv.p, H * Fq, 1, T);
        conv(dqk, at.qk, da1, 1, true, nullptr, &dvf, nullptr, nullptr, 1.f, 1.f);
        conv(view(da1.p, H, Fq, T), at.proj_in, da0, 1, true, nullptr, nullptr, nullptr, nullptr, 1.f, 0.f);
        if (err) return;
        ck(babe_gn_bwd_partial_nogelu(z.p, da0.p, rec.scale, part, B(), N, G_GROUPS, (long)Fq * T, Sp, st));
        ck(babe_gn_bwd_apply_nogelu(z.p, da0.p, gz.p, rec.scale, rec.stats, part, gz.p, rc, B(), N, G_GROUPS, (long)Fq * T, Sp, GN_EPS, st));
    }

    // ---- ResnetBlock (unet_engine.py block_fwd / block_vjp)
    // fold (an output head): the caller's next step is fold = RS2 * out + RS2 * fold; a block that runs as the fused pass
    // (babe_pw_block_supported) does that itself, writes fold instead of out and sets *folded
    View block_fwd(const babe_unet_block& blk, Saved* saved, const View& x, const View& out, const View* x2,
                   const View* fold = nullptr, bool* folded = nullptr) {
        const int N = blk.N, Fq = x.F, T = x.T;
        bool pw = false;                         // the block ran as one fused pass (csrc/pw_block.hip)
        View z;
        if (blk.proj_in.Cout) {
            z = buf(N, Fq, T);
            conv(x, blk.proj_in, z, 1, false, x2, nullptr, nullptr, nullptr, 1.f, 0.f, 0, nullptr, blk.fb_proj_in);
        } else if (x.dense()) {
            z = x;
        } else {
            z = buf(N, Fq, T);
            axpby(x, z);
        }
        if (blk.attn) z = attn_fwd(blk, attn_rec(saved), z);
        // bf16 images: the GELU output goes to the wide (5,3) convs as bf16 units (half the bytes, both conv operands by LDS-DMA).
        // The buffer is carved wherever the static rule holds, whatever the per-layer verdict will be, so that
        // babe_unet_workspace_bytes does not depend on it; an fp32 plan never carves it.
        const bool units = blk.nd > 0 && babe_conv2d_bf16_units_shape(&blk.H[0], T) && z.dense();
        const long nu = units ? babe_units_size(N, Fq, T) : 0;
        void* au = units ? scratch_units((size_t)nu) : nullptr;
        double* zpart = nullptr;                 // GroupNorm sums of z formed by the conv that wrote it (zS slots per group; 0: none)
        int zS = 0;
        for (int d = 0; d < blk.nd; ++d) {
            // gate = film[:, goff : goff + N] made contiguous ([B][N]: the conv's oscale / the VJP's in_scale)
            float* gate;
            if (B() == 1) gate = const_cast<float*>(film_at(blk.film_gate[d]));       // one row IS contiguous (the caller keeps film alive until the VJP)
            else {
                gate = alloc((size_t)B() * N);
                if (!dry() && !err) ck(babe_axpby4d(film_at(blk.film_gate[d]), S->film_bs, 0, gate, N, 0, B(), 1, 1, N, 1.f, 0.f, st));
            }
            View znew = buf(N, Fq, T);
            float* a = scratch_a((size_t)B() * N * Fq * T);
            const long n = (long)(N / G_GROUPS) * Fq * T;
            const int Sp = splits(n);
            double* part = reinterpret_cast<double*>(alloc((size_t)B() * G_GROUPS * Sp * 2 * 2));
            float* stats = alloc((size_t)B() * G_GROUPS * 3);
            float* scale = alloc((size_t)B() * N);
            const int dil = blk.k53 ? (1 << d) : 1, cg = N / G_GROUPS;
            // the library's own verdict on the units call (ops.units_args: in_bs = units per item, in_cs = per 8-channel group, no
            // second source, no in_scale), asked BEFORE writing units
            babe_conv_args ua{};
            bool take_units = false;
            if (units && !dry() && !err) {
                ua = conv_args(z, znew, dil, nullptr, &z, nullptr, gate, RS2, RS2);
                ua.in = static_cast<const float*>(au); ua.in_bs = nu; ua.in_cs = nu / (N / 8);
                ua.Cin = ua.Cout = ua.cin_split = N; ua.KH = blk.H[d].KH; ua.KW = blk.H[d].KW;
                take_units = babe_conv2d_bf16_units_supported(&ua) != 0;
            }
            // a k = (1,1) block the library's rule takes: GroupNorm sums, then ONE pass for the rest of the block.  Everything is
            // carved as for the layer-by-layer form, so that babe_unet_workspace_bytes does not depend on the switch
            babe_pw_args pa;
            memset(&pa, 0, sizeof pa);
            if (blk.nd == 1 && !blk.k53 && !blk.attn && !dry() && !err) {
                pa.B = B(); pa.F = Fq; pa.T = T; pa.S = Sp;
                pa.plan_splits = P->main_blk[0].H[0].splits;                     // the (5,3) layers carry the network's precision
                pa.z = z.p; pa.z_bs = z.bs; pa.z_cs = z.cs;
                if (blk.proj_in.Cout) { pa.x = x.p; pa.x_bs = x.bs; pa.x_cs = x.cs; }
                const View& o = fold ? *fold : out;
                pa.out = o.p; pa.out_bs = o.bs; pa.out_cs = o.cs;
                if (fold) { pa.add = fold->p; pa.add_bs = fold->bs; pa.add_cs = fold->cs; }
                pa.part = part; pa.film = S->film; pa.film_bs = S->film_bs; pa.gate = gate; pa.stats = stats; pa.scale = scale;
                pw = !x2 && babe_pw_block_supported(&blk, &pa, 0) != 0;
            }
            if (pw) {
                ck(babe_gn_partial(z.p, part, B(), G_GROUPS, n, Sp, st));
                ck(babe_pw_block_fwd(&blk, &pa, st));
                if (fold && folded) *folded = true;
            } else if (take_units) {
                ck(babe_gn_partial(z.p, part, B(), G_GROUPS, n, Sp, st));
                ck(babe_gn_finalize(part, blk.gamma[d], film_at(blk.film_aff[d]), S->film_bs, stats, scale, B(), N, G_GROUPS, n, Sp, GN_EPS, st));
                ck(babe_scale_gelu_units(z.p, scale, au, B(), N, Fq, T, st));
                ck(babe_conv2d_bf16_units(&ua, blk.H[d].fwd, st));
            } else if (!dry() && !err) {
                if (!zS) ck(babe_gn_partial(z.p, part, B(), G_GROUPS, n, Sp, st));
                ck(babe_scale_gelu_fin(z.p, zS ? zpart : part, blk.gamma[d], film_at(blk.film_aff[d]), S->film_bs, stats, scale, a, B(), N,
                                       G_GROUPS, (long)Fq * T, zS ? zS : Sp, GN_EPS, st));
            }
            View av = z; av.p = a; av.cs = (long)Fq * T; av.bs = (long)N * Fq * T;
            // the next layer's GroupNorm reads znew: its sums come out of this conv's epilogue when the F(4,5) kernel runs it
            // (unet_engine.py: ops.conv2d(..., fwd_stat=))
            double* npart = nullptr;
            int nS = 0;
            // (carved whatever the form is, so that babe_unet_workspace_bytes does not depend on it: a form may change between
            // the dry pass that sized the workspace and the evaluation)
            if (d + 1 < blk.nd && blk.k53 && cg % 4 == 0) {
                nS = stat_slots(cg, Fq, T, dil);
                npart = reinterpret_cast<double*>(alloc((size_t)B() * G_GROUPS * nS * 2 * 2));
            }
            const bool made = !pw && !take_units && conv(av, blk.H[d], znew, dil, false, nullptr, &z, nullptr, gate, RS2, RS2, cg, form(BABE_FORM_FUSE_GN_FWD) ? npart : nullptr);
            zS = made ? nS : 0;                                                      // (a units layer drops the carried sums)
            zpart = npart;
            saved[d] = Saved{z, stats, scale, gate};
            z = znew;
        }
        if (blk.proj_out.Cout) {
            View zo = buf(blk.proj_out.Cout, Fq, T);
            if (!pw) conv(z, blk.proj_out, zo, 1, false, nullptr, nullptr, nullptr, nullptr, 1.f, 0.f);
            z = zo;
        }
        if (pw) return out;
        if (blk.res_conv.Cout) conv(x, blk.res_conv, out, 1, false, x2, &z, nullptr, nullptr, RS2, RS2, 0, nullptr, blk.fb_res_conv);
        else axpby2(z, x, out, RS2, RS2);
        return out;
    }
    // the transposed conv of dilation layer d, with the GroupNorm-VJP partial sums formed in its epilogue when it takes the F(4,5)
    // kernel (unet_engine.py: ops.conv2d(..., vjp_stat=)): returns the slot count S (0: not fused) and the buffer in *part
    int conv_vjp(const View& src, const babe_unet_block& blk, int d, const View& da, const Saved& sv, double** part) {
        const View& z = sv.z;
        const int dil = blk.k53 ? (1 << d) : 1, cg = z.C / G_GROUPS;
        const int Sf = cg % 4 == 0 ? stat_slots(cg, z.F, z.T, dil) : 0;
        const long n = (long)cg * z.F * z.T;
        const int Sp = splits(n);
        *part = reinterpret_cast<double*>(alloc((size_t)B() * G_GROUPS * (Sf > Sp ? Sf : Sp) * 2));     // (floats: 2 per double)
        if (dry() || err) return 0;
        babe_conv_args a = conv_args(src, da, dil, nullptr, nullptr, sv.gate, nullptr, RS2, 0.f);
        if (form(BABE_FORM_FUSE_GN) && blk.k53 && cg % 4 == 0 && z.dense() && da.dense()) {
            a.stat_mode = 2; a.stat_cg = cg; a.stat_x = z.p; a.stat_scale = sv.scale; a.stat_part = *part;
        }
        ck(babe_conv2d_auto(&a, &blk.H[d], 1, st));
        return a.stat_mode == 2 ? Sf : 0;
    }
    static bool form(int which) { return unet_form(which).load(std::memory_order_relaxed) != 0; }
    void gn_bwd(const Saved& sv, const View& da, const View& gy, const View& gx, float rbeta, const View* acc, double* part, int Sf) {
        const View& z = sv.z;
        const long n = (long)(z.C / G_GROUPS) * z.F * z.T;
        const int Sp = Sf > 0 ? Sf : splits(n);
        if (dry() || err) return;
        if (Sf <= 0) ck(babe_gn_bwd_partial(z.p, da.p, sv.scale, part, B(), z.C, G_GROUPS, (long)z.F * z.T, Sp, st));
        if (acc)          // the block's tail merged in: gx = RS2*acc + RS2*(this layer's gradient)
            ck(babe_gn_bwd_apply_merge(z.p, da.p, gy.p, sv.scale, sv.stats, part, gx.p, rbeta, B(), z.C, G_GROUPS, (long)z.F * z.T, Sp, GN_EPS, st,
                                       acc->p, RS2, RS2));
        else
            ck(babe_gn_bwd_apply(z.p, da.p, gy.p, sv.scale, sv.stats, part, gx.p, rbeta, B(), z.C, G_GROUPS, (long)z.F * z.T, Sp, GN_EPS, st));
    }
    // g_in (+)= VJP of the block w.r.t. its (concatenated) input; consume: g_out is a dense buffer that may be overwritten
    View block_vjp(const babe_unet_block& blk, const Saved* saved, const View& g_out, const View& g_in, bool accumulate, bool consume) {
        const int N = blk.N, Fq = g_out.F, T = g_out.T;
        const float beta = accumulate ? 1.f : 0.f;
        auto da_view = [&]() { View v; v.p = scratch_a((size_t)B() * N * Fq * T); v.C = N; v.F = Fq; v.T = T; v.cs = (long)Fq * T; v.bs = (long)N * Fq * T; return v; };
        if (!blk.res_conv.Cout && !blk.proj_out.Cout && !blk.proj_in.Cout && !accumulate && blk.nd > 0 && g_out.dense() && !blk.attn) {
            View gz;
            if (blk.nd > 1) gz = buf(N, Fq, T);
            View da = da_view();
            View src = g_out;
            const bool merged = g_in.dense() && al16(g_in) && al16(g_out);
            for (int d = blk.nd - 1; d >= 0; --d) {
                double* part;
                const int Sf = conv_vjp(src, blk, d, da, saved[d], &part);
                if (d == 0 && merged) {
                    gn_bwd(saved[d], da, src, g_in, RS2, &g_out, part, Sf);
                } else {
                    if (!gz.p && !gz.C) gz = buf(N, Fq, T);
                    gn_bwd(saved[d], da, src, gz, RS2, nullptr, part, Sf);
                    src = gz;
                }
            }
            if (!merged) axpby2(g_out, gz, g_in, RS2, RS2);
            return g_in;
        }
        if (blk.res_conv.Cout) conv(g_out, blk.res_conv, g_in, 1, true, nullptr, accumulate ? &g_in : nullptr, nullptr, nullptr, RS2, beta);
        else axpby(g_out, g_in, RS2, beta);
        float c = 1.f;
        View gz;
        if (blk.proj_out.Cout) {
            gz = buf(N, Fq, T);
            conv(g_out, blk.proj_out, gz, 1, true, nullptr, nullptr, nullptr, nullptr, RS2, 0.f);
        } else if (consume && g_out.dense()) {
            gz = g_out;
            c = RS2;
        } else {
            gz = buf(N, Fq, T);
            axpby(g_out, gz, RS2);
        }
        View da = da_view();
        for (int d = blk.nd - 1; d >= 0; --d) {
            double* part;
            const int Sf = conv_vjp(gz, blk, d, da, saved[d], &part);
            gn_bwd(saved[d], da, gz, gz, RS2, nullptr, part, Sf);
        }
        if (blk.attn) {
            attn_vjp(blk, attn_rec(saved), gz, c == 1.f ? 1.0 : RS2D);
            c = 1.f;
        }
        if (blk.proj_in.Cout) conv(gz, blk.proj_in, g_in, 1, true, nullptr, &g_in, nullptr, nullptr, c, 1.f);
        else axpby(gz, g_in, c, 1.f);
        return g_in;
    }

    // ---- the network (unet_engine.py forward / vjp).  C_in[j]: [B][2][bpo][T_j], index 0 = lowest octave
    void forward(const float* const* C_in, float** outs) {
        const int n = P->nocts, bpo = P->bpo;
        const int* Ns = P->Ns;
        const int* Ts = S->Ts;                     // level i time length (level 0 = the highest octave's rate... = C_in[n-1])
        auto cview = [&](int lvl) { View v; v.p = const_cast<float*>(C_in[n - 1 - lvl]); v.C = 2; v.F = bpo; v.T = Ts[lvl]; v.cs = (long)bpo * Ts[lvl]; v.bs = 2 * v.cs; return v; };
        View XC = buf(Ns[0], bpo, Ts[0]);
        View pyr_prev, X;
        for (int i = 0; i < n; ++i) {
            const View C = cview(i);
            const int Fi = bpo * (i + 1);
            block_fwd(P->init_blk[i], S->saved[0][i], C, sub_f(XC, 0, bpo), nullptr);
            View pyr;
            if (i == 0) {
                pyr = buf(2, bpo, Ts[0] / 2);
                resample(C, pyr, 0);
            } else if (i < n - 1) {
                pyr = buf(2, Fi, Ts[i] / 2);
                resample(C, sub_f(pyr, 0, bpo), 0);
                resample(pyr_prev, sub_f(pyr, bpo, Fi - bpo), 0);
            } else {
                pyr = buf(2, Fi, Ts[i]);
                axpby(C, sub_f(pyr, 0, bpo));
                axpby(pyr_prev, sub_f(pyr, bpo, Fi - bpo));
            }
            pyr_prev = pyr;
            View H = buf(Ns[i], Fi, Ts[i]);
            block_fwd(P->main_blk[i], S->saved[1][i], XC, H, nullptr);
            S->hs[i] = H;
            if (i < n - 1) {
                View XCn = buf(Ns[i], Fi + bpo, Ts[i + 1]);
                View sub = sub_f(XCn, bpo, Fi);
                resample(H, sub, 0);
                conv(pyr, P->pyr_conv[i], sub, 1, false, nullptr, &sub, nullptr, nullptr, RS2, RS2);
                XC = XCn;
            } else {
                X = buf(Ns[i], Fi, Ts[i]);
                conv(pyr, P->pyr_conv[i], X, 1, false, nullptr, &H, nullptr, nullptr, RS2, RS2);
            }
        }
        {
            View Xm = buf(X.C, X.F, X.T);
            block_fwd(P->mid_blk, S->saved[4][0], X, Xm, nullptr);
            X = Xm;
        }
        View Xout = buf(2, bpo * n, Ts[n - 1]);
        block_fwd(P->mid_out, S->saved[5][0], X, Xout, nullptr);
        for (int i = 0; i < n; ++i) {
            const int j = n - 1 - i;
            const int Fj = bpo * (j + 1);
            const int Nout = Ns[j > 0 ? j - 1 : 0];
            View R = buf(Nout, Fj, Ts[j]);
            block_fwd(P->up_blk[i], S->saved[3][i], X, R, &S->hs[j]);
            View O = buf(2, Fj, Ts[j]);
            bool folded = false;                                     // the fused head adds itself into Xout
            block_fwd(P->up_out[i], S->saved[2][i], R, O, nullptr, &Xout, &folded);
            if (!folded) axpby(O, Xout, RS2, RS2);
            View o; o.p = outs[i]; o.C = 2; o.F = bpo; o.T = Ts[j]; o.cs = (long)bpo * Ts[j]; o.bs = 2 * o.cs;
            axpby(sub_f(Xout, 0, bpo), o);
            if (j > 0) {
                View Xn = buf(Nout, Fj - bpo, Ts[j - 1]);
                resample(sub_f(R, bpo, Fj - bpo), Xn, 1);
                View Xo = buf(2, Fj - bpo, Ts[j - 1]);
                resample(sub_f(Xout, bpo, Fj - bpo), Xo, 1);
                X = Xn;
                Xout = Xo;
            }
        }
    }

    void vjp(const float* const* gouts, float** gC) {
        const int n = P->nocts, bpo = P->bpo;
        const int* Ns = P->Ns;
        const int* Ts = S->Ts;
        View gH[8];
        View gX_prev, gXO_prev;
        for (int j = 0; j < n; ++j) {
            const int i = n - 1 - j;
            const int Fj = bpo * (j + 1);
            const int Nout = Ns[j > 0 ? j - 1 : 0];
            // (what outlives the level first: the next level reads gXOn / gcat[:, :N], the encoder VJP gcat[:, N:])
            View gXOn = buf(2, Fj, Ts[j]);
            View gcat = buf(2 * Ns[j], Fj, Ts[j]);
            const size_t lvl = mark();
            View gXOp = buf(2, Fj, Ts[j]);
            View go; go.p = const_cast<float*>(gouts[i]); go.C = 2; go.F = bpo; go.T = Ts[j]; go.cs = (long)bpo * Ts[j]; go.bs = 2 * go.cs;
            axpby(go, sub_f(gXOp, 0, bpo));
            View gR = buf(Nout, Fj, Ts[j]);
            bool accumulate = false;
            if (j > 0) {
                resample(gXO_prev, sub_f(gXOp, bpo, Fj - bpo), 3);
                if (!dry() && !err) ck(babe_fill4d(gR.p, gR.bs, gR.cs, B(), Nout, bpo, Ts[j], 0.f, st));      // gR[:, :, :bpo, :] = 0
                resample(gX_prev, sub_f(gR, bpo, Fj - bpo), 3);
                accumulate = true;
            }
            View gO = buf(2, Fj, Ts[j]);
            axpby(gXOp, gO, RS2);
            block_vjp(P->up_out[i], S->saved[2][i], gO, gR, accumulate, true);
            axpby(gXOp, gXOn, RS2);
            gXO_prev = gXOn;
            block_vjp(P->up_blk[i], S->saved[3][i], gR, gcat, false, true);
            gX_prev = sub_c(gcat, 0, Ns[j]);
            gH[j] = sub_c(gcat, Ns[j], Ns[j]);
            release(lvl);
        }
        View gM = buf(Ns[n - 1], bpo * n, Ts[n - 1]);
        axpby(gX_prev, gM);
        block_vjp(P->mid_out, S->saved[5][0], gXO_prev, gM, true, true);
        View gXm = buf(gM.C, gM.F, gM.T);
        block_vjp(P->mid_blk, S->saved[4][0], gM, gXm, false, true);
        View gpyr_next, gP;
        bool have_next = false;
        for (int i = n - 1; i >= 0; --i) {
            const int Fi = bpo * (i + 1);
            const int Nin = Ns[i > 0 ? i - 1 : 0];
            // (read by the next level: gXC[:, :, bpo:] = g_P, the pyramid gradient; the level's own temporaries come after the mark)
            View gXC = buf(Nin, Fi, Ts[i]);
            View gpyr = i == n - 1 ? buf(2, Fi, Ts[i]) : buf(2, Fi, Ts[i] / 2);
            View nx;
            if (i > 0 && i < n - 1) nx = buf(2, Fi - bpo, Ts[i]);
            const size_t lvl = mark();
            View gHi = buf(Ns[i], Fi, Ts[i]);
            if (i == n - 1) {
                axpby2(gH[i], gXm, gHi, 1.f, RS2);
                conv(gXm, P->pyr_conv[i], gpyr, 1, true, nullptr, nullptr, nullptr, nullptr, RS2, 0.f);
            } else {
                resample(gP, gHi, 2, RS2, 1.f, &gH[i]);
                conv(gP, P->pyr_conv[i], gpyr, 1, true, nullptr, have_next ? &gpyr_next : nullptr, nullptr, nullptr, RS2, have_next ? 1.f : 0.f);
            }
            block_vjp(P->main_blk[i], S->saved[1][i], gHi, gXC, false, true);
            View gCi; gCi.p = gC[n - 1 - i]; gCi.C = 2; gCi.F = bpo; gCi.T = Ts[i]; gCi.cs = (long)bpo * Ts[i]; gCi.bs = 2 * gCi.cs;
            block_vjp(P->init_blk[i], S->saved[0][i], sub_f(gXC, 0, bpo), gCi, false, false);
            release(lvl);
            if (i > 0) gP = sub_f(gXC, bpo, Fi - bpo);
            if (i == n - 1) {
                axpby(sub_f(gpyr, 0, bpo), gCi, 1.f, 1.f);
                gpyr_next = sub_f(gpyr, bpo, Fi - bpo);
                have_next = true;
            } else if (i > 0) {
                resample(sub_f(gpyr, 0, bpo), gCi, 2, 1.f, 1.f);
                resample(sub_f(gpyr, bpo, Fi - bpo), nx, 2);
                gpyr_next = nx;
                have_next = true;
            } else {
                resample(gpyr, gCi, 2, 1.f, 1.f);
            }
        }
    }
};

// A descriptor arrives from ANY C-ABI host: everything the sequencer indexes with (saved[kind][i][8], H[8], gamma[8], the FiLM
// offsets) and every pointer it dereferences unconditionally is checked here, for every block of the plan.
bool block_ok(const babe_unet_block& b, bool required) {
    if (b.nd == 0 && !required) return true;
    if (b.nd < 0 || b.nd > 8) return false;
    if (required && b.nd < 1) return false;
    if (b.N < G_GROUPS || b.N % G_GROUPS) return false;
    for (int d = 0; d < b.nd; ++d) {
        if (!b.gamma[d] || b.film_aff[d] < 0 || b.film_gate[d] < 0) return false;
        const babe_packed_conv& h = b.H[d];
        if (h.Cout != b.N || h.Cin != b.N || h.KH < 1 || h.KW < 1) return false;
        if (!h.fwd && !h.w_raw && !h.fwd_wino45 && !h.fwd_wino4 && !h.fwd_wino) return false;      // no packed image at all
    }
    for (const babe_packed_conv* pc : {&b.proj_in, &b.res_conv, &b.proj_out})
        if (pc->Cout != 0 && (pc->Cout < 0 || pc->Cin < 1 || (!pc->fwd && !pc->w_raw))) return false;
    return true;
}
bool desc_ok(const babe_unet_plan_desc* d) {
    if (!d || d->nocts < 1 || d->nocts > 8 || d->bpo < 1) return false;
    for (int i = 0; i < d->nocts; ++i) {
        if (d->Ns[i] < G_GROUPS || d->Ns[i] % G_GROUPS) return false;
        if (!block_ok(d->init_blk[i], true) || !block_ok(d->main_blk[i], true) || !block_ok(d->up_blk[i], true) ||
            !block_ok(d->up_out[i], true))
            return false;
    }
    return block_ok(d->mid_blk, true) && block_ok(d->mid_out, true);
}
// One attention branch of block b, which runs at F frequency rows: what the sequencer dereferences, and the shapes the attention
// kernels take (attn_check_shape, csrc/attention_common.h).  false: the message names the field.
bool attn_ok(const babe_unet_attn& a, const babe_unet_block& b, int attn_core, int F) {
    const char* bad = nullptr;
    const auto conv11 = [](const babe_packed_conv& pc, int Cout, int Cin) {
        return pc.Cout == Cout && pc.Cin == Cin && pc.KH == 1 && pc.KW == 1 && (pc.fwd || pc.w_raw) && (pc.bwd || pc.w_raw);
    };
    if (attn_core == 0) bad = "attn_core = 0 (choose the attention core: 1 fp32, 2 bf16) while a block has an attention branch";
    else if (a.H < 1 || a.H > 64) bad = "babe_unet_attn.H (1..64 heads)";
    else if (a.F != F || a.F % 64 || a.F < 64 || a.F > 448) bad = "babe_unet_attn.F (the block's frequency rows: a multiple of 64, at most 448)";
    else if (!(a.scale > 0.f)) bad = "babe_unet_attn.scale";
    else if (!a.gamma) bad = "babe_unet_attn.gamma";
    else if (a.film_aff < 0 || a.film_gate < 0) bad = "babe_unet_attn.film_aff / film_gate";
    else if (!conv11(a.proj_in, a.H, b.N)) bad = "babe_unet_attn.proj_in (a packed (1,1) conv N -> H)";
    else if (!conv11(a.qk, 2 * a.H * a.F, a.H * a.F)) bad = "babe_unet_attn.qk (a packed (1,1) conv H*F -> 2*H*F)";
    else if (!conv11(a.proj_out, b.N, a.H)) bad = "babe_unet_attn.proj_out (a packed (1,1) conv H -> N)";
    else if (a.emb && (a.num_buckets < 4 || a.num_buckets > 64)) bad = "babe_unet_attn.num_buckets (4..64)";
    if (bad) babe_set_error("unet_plan_create: bad attention descriptor: %s", bad);
    return !bad;
}

}  // namespace

extern "C" void* babe_unet_plan_create(const babe_unet_plan_desc* desc) {
    if (!desc_ok(desc)) {
        babe_set_error("unet_plan_create: bad descriptor (1..8 octaves; every block: 1..8 dilation layers, channels a positive "
                       "multiple of 8, gamma / FiLM offsets / packed weights present)");
        return nullptr;
    }
    if (desc->attn_core < 0 || desc->attn_core > 2) {
        babe_set_error("unet_plan_create: attn_core = %d is none of 0 (no attention), 1 (fp32 core), 2 (bf16 core)", desc->attn_core);
        return nullptr;
    }
    for (int i = 0; i < 8; ++i)
        if (desc->init_blk[i].attn || desc->up_out[i].attn || desc->mid_out.attn) {
            babe_set_error("unet_plan_create: babe_unet_block.attn is set on an init block or an output head (main, middle and decoder "
                           "blocks carry attention)");
            return nullptr;
        }
    auto* p = new (std::nothrow) UnetPlan();
    if (!p) return nullptr;
    memcpy(&p->d, desc, sizeof p->d);
    const int n = desc->nocts;
    for (int k = 0; k < 2 * n + 1; ++k) {                // main_blk[0..n), mid_blk, up_blk[0..n)
        babe_unet_block& b = k < n ? p->d.main_blk[k] : (k == n ? p->d.mid_blk : p->d.up_blk[k - n - 1]);
        const int level = k < n ? k : (k == n ? n - 1 : n - 1 - (k - n - 1));
        if (!b.attn) continue;
        AttnPlan& ap = p->at[p->nat++];
        ap.a = *b.attn;
        b.attn = &ap.a;
        if (!attn_ok(ap.a, b, desc->attn_core, desc->bpo * (level + 1)) ||
            (ap.a.emb && babe_attn_bucket_thresholds(&ap.thr, ap.a.num_buckets, ap.a.max_distance) != BABE_OK)) {
            delete p;                                    // (the message is attn_ok's or babe_attn_bucket_thresholds')
            return nullptr;
        }
    }
    return p;
}
extern "C" void babe_unet_plan_destroy(void* plan) { delete static_cast<UnetPlan*>(plan); }
extern "C" void* babe_unet_state_create(void) { return new babe_unet_state_s(); }
extern "C" void babe_unet_state_destroy(void* st) { delete static_cast<babe_unet_state_s*>(st); }

static int unet_set_shape(babe_unet_state_s* S, const babe_unet_plan_desc* P, int B, const int* T_oct) {
    BABE_CHECK_ARG(B > 0 && T_oct, "unet: bad batch / octave lengths");
    S->B = B;
    for (int i = 0; i < P->nocts; ++i) {
        S->Ts[i] = T_oct[P->nocts - 1 - i];                 // level i = octave n-1-i (index 0 of T_oct = lowest octave)
        BABE_CHECK_ARG(S->Ts[i] >= 8 && S->Ts[i] % 2 == 0, "unet: octave length %d unsupported (even, >= 8: the resamplers)", S->Ts[i]);
    }
    return BABE_OK;
}

/* bytes of workspace one evaluation (forward + VJP) needs for batch B and octave lengths T_oct[nocts] (index 0 = lowest octave) */
extern "C" long babe_unet_workspace_bytes(const void* plan, int B, const int* T_oct) {
    if (!plan) return -1;
    babe_unet_state_s S;
    const auto* P = static_cast<const babe_unet_plan_desc*>(plan);
    if (unet_set_shape(&S, P, B, T_oct)) return -1;
    S.dry = true;
    Ctx c{P, &S, nullptr};
    float* dummy[8] = {};
    const float* cdummy[8] = {};
    c.forward(cdummy, dummy);
    c.vjp(cdummy, dummy);
    // exactly what the two passes carve (a multiple of the 256-byte granule; every buffer carries its own skew of slack behind it):
    // a workspace one granule smaller is refused by the evaluation ("workspace too small")
    return (long)S.high;
}

/* outs[i] / C_in[j]: caller-owned [B][2][bpo][T] tensors (index 0 = lowest octave); film: [B][J] FiLM vector of every layer
 * (babe_linear of the embedding), row stride film_bs.  The state keeps what babe_unet_vjp needs inside `workspace`, which must
 * stay untouched until the VJP (or the next forward) has run. */
extern "C" int babe_unet_fwd(const void* plan, void* state, const float* const* C_in, const float* film, long film_bs, int B,
                             const int* T_oct, void* workspace, long workspace_bytes, float* const* outs, void* stream) {
    BABE_CHECK_ARG(plan && state && C_in && film && outs && workspace, "unet_fwd: null arguments");
    BABE_CHECK_ARG(((uintptr_t)workspace & 255) == 0, "unet_fwd: workspace must be 256-byte aligned");
    const auto* P = static_cast<const babe_unet_plan_desc*>(plan);
    auto* S = static_cast<babe_unet_state_s*>(state);
    if (int e = unet_set_shape(S, P, B, T_oct)) return e;
    S->ws = static_cast<float*>(workspace); S->cap = (size_t)workspace_bytes; S->off = 0; S->high = 0; S->dry = false;
    S->scr_a = nullptr; S->scr_a_n = 0; S->units = nullptr; S->units_n = 0; S->nbuckets = 0; S->film = film; S->film_bs = film_bs; S->have_fwd = false;
    Ctx c{P, S, (hipStream_t)stream};
    c.forward(C_in, const_cast<float**>(outs));
    if (c.err) return c.err;
    S->have_fwd = true;
    return BABE_OK;
}

/* gC[j] (+)= gradient w.r.t. C_in[j] given gouts[i] = gradient w.r.t. outs[i]; overwrites gC.  One VJP per forward. */
extern "C" int babe_unet_vjp(const void* plan, void* state, const float* const* gouts, float* const* gC, void* stream) {
    BABE_CHECK_ARG(plan && state && gouts && gC, "unet_vjp: null arguments");
    const auto* P = static_cast<const babe_unet_plan_desc*>(plan);
    auto* S = static_cast<babe_unet_state_s*>(state);
    BABE_CHECK_ARG(S->have_fwd, "unet_vjp: no forward pass in this state");
    Ctx c{P, S, (hipStream_t)stream};
    c.vjp(gouts, const_cast<float**>(gC));
    S->have_fwd = false;
    return c.err;
}
