// One Conv2d's packed images from end to end: which exist and how large each is (babe_packed_conv_plan), filling them
// (babe_packed_conv_pack) and picking a kernel from them (babe_conv2d_auto).  Both builders of a babe_packed_conv - csrc/model.hip
// and babe_amd/ops.py::PackedConv - ask the first and call the second, so they cannot disagree; the channel clauses are the
// conv_*_shape predicates of conv_common.h, which the kernels' *_supported rules call too.  Two more rules both builders and both
// UNet sequencers share live here: which convs a precision turns into bf16 products (babe_conv_splits_for) and which layers may
// take bf16 units (babe_conv2d_bf16_units_shape).  Host code only.
#include "conv_common.h"

/* Pure host arithmetic: no HIP call, no environment variable.  Slot i of bytes[] is direction i & 1 (0 the conv, 1 its input-VJP)
 * of family i / 2: direct, F(2,3), F(4,3), F(2,5)xF(4,3), F(4,5)xF(4,3). */
extern "C" int babe_packed_conv_plan(int Cout, int Cin, int KH, int KW, int splits, int nt, int nt11, int forms,
                                     babe_packed_conv_layout* out) {
    BABE_CHECK_ARG(out && Cout >= 1 && Cin >= 1 && KH >= 1 && KW >= 1 && splits >= 0 && splits <= 2 && nt >= 0 && nt11 >= 0,
                   "packed_conv_plan: bad arguments (weights [%d][%d][%d][%d], splits %d, nt %d, nt11 %d)", Cout, Cin, KH, KW, splits, nt, nt11);
    memset(out, 0, sizeof *out);
    out->splits = splits;
    // the (1,1) rule: nt11 row tiles per workgroup where the 32-channel tile counts of both directions are multiples of it
    const bool rule11 = nt == 0 && nt11 && KH * KW == 1 && cdiv(Cout, 32) % nt11 == 0 && cdiv(Cin, 32) % nt11 == 0;
    out->nt = rule11 ? nt11 : nt;
    for (int tf = 0; tf < 2; ++tf) {
        long* b = out->bytes + tf;
        if (splits) {
            b[0] = 2 * babe_conv_packed_size_bf16(Cout, Cin, KH, KW, tf, splits);
            continue;
        }
        const ConvIO io = conv_exec_io(Cout, Cin, tf);
        b[0] = 4 * babe_conv_packed_size(Cout, Cin, KH, KW, tf);
        if (KW == 3 && (forms & BABE_CONV_FORM_F23)) b[2] = 4 * babe_conv_packed_size_wino(Cout, Cin, KH, tf);
        if (KW == 3 && (forms & BABE_CONV_FORM_F43)) b[4] = 4 * babe_conv_packed_size_wino4(Cout, Cin, KH, tf);
        if ((forms & BABE_CONV_FORM_F25) && conv_wino45_shape(io.ci, io.co, KH, KW)) b[6] = 4 * babe_conv_packed_size_wino45(Cout, Cin, tf);
        if ((forms & BABE_CONV_FORM_F45) && conv_wino85_shape(io.ci, io.co, KH, KW)) b[8] = 4 * babe_conv_packed_size_wino85(Cout, Cin, tf);
    }
    // one raw image serves whichever direction executes with <= 4 output channels
    out->raw = !splits && (forms & BABE_CONV_FORM_FEWCO) && (conv_fewco_shape(Cout, KW) || conv_fewco_shape(Cin, KW));
    return BABE_OK;
}

/* Which convs a requested precision turns into bf16 products - the one statement of that rule (ops.PackedConv.splits_for and the
 * model loader both ask it).  Shapes that gain nothing from bf16 MFMA stay on the fp32 kernels under hbm_f32 (exact AND at least
 * as fast): <= 4 channels on one side (few-channel kernels), (1,1) kernels with fewer than 32 channels on one side (HBM-bound:
 * all-DMA kernel), and every (1,1) kernel of bf16x3.  Wide (1,1) kernels are MFMA-bound in fp32 and take the pipelined bf16
 * kernel under bf16.  Bad arguments: -1 with the message set. */
extern "C" int babe_conv_splits_for(int Cout, int Cin, int KH, int KW, int precision, int hbm_f32) {
    if (Cout < 1 || Cin < 1 || KH < 1 || KW < 1 || precision < BABE_PRECISION_F32 || precision > BABE_PRECISION_BF16X3) {
        babe_set_error("conv_splits_for: bad arguments (weights [%d][%d][%d][%d], precision %d)", Cout, Cin, KH, KW, precision);
        return -1;
    }
    const int splits = precision, narrow = Cout < Cin ? Cout : Cin;
    const bool k11 = KH * KW == 1;
    if (splits && hbm_f32 && (narrow <= 4 || (k11 && (splits == 2 || narrow < 32)))) return 0;
    return splits;
}

/* The static half of "this (5,3) forward conv takes its input as bf16 units" (csrc/conv_bf16p.hip, UNITS variant): what the
 * weights and the time length decide.  Alignment, the 2 GiB descriptor limits and BABE_CONV_BF16U are the call's own verdict,
 * babe_conv2d_bf16_units_supported. */
extern "C" int babe_conv2d_bf16_units_shape(const babe_packed_conv* pc, int T) {
    return pc && pc->splits == 1 && pc->KH == 5 && pc->KW == 3 && T > 0 && T % 4 == 0 && pc->Cin % 8 == 0 && pc->Cout > 32;
}

/* Per direction: direct, then F(2,3), F(4,3), F(2,5)xF(4,3), F(4,5)xF(4,3); a NULL image is skipped.  Enqueues the pack kernels
 * on `stream` and nothing else: no allocation, no wait.  (The descriptor's pointers are const for the dispatch, which only reads
 * the images; the memory is the caller's, who passes it here to be written.) */
extern "C" int babe_packed_conv_pack(const babe_packed_conv* pc, const float* w, void* stream) {
    BABE_CHECK_ARG(pc && w, "packed_conv_pack: null arguments");
    const int Cout = pc->Cout, Cin = pc->Cin, KH = pc->KH, KW = pc->KW;
    auto img = [](const void* p) { return static_cast<float*>(const_cast<void*>(p)); };
    for (int tf = 0; tf < 2; ++tf) {
        float* direct = img(tf ? pc->bwd : pc->fwd);
        if (pc->splits) {
            if (direct) BABE_TRY(babe_conv_pack_weights_bf16(w, direct, Cout, Cin, KH, KW, tf, pc->splits, stream));
            continue;
        }
        if (direct) BABE_TRY(babe_conv_pack_weights_nt(w, direct, Cout, Cin, KH, KW, tf, pc->nt, stream));
        if (float* d = img(tf ? pc->bwd_wino : pc->fwd_wino)) BABE_TRY(babe_conv_pack_weights_wino(w, d, Cout, Cin, KH, KW, tf, stream));
        if (float* d = img(tf ? pc->bwd_wino4 : pc->fwd_wino4)) BABE_TRY(babe_conv_pack_weights_wino4(w, d, Cout, Cin, KH, KW, tf, stream));
        if (float* d = img(tf ? pc->bwd_wino45 : pc->fwd_wino45)) BABE_TRY(babe_conv_pack_weights_wino45(w, d, Cout, Cin, KH, KW, tf, stream));
        if (float* d = img(tf ? pc->bwd_wino85 : pc->fwd_wino85)) BABE_TRY(babe_conv_pack_weights_wino85(w, d, Cout, Cin, KH, KW, tf, stream));
    }
    return BABE_OK;
}

/* out = alpha*conv(in[,in2]; W)*oscale + rbeta*res with the kernel chosen by the library - the one place that choice is made
 * (babe_amd/ops.py::conv2d calls this too): bf16 images, few-output-channel vector kernel, nested Winograd F(4,5)xF(4,3) /
 * F(2,5)xF(4,3) where their tiles are full, F(4,3), F(2,3), direct / pipelined (1,1); an image left NULL takes its kernel out.
 * The caller fills every field of *a except w_packed, Cin, Cout, KH, KW (taken from pc and transpose).  A requested fused
 * reduction (a->stat_mode) is formed only by the F(4,5) kernels: on return a->stat_mode is 0 if it was NOT produced.
 * A frequency bias (a->fbias) is never dropped: every *_supported rule asked here refuses it, so such a call ends in babe_conv2d_nt,
 * which adds it ((1,1) kernels) or returns an error; so does babe_conv2d_bf16. */
extern "C" int babe_conv2d_auto(babe_conv_args* a, const babe_packed_conv* pc, int transpose, void* stream) {
    BABE_CHECK_ARG(a && pc, "conv2d_auto: null arguments");
    a->Cin = transpose ? pc->Cout : pc->Cin;
    a->Cout = transpose ? pc->Cin : pc->Cout;
    a->KH = pc->KH;
    a->KW = pc->KW;
    const void* wq = transpose ? pc->bwd : pc->fwd;
    BABE_CHECK_ARG(wq, "conv2d_auto: weights not packed for this direction");
    if (!a->in2) a->cin_split = a->Cin;
    if (pc->splits) {
        a->w_packed = nullptr;
        a->stat_mode = 0;
        return babe_conv2d_bf16(a, wq, pc->splits, stream);
    }
    a->w_packed = (const float*)wq;
    const float* w45 = transpose ? pc->bwd_wino45 : pc->fwd_wino45;
    if (pc->w_raw && a->Cout <= 4 && babe_conv2d_fewco_supported(a)) {
        a->stat_mode = 0;
        return babe_conv2d_fewco(a, pc->w_raw, transpose, stream);
    }
    const float* w85 = transpose ? pc->bwd_wino85 : pc->fwd_wino85;
    if (w85 && !a->in2 && babe_conv2d_wino85_preferred(a)) return babe_conv2d_wino85(a, w85, stream);
    a->stat_mode = 0;                  // only the F(4,5) kernels form the fused reduction: tell the caller it was not produced
    if (w45 && babe_conv2d_wino45_preferred(a)) return babe_conv2d_wino45(a, w45, stream);
    if (pc->fwd_wino4 && babe_conv2d_wino4_supported(a)) return babe_conv2d_wino4(a, transpose ? pc->bwd_wino4 : pc->fwd_wino4, stream);
    if (pc->fwd_wino && babe_conv2d_wino_supported(a)) return babe_conv2d_wino(a, transpose ? pc->bwd_wino : pc->fwd_wino, stream);
    return babe_conv2d_nt(a, pc->nt, stream);
}
