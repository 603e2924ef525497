/* babe_hip.h — C-ABI of the MI355X (gfx950) kernels behind the BABE blind-BWE hot path.
 *
 * The reference (eloimoliner/BABE) has no FFI: its "plug-in" boundary is Python classes
 * (utils/setup.py:47-96).  Each entry point below replaces the ATen call(s) cited beside it.
 * Conventions: raw device pointers (fp32 unless noted), explicit shapes/strides (in ELEMENTS),
 * hipStream_t passed as void*, every call is asynchronous on that stream, returns 0 on success
 * or a negative code (message: babe_last_error()).  The library never allocates on the hot
 * path; the caller owns all buffers and workspaces.
 */
#ifndef BABE_HIP_H
#define BABE_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

const char* babe_version(void);
const char* babe_last_error(void);

/* Strided 4-D tensor view [B][C][F][T], T contiguous, row stride = T. */
typedef struct { float* p; long bs; long cs; } babe_view;

/* ---- Conv2d "same", no bias: networks/cqtdiff+.py:79-88 (F.conv2d) ------------------------
 * w_packed: [KH][KW][CinP][CoutP] from babe_conv_pack_weights (CinP = ceil8(Cin), CoutP = ceil32(Cout)).
 * Input channels [0,cin_split) come from `in`, [cin_split,Cin) from `in2` (torch.cat dim=1, :814).
 * out = alpha * acc * oscale[b,co] * (in_scale folded per input channel) + rbeta * res      */
typedef struct {
    const float* in;  long in_bs,  in_cs;
    const float* in2; long in2_bs, in2_cs; int cin_split;
    const float* w_packed;
    float* out;       long out_bs, out_cs;
    const float* res; long res_bs, res_cs;
    const float* in_scale;   /* [B][Cin] or NULL  */
    const float* oscale;     /* [B][Cout] or NULL */
    float alpha, rbeta;
    int B, Cin, Cout, F, T, KH, KW, dil;
    /* Optional reduction fused into the EPILOGUE of the F(4,5) x F(4,3) kernels (babe_conv2d_wino85; every other kernel ignores
     * these fields - zero them): the sums a GroupNorm pass would otherwise re-read the freshly written output for (round 6).
     *   stat_mode 1: stat_part[((b*G + g)*S + slot)*2 + {0,1}] = sum, sum of squares of the slot's outputs (the values stored in
     *                out) - the partial sums of the NEXT layer's GroupNorm, in the layout babe_scale_gelu_fin / babe_gn_finalize read
     *                with that S (what babe_gn_partial would re-read out for).
     *   stat_mode 2: stat_part[(b*G + g)*S + slot] = sum over the slot's outputs y of y * u * gelu'(u), u = stat_scale[b][c] *
     *                stat_x[b][c][f][t] - the S_g partial sums of the GroupNorm / FiLM / GELU input-VJP (babe_gn_bwd_partial) for
     *                the transposed conv that writes da; stat_x: dense [B][Cout][F][T] (the layer's saved input), stat_scale [B][Cout].
     * G = Cout / stat_cg groups of stat_cg channels (a multiple of 4); S = babe_conv2d_wino85_stat_slots(a) slots per group, each
     * written exactly once (deterministic), in the layout babe_gn_bwd_apply reads with that S. */
    int stat_mode, stat_cg;
    const float* stat_x; const float* stat_scale; double* stat_part;
    /* Optional bias per output channel and FREQUENCY ROW, dense [Cout][F], NULL = none: out = alpha * oscale * (acc + fbias[co][f]) +
     * rbeta * res.  The folded frequency encodings of the UNet's init blocks (cqtdiff+.py:213-263, 675: the 64 encoding channels
     * are constant over batch and time, so their share of a (1,1) conv is this table, babe_fenc_bias).  Implemented by the fp32
     * (1,1) kernels behind babe_conv2d / babe_conv2d_nt (KH = KW = 1); every other conv entry point returns an error for a
     * non-NULL fbias, and babe_conv2d_auto never picks one of them for such a call. */
    const float* fbias;
} babe_conv_args;
/* slots per GroupNorm group the fused reduction writes: (row-quad x time tiles of one batch element) * stat_cg / sg, sg = the largest
 * of 16, 8, 4 that divides stat_cg */
int babe_conv2d_wino85_stat_slots(const babe_conv_args* a);
int babe_conv2d(const babe_conv_args* a, void* stream);
/* w: [Cout][Cin][KH][KW] (reference layout) -> packed; transpose_flip=1 builds the bwd-data weights
 * (w'[ci][co][KH-1-kh][KW-1-kw]) so that babe_conv2d computes the input-VJP (replaces autograd's
 * convolution_backward for the input).  dst size = KH*KW*ceil8(Cin')*ceil32(Cout') floats. */
int babe_conv_pack_weights(const float* w, float* dst, int Cout, int Cin, int KH, int KW,
                           int transpose_flip, void* stream);
long babe_conv_packed_size(int Cout, int Cin, int KH, int KW, int transpose_flip);
/* Same with an explicit row-tile count per workgroup (nt x 32 output channels; 0 = the default, the largest of 4..1 that
 * divides ceil32(Cout)/32).  nt = 1 gives the most workgroups: used for the dense DFT stages of the length-L real FFT,
 * whose "positions" are only a few hundred (networks/cqtdiff+.py:743 -> CQT_nsgt.fwd -> torch.fft).  Weights packed with
 * a given nt must be used with the same nt. */
int babe_conv2d_nt(const babe_conv_args* a, int nt, void* stream);
int babe_conv_pack_weights_nt(const float* w, float* dst, int Cout, int Cin, int KH, int KW, int transpose_flip, int nt,
                              void* stream);
/* bf16-MFMA variants (fp32 tensors in HBM, bf16 operands, fp32 accumulate): splits=1 plain bf16 (configs #3-#5),
 * splits=2 "bf16x3" (hi/lo split of both operands, three products: 16-bit-mantissa multiplies).
 * w_bf16 from babe_conv_pack_weights_bf16: [splits][KH][KW][ceil16(Cin)/8][ceil32(Cout)][8] bf16. */
int babe_conv2d_bf16(const babe_conv_args* a, const void* w_bf16, int splits, void* stream);
int babe_conv_pack_weights_bf16(const float* w, void* dst, int Cout, int Cin, int KH, int KW, int transpose_flip,
                                int splits, void* stream);
long babe_conv_packed_size_bf16(int Cout, int Cin, int KH, int KW, int transpose_flip, int splits);
/* bf16 "units" path for the forward (5,3) layers under precision='bf16' (csrc/conv_bf16p.hip, UNITS variant).  The
 * producer of a conv's input - GroupNorm scale * GELU, networks/cqtdiff+.py:472-482 - writes it as bf16 units instead of
 * fp32: a unit = 8 consecutive channels of one (f, t) = 16 bytes = one lane's MFMA operand fragment; tensor layout
 * [B][C/8][F][4 planes][T/4 + 1] units, plane p entry j = time step 4j + p - 1 (t = -1 and t >= T stored as zeros).
 * babe_units_size = units per batch item.  babe_conv2d_bf16_units takes such a tensor as a->in (a->in_bs / a->in_cs = units
 * per batch item / per 8-channel group = F*4*(T/4+1); no second source, no in_scale) and moves BOTH operands by LDS-DMA;
 * result identical to babe_conv2d_bf16 (splits = 1) on the fp32 tensor.  Needs KH x KW = 5 x 3, T % 4 == 0, Cin % 8 == 0,
 * Cout > 32, 16-byte aligned out / res rows (babe_conv2d_bf16_units_supported: the verdict on one call, BABE_CONV_BF16U included;
 * what the weights and the time length alone decide is babe_conv2d_bf16_units_shape, declared with babe_packed_conv below).  Both
 * UNet sequencers - babe_amd/networks/unet_engine.py and csrc/unet_engine.hip - ask the static rule per block and the verdict per
 * layer, and launch babe_gn_partial, babe_gn_finalize, babe_scale_gelu_units, babe_conv2d_bf16_units in that order. */
long babe_units_size(int C, int F, int T);
int babe_scale_gelu_units(const float* x, const float* scale, void* units, int B, int C, int F, int T, void* stream);
int babe_conv2d_bf16_units_supported(const babe_conv_args* a);
int babe_conv2d_bf16_units(const babe_conv_args* a, const void* w_bf16, void* stream);
/* Winograd F(2,3)-along-time variant of the exact-fp32 conv for KW == 3 (csrc/conv_wino.hip): 2/3 of the MFMA work,
 * same result up to fp32 rounding.  w_wino from babe_conv_pack_weights_wino: [KH][ceil8(Cin)][ceil32(Cout)][4].
 * babe_conv2d_wino_supported() tells whether a problem qualifies (even T, aligned rows, tileable Cout). */
int babe_conv2d_wino(const babe_conv_args* a, const float* w_wino, void* stream);
int babe_conv2d_wino_supported(const babe_conv_args* a);
int babe_conv_pack_weights_wino(const float* w, float* dst, int Cout, int Cin, int KH, int KW, int transpose_flip,
                                void* stream);
long babe_conv_packed_size_wino(int Cout, int Cin, int KH, int transpose_flip);
/* Winograd F(4,3)-along-time variant (csrc/conv_wino4.hip): half of the direct kernel's MFMA work, fp32, about 2.5x the
 * rounding error of F(2,3) (1e-6 relative).  w_wino4 from babe_conv_pack_weights_wino4:
 * [KH][ceil8(Cin)][2][ceil32(Cout)][4].  Needs T % 4 == 0, 16-byte aligned in/out/res rows, Cout in 64, 96 or a multiple
 * of 128 (after rounding up to 32). */
int babe_conv2d_wino4(const babe_conv_args* a, const float* w_wino4, void* stream);
int babe_conv2d_wino4_supported(const babe_conv_args* a);
int babe_conv_pack_weights_wino4(const float* w, float* dst, int Cout, int Cin, int KH, int KW, int transpose_flip,
                                 void* stream);
long babe_conv_packed_size_wino4(int Cout, int Cin, int KH, int transpose_flip);
/* NESTED Winograd variant (csrc/conv_wino45.hip, round 3): F(2,5) along frequency x F(4,3) along time, 4.5 multiplies per
 * output instead of 7.5 (0.6 of the F(4,3) kernel's matrix work, 0.3 of the direct kernel's), fp32 MFMA, rounding error
 * about 3.4x the F(4,3) kernel's (2-3e-6 relative).  Replaces the same F.conv2d call (cqtdiff+.py:85) and its input-VJP.
 * w_wino45 from babe_conv_pack_weights_wino45: [3 passes][ceil8(Cin)][ceil64(Cout)][12].  Needs KH x KW = 5 x 3,
 * T % 4 == 0, T >= 64, Cin % 16 == 0, Cout > 32, 16-byte aligned in/out/res rows, ONE source (no in2), views < 1 GiB. */
/* Two tilings behind the one entry point: 64-channel tiles x 64 units (any Cout; a PADC variant skips the MFMAs of waves whose
 * channels are padding, e.g. Cout = 96) and, for Cout % 128 == 0 or Cout % 96 == 0 where they fill at least as well, 128- / 96-
 * channel tiles x 32 units that transform 16 input channels at a time.  Same arithmetic in the same order in both. */
int babe_conv2d_wino45(const babe_conv_args* a, const float* w_wino45, void* stream);
int babe_conv2d_wino45_supported(const babe_conv_args* a);   /* the kernel CAN run this problem */
int babe_conv2d_wino45_preferred(const babe_conv_args* a);   /* ... and its tiles are full enough to beat the F(4,3) kernel */
int babe_conv_pack_weights_wino45(const float* w, float* dst, int Cout, int Cin, int KH, int KW, int transpose_flip,
                                  void* stream);
long babe_conv_packed_size_wino45(int Cout, int Cin, int transpose_flip);
/* (KH,3) conv with at most 4 OUTPUT channels on the vector ALU (csrc/conv_fewco.hip): the input-VJP of the UNet's 2-channel
 * pyramid projections (cqtdiff+.py:676, 794).  w is in the REFERENCE layout, not packed: [Cout][Cin][KH][3] for
 * transpose_flip = 0; for transpose_flip = 1 the weights [Cin][Cout][KH][3] of the conv whose input-VJP is computed (a->Cin,
 * a->Cout describe the op as executed).  One source, no in_scale. */
int babe_conv2d_fewco(const babe_conv_args* a, const float* w, int transpose_flip, void* stream);
int babe_conv2d_fewco_supported(const babe_conv_args* a);
/* Measurement hook (bench.py; csrc/prof.h lists the slots): when enabled EVERY entry point of this library brackets
 * its launch with HIP events on the launch stream and tallies, per slot, the kernel time, the ALGORITHMIC bytes and flops
 * (conv: 2*B*Cout*Cin*KH*KW*F*T with the unpadded channel counts) and the flops the matrix pipe executes (Winograd
 * F(2,3): 2/3, F(4,3): 1/2 of the algorithmic count).  babe_prof_read() waits for the events, fills arrays of
 * babe_prof_nslots() entries and resets.  babe_prof_dispatch_counts() is always on: launches per slot, i.e. which
 * kernel a conv call really dispatched to.  Diagnostics only; single host thread. */
int babe_prof_nslots(void);
const char* babe_prof_slot_name(int slot);
int babe_prof_enable(int on);          /* on < 0: query, returns 1 / 0 */
int babe_prof_conv_slot(int slot);      /* >= 0: tally conv launches in that slot (the CQT's dense DFT stages); -1: off */
int babe_prof_read(double* ms, double* bytes, double* flops, double* exec_flops, long* launches);
int babe_prof_dispatch_counts(long* counts, int reset);
/* per-launch timeline of the records pending since the last babe_prof_read (call before it): event times in ms relative to the
 * first record, slot, lane (stream index in order of first appearance), tallied flops; returns the count written (<= cap) */
long babe_prof_timeline(double* t0_ms, double* t1_ms, int* slot, int* lane, double* flops, long cap);
long babe_prof_pending(void);

/* ---- BiasFreeGroupNorm + FiLM + GELU: cqtdiff+.py:147-163, :472-482 ------------------------ */
/* split count S of a GroupNorm group of n elements, as both sequencers launch it: max(1, min(64, n / 16384)) */
long babe_gn_splits(long n);
/* partial sums (double) of x and x^2 per (b,group,split): part[(b*G+g)*S+s] = {sum, sumsq} */
int babe_gn_partial(const float* x, double* part, int B, int G, long n_per_group, int S, void* stream);
/* babe_gn_partial + babe_gn_finalize in one launch (the workgroup that finishes a group last finalises it; bit-identical
 * results).  ticket: B*G ints, zero before the first use and left zero by every call; one buffer per concurrently used stream. */
int babe_gn_stats(const float* x, double* part, int* ticket, const float* gamma, const float* film, long film_bs,
                  float* stats, float* scale, int B, int C, int G, long n_per_group, int S, float eps, void* stream);
/* stats[b*G+g] = {mean, std, 1/(std+eps)}; scale[b][c] = gamma[c]*(film[b][c]+1)/(std+eps) */
int babe_gn_finalize(const double* part, const float* gamma, const float* film, long film_bs,
                     float* stats, float* scale, int B, int C, int G, long n_per_group, int S,
                     float eps, void* stream);
/* babe_gn_finalize + babe_scale_gelu in one launch (every workgroup re-derives its channel's scale from the partial sums in
 * gn_finalize's order; the first one stores scale / stats for the VJP): bit-identical to the two calls. */
int babe_scale_gelu_fin(const float* x, const double* part, const float* gamma, const float* film, long film_bs, float* stats,
                        float* scale, float* a, int B, int C, int G, long hw, int S, float eps, void* stream);
/* a = gelu(x * scale[b][c]) */
int babe_scale_gelu(const float* x, const float* scale, float* a, int B, int C, long hw, void* stream);
/* VJP pass 1: with du = da * gelu'(x*scale) (never stored): part[(b*G+g)*S+s] = sum(du * scale*(std+eps) * x) */
int babe_gn_bwd_partial(const float* x, const float* da, const float* scale, double* part,
                        int B, int C, int G, long hw, int S, void* stream);
/* VJP pass 2: gx = rbeta*gy + scale*du - (x-mean)*coef_g with du recomputed from da; coef from part and stats */
int babe_gn_bwd_apply(const float* x, const float* da, const float* gy, const float* scale,
                      const float* stats, const double* part, float* gx, float rbeta,
                      int B, int C, int G, long hw, int S, float eps, void* stream);
/* the same pass with a ResnetBlock's VJP tail merged in: gx_out = ca*acc + cb*(the gx babe_gn_bwd_apply would store) - the residual
 * path's rs2*g_out plus the main path's rs2*gz of an N -> N block, without storing gz and re-reading it (acc dense, 16-byte aligned) */
int babe_gn_bwd_apply_merge(const float* x, const float* da, const float* gy, const float* scale,
                            const float* stats, const double* part, float* gx, float rbeta,
                            int B, int C, int G, long hw, int S, float eps, void* stream,
                            const float* acc, float ca, float cb);
/* babe_gn_bwd_partial / babe_gn_bwd_apply for GroupNorm * FiLM WITHOUT the GELU (forward a = x * scale, the time-attention
 * branch's norm2): du = da.  Same arguments and partial-sum layout. */
int babe_gn_bwd_partial_nogelu(const float* x, const float* da, const float* scale, double* part, int B, int C, int G, long hw,
                               int S, void* stream);
int babe_gn_bwd_apply_nogelu(const float* x, const float* da, const float* gy, const float* scale, const float* stats,
                             const double* part, float* gx, float rbeta, int B, int C, int G, long hw, int S, float eps,
                             void* stream);

/* ---- UpDownResample ('cubic', reflect): cqtdiff+.py:549-580 (conv1d / conv_transpose1d with a
 * dense diagonal weight) as a depth-wise 8-tap polyphase FIR.  mode: 0 down, 1 up, 2 down^T, 3 up^T.
 * T = time length of the INPUT of the forward op (for the adjoints: of the forward op's input too). */
int babe_resample(const float* in, long in_bs, long in_cs, float* out, long out_bs, long out_cs,
                  int B, int C, int F, int T, int mode, float alpha, float beta, void* stream);
/* out = alpha*resample(in) + beta*res with res a separate tensor of out's shape (16-byte aligned views): the encoder VJP's
 * g_H = g_skip + rs2 * down^T(g_P) (cqtdiff+.py:776-794 backwards) without first copying g_skip into out */
int babe_resample_res(const float* in, long in_bs, long in_cs, const float* res, long res_bs, long res_cs, float* out,
                      long out_bs, long out_cs, int B, int C, int F, int T, int mode, float alpha, float beta, void* stream);

/* ---- sample-rate conversion of the file-level flows: torchaudio.functional.resample as published (Hann-windowed sinc,
 * lowpass_filter_width 6, rolloff 0.99), testing/blind_bwe_tester.py:410,744,930, testing/denoise_and_bwe_tester.py:282-289.
 * orig / new_: the two rates divided by their gcd; kernel [new_][2 width + orig] (host-built, babe_amd/resample.py);
 * krange [new_][2] = first and one-past-last non-zero tap of each phase.  out[b][i new_ + j] = sum_k kernel[j][k] xpad[b][i orig + k]
 * with xpad = x padded by (width, width + orig) zeros; L_out = ceil(new_ L_in / orig). */
int babe_resample_sinc(const float* x, long x_bs, float* out, long out_bs, int B, long L_in, long L_out, const float* kernel,
                       const int* krange, int orig, int new_, int width, void* stream);
/* Transpose of babe_resample_sinc (same kernel / krange / rates): g [B][L_out] -> out [B][L_in], a gather per input sample
 * (deterministic, no atomics).  The guidance VJP of predict_bwe(..., 'resample'). */
int babe_resample_sinc_adjoint(const float* g, long g_bs, float* out, long out_bs, int B, long L_in, long L_out,
                               const float* kernel, const int* krange, int orig, int new_, int width, void* stream);

/* ---- known degradations of predict_bwe beyond the FIR (testing/blind_bwe_sampler.py:219-230; csrc/degrade.hip) ----------
 * IIR filter with torchaudio.functional.lfilter semantics: y[n] = sum_{k=0..order} b[k] x[n-k] - sum_{k=1..order} a[k] y[n-k],
 * zero initial state; b, a [order+1] fp32 already normalised by a[0] (a[0] is not read), order 1..16; recursion state in fp64,
 * parallel over time (chunked state-space scan, exact).  clamp: output clipped to [-1, 1] (lfilter's default, biquad); the
 * forward then writes mask [B][L] = (|y| <= 1) if mask is not NULL.  adjoint=1: out = reverse(lfilter(reverse(g))), the
 * transpose; with clamp the seed is first zeroed where mask is 0 (mask required).  x and y must not alias.  Workspace:
 * babe_iir_workspace(B, L, order) bytes (-1 for bad arguments). */
long babe_iir_workspace(int B, long L, int order);
int babe_iir_filter(const float* x, long x_bs, float* y, long y_bs, int B, long L, const float* b, const float* a, int order,
                    int clamp, int adjoint, unsigned char* mask, long mask_bs, void* workspace, long workspace_bytes, void* stream);
/* Decimation x[..., 0:-1:factor]: adjoint=0 out[b][m] = in[b][m factor], m < L_dec (in has L_full samples); adjoint=1 the
 * zero-stuffing transpose, in [B][L_dec] -> out [B][L_full].  Requires (L_dec - 1) factor < L_full. */
int babe_decimate(const float* in, long in_bs, float* out, long out_bs, int B, long L_full, long L_dec, int factor, int adjoint,
                  void* stream);

/* ---- observation operators of the EDM sampler's declipping and phase-retrieval tasks (testing/edm_sampler.py:308-384;
 * csrc/edm_tasks.hip).  No atomics: repeats are bit-identical, a row never depends on B.
 * Clip A(x) = clip(x, -c, c), c >= 0.  babe_clip_residual, one pass over [B][L]: r = y - clip(x), mask [B][L] (uint8) = |x| <= c
 * (torch.clip's gradient: 1 on the closed interval), part [B][nblk] = the sums of r^2 babe_sumsq_partial(r, nblk) writes, bit for
 * bit.  babe_clip_adj: out = g where mask != 0, else 0.  16-byte loads and stores where the rows are 16-byte aligned (mask rows:
 * 4-byte), element-wise otherwise; any L. */
int babe_clip_residual(const float* x, long x_bs, const float* y, long y_bs, float c, float* r, long r_bs, unsigned char* mask,
                       long mask_bs, double* part, int nblk, int B, long L, void* stream);
int babe_clip_fwd(const float* x, long x_bs, float c, float* out, long out_bs, int B, long L, void* stream);
int babe_clip_adj(const float* g, long g_bs, const unsigned char* mask, long mask_bs, float* out, long out_bs, int B, long L,
                  void* stream);
/* STFT magnitude A(x) = |torch.stft(cat(x, zeros(win)), win, hop, window, center=False)|: frames = 1 + L / hop, samples at or
 * beyond L read as zero (no padded copy).  win a power of two in 256..4096, 1 <= hop <= win; window [win] (the host passes the
 * periodic Hamming window); tw4096 [2048][2] = exp(-2 pi i q / 4096).  Forward: mag [B][win/2+1][frames] (torch.stft's layout)
 * and spec [B][frames][win/2+1] complex, which the VJP reads.  VJP of G [B][win/2+1][frames]: per bin Z = G X / |X|, and 0
 * where |X| == 0 (torch's sqrt has a NaN gradient there); the adjoint of the one-sided real transform
 * f[n] = sum_k Re(Z_k) cos(2 pi k n / win) - Im(Z_k) sin(2 pi k n / win), interior bins NOT doubled (not irfft); the window; the
 * overlap-add into gx [B][L] as a gather, every sample summing its frames in ascending order, the padding dropped.  Workspace:
 * babe_stft_mag_workspace(B, frames, win) bytes (-1 for bad arguments). */
/* Gradient of the matrix 2-norm (largest singular value s1) of a residual r [B][rows][cols] = y - rec with respect to rec:
 * out = -u1 v1^T, by `iters` power iterations on r^T r started from u = ones (the error shrinks by (s2 / s1)^2 per iteration);
 * 0 where r is zero.  What torch.linalg.norm(y - rec, dim=(1, 2), ord=2) differentiates to: the guidance distance the
 * reference's EDM sampler applies to a 3-D observation (phase retrieval).  Workspace: babe_specnorm_workspace bytes. */
long babe_specnorm_workspace(int B, int rows, int cols);
int babe_specnorm_seed(const float* r, long r_bs, int rows, int cols, int iters, float* out, long out_bs, int B, void* workspace,
                       long workspace_bytes, void* stream);
long babe_stft_mag_workspace(int B, int frames, int win);
int babe_stft_mag_fwd(const float* x, long x_bs, long L, const float* window, int win, int hop, float* spec, float* mag, int B,
                      int frames, const float* tw4096, void* stream);
int babe_stft_mag_vjp(const float* G, const float* spec, const float* window, int win, int hop, float* gx, long gx_bs, long L,
                      int B, int frames, const float* tw4096, void* workspace, long workspace_bytes, void* stream);

/* ---- nested Winograd F(4,5) along frequency x F(4,3) along time for the same (5,3) convs as babe_conv2d_wino45 (Conv2d at
 * networks/cqtdiff+.py:79-88, 433-436): 3.0 multiplies per output instead of 4.5 (csrc/conv_wino85.hip).  Output-channel tiles of
 * 128, 96 or 64 (Cout a multiple of one of them), Cin % 16 == 0, one source; weights [2 passes][Cin/4][2][Cout/16][3][4][16][4] from
 * babe_conv_pack_weights_wino85.  _preferred: the problem is supported AND its row quads x time tiles are >= 80 % full - what
 * babe_conv2d_auto dispatches on (BABE_CONV_F45=0 in the Python host packs no F(4,5) images: everything is left to wino45). */
long babe_conv_packed_size_wino85(int Cout, int Cin, int transpose_flip);
int babe_conv_pack_weights_wino85(const float* w, float* dst, int Cout, int Cin, int KH, int KW, int transpose_flip, void* stream);
int babe_conv2d_wino85_supported(const babe_conv_args* a);
int babe_conv2d_wino85_preferred(const babe_conv_args* a);
int babe_conv2d_wino85(const babe_conv_args* a, const float* w_wino85, void* stream);
/* Form of the kernel's 128-channel tile: 12 (default; 8 multiplying + 4 transform waves, three per SIMD) or 8 (round 5: waves 0-3
 * transform and multiply).  Bit-identical outputs; BABE_W85_12W=0 selects 8 for the process. */
int babe_conv2d_wino85_set_waves(int waves);

/* ---- the whole UNet body from one call: networks/cqtdiff+.py:746-839 (forward), ResnetBlock :452-493, and its input-VJP
 * (the autograd pass of testing/blind_bwe_sampler.py:120).  csrc/unet_engine.hip sequences the op-level functions of this header
 * exactly as babe_amd/networks/unet_engine.py does (bit-identical results), whatever the images' precision: fp32 images, bf16 /
 * bf16x3 images over fp32 activations, and under bf16 the units path of the wide (5,3) layers.  All device memory is the caller's. */
typedef struct {                       /* the images of one Conv2d, as babe_packed_conv_plan lays them out; NULL = not packed */
    int Cout, Cin, KH, KW, nt, splits; /* Cout == 0: the layer does not exist; splits: 0 fp32, 1 bf16, 2 bf16x3 */
    const void *fwd, *bwd;             /* babe_conv_pack_weights_nt (fp32) or babe_conv_pack_weights_bf16 images, transpose_flip 0 / 1 */
    const float *fwd_wino, *bwd_wino, *fwd_wino4, *bwd_wino4, *fwd_wino45, *bwd_wino45;
    const float* w_raw;                /* reference layout, for babe_conv2d_fewco (<= 4 channels on one side) */
    const float *fwd_wino85, *bwd_wino85;  /* babe_conv_pack_weights_wino85 images, or NULL */
} babe_packed_conv;
/* Which images one Conv2d with weights [Cout][Cin][KH][KW] gets and how large each is - the one statement of that rule; both the
 * model loader and babe_amd/ops.py::PackedConv build their descriptors from it.  Pure host arithmetic like the packed_size
 * functions: no GPU, no environment variable.
 *   splits  0: fp32 images; 1 / 2: only fwd / bwd exist, babe_conv_pack_weights_bf16 images (2-byte elements)
 *   nt      the caller's row-tile count for the direct kernel; 0: nt11 (0 = none) for a (1,1) conv whose 32-channel tile counts
 *           are multiples of it in both directions, the library default otherwise.  The layout's nt goes into the descriptor.
 *   forms   mask of the kernel families that may get an image (a direction gets a family's image where that family's kernel
 *           takes the executed op's channels and kernel size), BABE_CONV_FORMS_ALL by default
 *   raw     set the descriptor's w_raw to the raw weights themselves (they stay the caller's memory): <= 4 channels on one side
 * bytes[i], in the order fwd, bwd, fwd_wino, bwd_wino, fwd_wino4, bwd_wino4, fwd_wino45, bwd_wino45, fwd_wino85, bwd_wino85: the
 * size of that image, 0 = the image is absent and its pointer stays NULL. */
enum { BABE_CONV_FORM_F23 = 1, BABE_CONV_FORM_F43 = 2, BABE_CONV_FORM_F25 = 4, BABE_CONV_FORM_F45 = 8, BABE_CONV_FORM_FEWCO = 16,
       BABE_CONV_FORMS_ALL = 31 };
typedef struct { int nt, splits, raw; long bytes[10]; } babe_packed_conv_layout;
int babe_packed_conv_plan(int Cout, int Cin, int KH, int KW, int splits, int nt, int nt11, int forms,
                          babe_packed_conv_layout* out);
/* The `splits` a conv with weights [Cout][Cin][KH][KW] runs with under a requested precision - the one statement of that rule
 * (ops.PackedConv.splits_for and the model loader ask it).  Host arithmetic.  With hbm_f32 != 0 (the default form
 * BABE_BF16_HBM_F32) the shapes bf16 MFMA gains nothing on stay fp32, whatever the precision: <= 4 channels on one side, a (1,1)
 * kernel with fewer than 32 channels on one side, every (1,1) kernel under bf16x3.  -1: bad arguments (babe_last_error). */
enum { BABE_PRECISION_F32 = 0, BABE_PRECISION_BF16 = 1, BABE_PRECISION_BF16X3 = 2 };
int babe_conv_splits_for(int Cout, int Cin, int KH, int KW, int precision, int hbm_f32);
/* The static half of the units rule (see babe_units_size above): may the forward of this conv at time length T take its input as
 * bf16 units?  splits == 1, 5 x 3, T % 4 == 0, Cin % 8 == 0, Cout > 32.  Host arithmetic; both UNet sequencers ask it per block
 * and then, per layer, the call's own verdict babe_conv2d_bf16_units_supported (alignment, 2 GiB limits, BABE_CONV_BF16U). */
int babe_conv2d_bf16_units_shape(const babe_packed_conv* pc, int T);
/* Fills every non-NULL image of *pc (shape, nt, splits set) from raw weights w of that shape: the per-family pack_weights calls,
 * enqueued on stream.  Allocates nothing, waits for nothing, leaves w_raw alone. */
int babe_packed_conv_pack(const babe_packed_conv* pc, const float* w, void* stream);
/* conv with the kernel chosen by the library; a->w_packed, Cin, Cout, KH, KW are filled in from pc / transpose */
int babe_conv2d_auto(babe_conv_args* a, const babe_packed_conv* pc, int transpose, void* stream);
/* The time-attention branch of a ResnetBlock (TimeAttentionBlock; babe_amd/networks/unet_engine.py::_Attn), between the block's
 * proj_in and its dilation stack:
 *   a1 = proj_in(z * scale2)   scale2 = gamma * (affine2(emb) + 1) / (std_g(z) + eps), no GELU
 *   qk = qk(a1 as [B][H*F][1][T])      o = attention(qk, V = a1)      z' = (gate2(emb) * proj_out(o) + z) / sqrt2
 * The attention core is the plan's (babe_unet_plan_desc::attn_core).  The relative-position bucket table of a time length is
 * built in the workspace by babe_attn_bucket_table from thresholds computed once at plan creation. */
typedef struct {
    int H, F;                          /* heads; features per head = the block's frequency rows (a multiple of 64, at most 448) */
    float scale;                       /* F^-1/2 */
    babe_packed_conv proj_in, qk, proj_out;   /* N -> H (1,1); H*F -> 2*H*F (1,1) on the [B][H*F][1][T] view; H -> N (1,1) */
    const float* gamma;                /* norm2's gamma [N] */
    int film_aff, film_gate;           /* offsets of affine2 / gate2 in the FiLM row */
    const float* qk_bias;              /* [2*H*F], or NULL */
    const float* emb;                  /* relative-position table [num_buckets][H], or NULL: no relative bias */
    int num_buckets, max_distance;     /* read with emb only */
} babe_unet_attn;
typedef struct {                       /* one ResnetBlock */
    int N, nd, k53;                    /* channels of the dilated stack, dilation layers (dilation 2^d when k53), (5,3) kernels? */
    babe_packed_conv proj_in, res_conv, proj_out, H[8];
    const float* gamma[8];             /* BiasFreeGroupNorm gamma of layer d, [N] */
    int film_aff[8], film_gate[8];     /* offsets of layer d's affine / gate vectors in the FiLM row */
    const float *fb_proj_in, *fb_res_conv;   /* babe_conv_args::fbias [N][bpo] of proj_in / res_conv: an init block with folded
                                              * frequency encodings (its packed convs hold the 2 signal columns); NULL: none */
    const babe_unet_attn* attn;        /* the block's time-attention branch, NULL: none.  Main, middle and decoder blocks only;
                                        * such a block never runs as the fused (1,1) pass */
} babe_unet_block;
typedef struct {
    int nocts, bpo;                    /* octaves (7), bins per octave (64) */
    int Ns[8];
    babe_unet_block init_blk[8], main_blk[8], up_out[8], up_blk[8], mid_blk, mid_out;
    babe_packed_conv pyr_conv[8];
    int attn_core;                     /* what the attention branches launch: 0 none (a block with attn is refused), 1 babe_attn_fwd /
                                        * _vjp (fp32), 2 babe_attn_fwd_bf16 / _vjp_bf16 */
} babe_unet_plan_desc;
/* copies the descriptor and every babe_unet_attn it points to (the weights stay the caller's).  NULL with a message naming the
 * field, before any launch: an attention branch with attn_core 0, a shape babe_attn_fwd refuses (F, num_buckets), a
 * num_buckets / max_distance pair babe_attn_bucket_thresholds refuses, a missing image, gamma or FiLM offset */
void* babe_unet_plan_create(const babe_unet_plan_desc* desc);
void babe_unet_plan_destroy(void* plan);
void* babe_unet_state_create(void);                                 /* one evaluation's bookkeeping; one per concurrent stream */
void babe_unet_state_destroy(void* state);
long babe_unet_workspace_bytes(const void* plan, int B, const int* T_oct);
int babe_unet_fwd(const void* plan, void* state, const float* const* C_in, const float* film, long film_bs, int B,
                  const int* T_oct, void* workspace, long workspace_bytes, float* const* outs, void* stream);
int babe_unet_vjp(const void* plan, void* state, const float* const* gouts, float* const* gC, void* stream);
/* The two forms of the layer path that babe_unet_fwd / babe_unet_vjp AND a host sequencing the same layers itself (babe_amd/
 * networks/unet_engine.py) act on, one value per process.  FUSE_GN_FWD: the next layer's GroupNorm sums come out of the forward
 * F(4,5) conv's epilogue (stat_mode 1; on unless BABE_FUSE_GN_FWD=0).  FUSE_GN: the GroupNorm-VJP partial sums come out of the
 * transposed F(4,5) conv's epilogue (stat_mode 2; off unless BABE_FUSE_GN is a non-zero number).  The environment is read once,
 * here and nowhere else; _set changes a form for every later call of either sequencer.  babe_unet_workspace_bytes does not depend
 * on them.  _get: 0 / 1, or -1 for a bad index. */
enum { BABE_FORM_FUSE_GN_FWD = 0, BABE_FORM_FUSE_GN = 1 };
int babe_unet_form_get(int which);
int babe_unet_form_set(int which, int on);

/* ---- the k = (1,1) ResnetBlocks (the init blocks 2 -> N and the output heads N -> 2, up_out / mid_out) forward as one fused pass
 * over the block's N-channel tensor (csrc/pw_block.hip): GroupNorm finalize, scale, GELU, the N x N layer on fp32 MFMA, gate,
 * residual and the block's 2-channel side convs in registers - z is read once where the layer-by-layer path moves 8 - 9 planes.
 * Views are (pointer, batch stride, channel stride) of [B][C][F][T] tensors with contiguous rows, as everywhere in this header.
 *   z     the GroupNorm input, N channels, dense: the head's block input; the init block's proj_in output (the caller runs
 *         that conv itself: z is what the VJP keeps)
 *   x     init: the block's 2-channel input; head: NULL
 *   out   head: 2 channels, out = RS2 res_conv(z) + RS2 proj_out(y); init: N channels, out = RS2 res_conv(x) + RS2 y, with
 *         y = RS2 gate H gelu(scale z) + RS2 z
 *   add   head, optional: out = RS2 (the block) + RS2 add, the decoder's running sum; may be `out` itself
 *   part, S      babe_gn_partial's sums of z (G = 8 groups, n = N / 8 * F * T, S splits)
 *   film, film_bs   the FiLM rows [B][J]; the block's own offsets (film_aff[0]) are applied here
 *   gate  [B][N] contiguous, film_gate[0]'s vector
 *   plan_splits  the precision of the network the block belongs to, as babe_packed_conv::splits of its (5,3) layers: 0 fp32.  In a
 *         bf16 / bf16x3 network the (1,1) blocks may hold fp32 images, but such a network keeps one GELU launch per layer
 *   stats [B][8][3], scale [B][N]: written bit for bit as babe_scale_gelu_fin writes them (the VJP reads them)
 * _supported is the ONE statement of which blocks take the pass, asked by both UNet sequencers: returns 0 (run the block layer by
 * layer), 1 (head) or 2 (init).  an fp32 network (plan_splits == 0) and fp32 images, one (1,1) layer, N % 32 == 0, 64 <= N <= 256, T % 4 == 0, 16-byte aligned views,
 * z dense, no frequency bias, no parameter gradients wanted (train == 0), and the process's switch on.
 * _enable sets that switch and returns its previous value; it starts from BABE_PW_BLOCK (0: off), read only by the library.
 * babe_unet_workspace_bytes does not depend on it. */
typedef struct {
    int B, F, T, S;
    int plan_splits;
    const float* z; long z_bs, z_cs;
    const float* x; long x_bs, x_cs;
    float* out; long out_bs, out_cs;
    const float* add; long add_bs, add_cs;
    const double* part;
    const float* film; long film_bs;
    const float* gate;
    float *stats, *scale;
} babe_pw_args;
int babe_pw_block_enable(int on);
int babe_pw_block_supported(const babe_unet_block* blk, const babe_pw_args* a, int train);
int babe_pw_block_fwd(const babe_unet_block* blk, const babe_pw_args* a, void* stream);

/* ---- strided copy / axpby: out = alpha*in + beta*out on [B][C][F][T] views (torch.cat / slicing /
 * (a+b)/sqrt2 residual merges, cqtdiff+.py:769-774,794,814-822) */
int babe_axpby4d(const float* in, long in_bs, long in_cs, float* out, long out_bs, long out_cs,
                 int B, int C, int F, int T, float alpha, float beta, void* stream);
/* out[b][c][:, :] = value on a [B][C][F][T] view */
int babe_fill4d(float* out, long out_bs, long out_cs, int B, int C, int F, int T, float value, void* stream);
/* out = alpha*x + beta*y in one pass (ResnetBlock's (x + h)/sqrt2 without res_conv, cqtdiff+.py:493); every view 16-byte aligned,
 * F*T % 4 == 0 */
int babe_axpby2_4d(const float* x, long x_bs, long x_cs, const float* y, long y_bs, long y_cs, float* out, long out_bs,
                   long out_cs, int B, int C, int F, int T, float alpha, float beta, void* stream);

/* ---- small dense: out[b][j] = act(sum_k x[b][k] W[j][k] + bias[j]); Linear :36-40, RFF_MLP :184-211 */
int babe_linear(const float* x, const float* W, const float* bias, float* out, int B, int K, int J,
                int relu, void* stream);
/* table = 2*pi*cnoise[b]*freq[j]; out[b] = [sin(table), cos(table)]  (:199-211) */
int babe_rff(const float* cnoise, const float* freq, float* out, int B, int R, void* stream);

/* ---- constant-Q transform (NSGT, mode "oct"): cqt_nsgt_pytorch.CQT_nsgt.fwd/.bwd/.apply_hpf_DC, call
 * sites networks/cqtdiff+.py:743,841 and testing/blind_bwe_sampler.py:156.  The length-L real DFT is a
 * four-step N1 x N2 transform whose two dense DFT stages run on babe_conv2d (1x1 convs with DFT matrices);
 * the entry points below are the remaining pieces.  Spectra are planar: spec[b][0][k] = Re, spec[b][1][k] = Im,
 * k = k1 + N1*k2 stored as [K2][N1] (natural order), KX = K2*N1 >= L/2+1. */
/* forward: in [B][2*N1][N2] (Re rows k1 then Im rows) -> out [B][2*N2][N1] = transpose(in * tw[k1][n2]);
 * adjoint=1: in [B][2*N2][N1] -> out [B][2*N1][N2] = transpose(in) * conj(tw). tw: [N1][N2] float2. */
/* Mixed-radix variant (csrc/fft_mixed.hip, round 4): the same four-step transform with both stages as Stockham FFTs of
 * length N1 / N2 in LDS (radices 2,3,4,5,7,11,13,23) - two launches per transform, no dense DFT matrices.  direction 0:
 * x_in [B][N1*N2] -> spec_out planar [B][2][K2*N1];  direction 1: the transpose, spec_in -> x_out (real part of the unnormalised
 * inverse DFT of the zero-padded half spectrum).  rad1 / rad2: radices whose product is N1 / N2 (at most 6 each); w1 / w2:
 * exp(-2 pi i j / N1|N2) as float2[N]; tw: [N1][N2] float2 exp(-2 pi i k1 n2 / L); work: [B][2][N1*N2] floats of scratch. */
int babe_rfft_mixed(const float* x_in, float* spec_out, const float* spec_in, float* x_out, float* work, int B, int N1,
                    int N2, int K2, const int* rad1, int nrad1, const int* rad2, int nrad2, const float* w1, const float* w2,
                    const float* tw, int direction, void* stream);
int babe_fft_twiddle_transpose(const float* in, float* out, const float* tw, int B, int N1, int N2,
                               int adjoint, void* stream);
typedef struct {
    int nbands; int L; int KX;
    const int* c;        /* [nbands] centre bin                               */
    const int* M;        /* [nbands] window length                            */
    const int* woff;     /* [nbands] offset of the band in the window tables  */
    const int* log2T;    /* [nbands] log2 of the band's coefficient count     */
    const int* oct;      /* [nbands] octave index (into coef[])               */
    const int* binoct;   /* [nbands] bin index inside the octave              */
    const float* tw4096; /* [2048] float2 exp(-2 pi i q/4096)                 */
    int nocts; int binsoct;
    float* coef[8];      /* per octave planar [B][2][binsoct][T_oct]          */
    /* workgroup table: workgroup w transforms bands wg_first[w] .. wg_first[w]+wg_count[w]-1, all of one octave
     * (same T), wg_count[w] * T <= 4096 points - or ONE band of T = 8192 points (a "long" workgroup, its own kernel).
     * Long bands are those of the HIGHEST octave only (an octave below has bands half as long): with max_log2T == 13 the last
     * binsoct bands of the table are the long ones and the last binsoct workgroups hold one of them each, in order; every
     * workgroup before them is a short one. */
    const int* wg_first; const int* wg_count; int nwg;
    /* the same tables packed for the kernel (one 16-byte load each instead of chains of dependent 4-byte loads - a
     * workgroup lives ~6 us and spent a third of that fetching its own description):
     * wg_rec[w] = {wg_first, wg_count, log2T, oct | binoct << 8},  band_rec[k] = {c, M, woff, 0}   (int4 each) */
    const int* wg_rec; const int* band_rec;
    int reserved;        /* must be 0 */
    /* host-side summary of the DEVICE tables above, validated by the entry points (the kernel keeps wg_count bands of
     * 3 ints in LDS and dispatches on log2T): max of wg_count (<= 64), min / max of log2T (2..13; 13 as described at the
     * workgroup table: then nwg >= binsoct and nbands >= binsoct, and a table of long bands alone - min_log2T == 13 - has
     * max_wg_count == 1 and nwg == nbands == binsoct) */
    int max_wg_count, min_log2T, max_log2T;
    long sum_T, sum_M;   /* sum over bands of T_k and M_k (for the measurement hook's algorithmic bytes) */
    double sum_TlogT;    /* sum over bands of T_k*log2(T_k) (algorithmic FFT flops = 5*that)            */
    /* Analytic Kaiser window (round 6): with win == NULL the band kernels evaluate the window g_k(m) / T_k themselves,
     * g_k(m) = I0(beta sqrt(a)) / I0(beta), a = 1 - (2 m / M_k)^2, as the polynomial sum_j kpoly[j] a^j, j <= kdeg
     * (kpoly[j] = (beta^2/4)^j / (j!)^2 / I0(beta): the power series of I0, truncated below 1e-9) - the table read was
     * 4 bytes per point and clip, 6 of the 45 us of the analysis launch at 32 clips.  kdeg = 0: not available (large
     * beta), the table has to be passed. */
    int kdeg; float kpoly[12];
} babe_cqt_bands;
/* analysis-type: coef_k = IFFT_T(fold(spec[(c_k+m) mod L] * win[woff_k+m']))  (win carries 1/T and any scale).
 * Used for CQT.fwd (win = g/T, or NULL: evaluated analytically, bands->kdeg > 0) and for the adjoint of CQT.bwd
 * (win = (2/L) T^2 gd). */
int babe_cqt_band_analysis(const babe_cqt_bands* bands, const float* spec, const float* win, int B, void* stream);
/* synthesis-type: bs[b][woff_k+m'] = FFT_T(coef_k)[m mod T] * win[woff_k+m']  (float2).
 * Used for CQT.bwd (win = T gd) and for the adjoint of CQT.fwd (win = g/T, or NULL: analytic). */
int babe_cqt_band_synthesis(const babe_cqt_bands* bands, float* bs, const float* win, long bs_stride, int B,
                            void* stream);
/* spec[b][:, n] = scale * sum over CSR entries of n of bs (conjugated when the entry's sign bit is set);
 * optionally multiplied by mul[n] (real, e.g. the DC/Nyquist high-pass) ; n > L/2 -> 0.
 * rec (optional, [L/2+1] int4): the same CSR as fixed records {src0, src1, src2, count}, count <= 3 for every bin; when
 * given, the record kernel runs (same sums in the same order), otherwise the CSR walk. */
int babe_cqt_gather(const float* bs, long bs_stride, const int* rowptr, const int* src, const int* rec, float* spec,
                    int KX, int L, float scale, const float* mul, int B, void* stream);
/* spec_out = spec_in * mul[n] * scale for n <= L/2, 0 above (apply_hpf_DC in the frequency domain);
 * optional second term: spec_out += spec2 * mul[n] * scale2. */
int babe_spec_scale(const float* spec_in, const float* spec2, float* spec_out, const float* mul, int KX, int L,
                    float scale, float scale2, int B, void* stream);

/* ---- the whole constant-Q transform from a plan handle (csrc/cqt_plan.hip, round 6): what a non-Python host binds instead of
 * cqt_nsgt_pytorch.CQT_nsgt(numocts, binsoct, mode="oct", window=("kaiser", beta), fs, audio_len) - constructed at
 * networks/cqtdiff+.py:620, .fwd :743, .bwd :841, .apply_hpf_DC testing/blind_bwe_sampler.py:156.  The band design (NSGT LogScale
 * grid, band lengths, Kaiser windows, painless-case dual frame incl. the mirrored bands, power-of-two rasterisation per octave,
 * the CSR of the overlap-add, the mixed-radix plan of the length-L real FFT) is computed by the library in float64 with the
 * arithmetic of babe_amd/cqt.py::design_bands (integer tables equal, float tables to a few ulp: tests/test_cqt_plan_cpu.py).
 *   design: host only, no GPU call.  babe_cqt_design_get copies table `name` (int64: M c T woff idx rowptr src; float64: f Om g
 *   gdual Tw hpf kpoly; int32: rad1 rad2 wg_first wg_count T_oct; one int64: nb nwin M_dc N1 N2 K2 KX kdeg) into out and returns
 *   its size in bytes (out = NULL: size only), -1 for an unknown name.
 *   plan: design + device tables (one allocation on the current device).  Coefficients are planar, one tensor per octave:
 *   coef[j] = [B][2][binsoct][T_oct[j]], j = 0 the LOWEST octave (the [B,2,64,T] tensors the UNet consumes).  ws: device scratch of
 *   babe_cqt_workspace_bytes(plan, B) bytes, owned by the caller (one per concurrent stream).  NULL / negative on failure
 *   (babe_last_error()).
 *   max_band (the _ex entries): the longest band transform the host is prepared for, 4096 or 8192 points (anything else: NULL).  A
 *   design whose longest band needs more is refused ("cqt design: ..." naming the limit); the top octave's bands have about
 *   0.01086 * audio_len samples whatever fs is, so 4096 reaches audio_len = 368368 (and not 384000) and 8192 about 754000.  The
 *   five-argument entries are the _ex entries with max_band = 4096: a host that sized its tables by that limit keeps it. */
void* babe_cqt_design_create(double fs, int audio_len, int numocts, int binsoct, double beta);
void* babe_cqt_design_create_ex(double fs, int audio_len, int numocts, int binsoct, double beta, int max_band);
void babe_cqt_design_destroy(void* design);
long babe_cqt_design_get(const void* design, const char* name, void* out, long capacity_bytes);
void* babe_cqt_plan_create(double fs, int audio_len, int numocts, int binsoct, double beta);
void* babe_cqt_plan_create_ex(double fs, int audio_len, int numocts, int binsoct, double beta, int max_band);
void babe_cqt_plan_destroy(void* plan);
const void* babe_cqt_plan_design(const void* plan);                  /* the plan's design (owned by the plan), for babe_cqt_design_get */
long babe_cqt_workspace_bytes(const void* plan, int B);
int babe_cqt_fwd(const void* plan, const float* x, float* const* coef, float* ws, int B, void* stream);            /* .fwd: x [B][L] -> coef */
int babe_cqt_bwd(const void* plan, float* const* coef, float* x, float* ws, int B, void* stream);                  /* .bwd: coef -> x [B][L] */
int babe_cqt_fwd_adjoint(const void* plan, float* const* gcoef, float* gx, float* ws, int B, void* stream);        /* (.fwd)^T, for the VJP */
int babe_cqt_bwd_adjoint(const void* plan, const float* gx, float* const* gcoef, float* ws, int B, void* stream);  /* (.bwd)^T, for the VJP */
int babe_cqt_hpf(const void* plan, const float* x, float* out, float* ws, int B, void* stream);                    /* .apply_hpf_DC (self-adjoint) */

/* ---- STFT-domain degradation model: utils/blind_bwe_utils.py:6-39 (apply_stft / apply_filter_istft /
 * apply_filter) and testing/blind_bwe_sampler.py:518-595.  nfft in {256..4096} (power of two), hop nfft/2,
 * periodic Hamming window, NFFT zeros appended, frames = 1 + L/hop.  spec: [B][frames][nfft/2+1] float2. */
/* spec = rfft(frame * w); if pre (length nfft+hop*(frames-1)) != NULL the signal is multiplied by pre[n] first
 * (1/envelope, used by the adjoint of the iSTFT normalisation). */
int babe_stft_fwd(const float* x, long x_bs, int L, const float* pre, float* spec, int B, int nfft, int frames,
                  const float* tw4096, void* stream);
/* frames_out[b][t][:] = w * irfft(spec[b][t] * H[b or 0][:]) ; H stride H_bs (0 = one filter for the batch) */
int babe_spec_filter_istft(const float* spec, const float* H, long H_bs, float* frames_out, int B, int nfft,
                           int frames, const float* tw4096, void* stream);
/* overlap-add of frames, times post[n] if given (1/envelope), cropped to L.
 * y == NULL: out = ola.   y != NULL: out = y - ola (the residual) and part[b][blk] = sum of squares (double). */
int babe_ola(const float* frames_in, const float* post, const float* y, long y_bs, float* out, long out_bs,
             double* part, int nblk, int B, int L, int nfft, int frames, void* stream);
/* out[b][n] = -r[b][n] / ||r_b|| * post[n]  (seed of the guidance VJP: d||y-Ax|| / d(pre-normalisation OLA)).
 * shared_norm=1 is NOT used for the norm (the reference's norm is per item, blind_bwe_sampler.py:117). */
int babe_residual_seed(const float* r, long r_bs, const double* part, int nblk, const float* post, float* out,
                       long out_bs, int B, int L, void* stream);
/* per-bin sufficient statistics of the magnitude fit: stats[b][0..2][k] (double) =
 * sum_t |X|^2, sum_t |X||Y|, sum_t |Y|^2.  shared=1 sums over the batch too (reference batch semantics). */
int babe_stft_mag_stats(const float* specX, const float* specY, double* stats, int B, int nbins, int frames,
                        int shared, void* stream);
/* design_filter (utils/blind_bwe_utils.py:82-119): params [P][2][K] (fc row, A row) -> H [P][nbins];
 * bin frequencies are float32(k) * float32(fs/nfft) and masks are evaluated in float32 like the reference. */
int babe_design_filter(const float* params, float* H, int P, int K, int nbins, float fs, int nfft, void* stream);
typedef struct {
    float mu_fc, mu_A, tol_fc, tol_A, fcmin, fcmax, Amin, Amax;
    int max_iter, clamp_fc, clamp_A, only_negative_A, weighting; /* 0 None, 1 sqrt, 2 linear, 3 log */
    int kernel;  /* 0: filter_fit_fast_kernel (register-resident, v_exp/v_log segments; default), 1: filter_fit_kernel, the first
                  * kernel, which keeps the reference's operation order inside an iteration; both are pinned against the same
                  * goldens, and against each other over full runs (tests/test_gpu_stft.py) */
} babe_fit_cfg;
/* BlindSampler.fit_params (:533-595): projected gradient descent on (fc, A) from the statistics.
 * params [P][2][K] updated in place; n_iter[P] receives the iteration count. K <= 8. */
int babe_filter_fit(const double* stats, float* params, int* n_iter, int P, int K, int nbins, float fs, int nfft,
                    const babe_fit_cfg* cfg, void* stream);
/* The objective of that fit and its gradient at given parameters, no descent step (BlindSampler.optimizer_func + autograd,
 * :523-533, as compute_sweep :598-616 evaluates them on a grid): lossgrad [P][1 + 2K] = loss, d loss / d fc_j, d loss / d A_j for
 * each of the P parameter sets params [P][2][K]; stats_pstride: doubles between the statistics of consecutive sets (3 * nbins for
 * one set each, 0 for ONE set of statistics shared by all P).  Reference-order kernel (cfg.kernel is ignored). */
int babe_filter_loss_grad(const double* stats, long stats_pstride, const float* params, float* lossgrad, int P, int K,
                          int nbins, float fs, int nfft, const babe_fit_cfg* cfg, void* stream);

/* ---- known FIR degradation (config #1): F.conv1d(y[B,1,L], taps[1,1,ntaps], padding="same"),
 * testing/edm_sampler.py:245-252, utils/bandwidth_extension.py:76-95.  PyTorch pads (ntaps-1)/2 on the left and the
 * rest on the right (even ntaps: 249 | 250) and does not flip the kernel: out[n] = sum_k taps[k] x[n+k-padl].
 * adjoint=1 computes the transpose (the input-VJP). */
int babe_fir_same(const float* x, long x_bs, const float* taps, int ntaps, float* out, long out_bs, int B, int L,
                  int adjoint, void* stream);

/* ---- A-weighted training loss (diff_params/edm.py:201-206: error = AW(estimate - target), then error**2; AW =
 * utils/training_utils.py FIRFilter :124-138, F.conv1d(padding=K/2), no tap flip): the FIR fused with the subtraction in front
 * of it and the square behind it, and its transpose fused with the square's derivative - one pass over HBM per direction.
 * K odd, 1 <= K <= 255 (anything else is refused before a launch); any B >= 1, L >= 1 (L < K included).  est_bs / tgt_bs / g_bs:
 * row strides in elements; ew, err2 and dest are dense [B][L].  Every output is written exactly once and every sum runs over the
 * taps in order, without atomics: results are bit-identical from run to run and on any stream. */
int babe_fir_sqerr_fwd(const float* est, long est_bs, const float* tgt, long tgt_bs, const float* taps, int K,
                       float* ew, float* err2, int B, int L, void* stream);
    /* ew[b][n] = sum_k taps[k] * (est - tgt)[b][n + k - K/2]   (zeros outside [0,L));   err2 = ew * ew            */
int babe_fir_sqerr_bwd(const float* g, long g_bs, const float* ew, const float* taps, int K,
                       float* dest, int B, int L, void* stream);
    /* h = 2 * g * ew;   dest[b][m] = sum_k taps[k] * h[b][m - k + K/2]   (the transpose of the forward FIR)       */

/* ---- frequency-resolved error of the training log (stands in for training/trainer.py:329-334, a librosa CQT on the CPU): mean
 * energy per CQT bin of planar coefficients, one workgroup per (b, f).  Any T >= 1; B, F or T <= 0 or a NULL pointer return
 * BABE_ERR_ARG before a launch.  fp32 sums in one fixed order (per thread, within the wave, across the waves through LDS) and no
 * atomics: bit-identical from run to run; relative error at most (ceil(T / 256) + 11) * 2^-24, every term being non-negative. */
int babe_plane_bin_energy(const float* c, float* out, int B, int F, int T, void* stream);
    /* c [B][2][F][T] planar (re, im), out[b][f] = (1/T) * sum_t (re^2 + im^2) */

/* ---- evaluation metric: log-spectral distance (LSD) of an estimate against a reference, this project's own definition (the
 * reference computes none; INTEGRATION.md "Evaluating a prior").  Full frames only, T = 1 + (L - nfft) / hop, no centring and no
 * padding; periodic Hann window; P = |rfft(w frame)|^2 (unnormalised), floored at floor_pow; d[t][k] = log10 Pref - log10 Pest;
 * frame_lsd[b][t] = sqrt(mean over k in [k_lo, k_hi) of d^2); clip_lsd[b] = mean over t of frame_lsd[b][t].
 * nfft a power of two in 256..4096, 1 <= hop <= nfft, L >= nfft, 0 <= k_lo < k_hi <= nfft/2 + 1, floor_pow > 0, 1 <= B <= 65535,
 * non-NULL pointers (clip_lsd may be NULL: the second launch is left out); anything else returns BABE_ERR_ARG before a launch.
 * ref_bs / est_bs: row strides in elements (the signals may live in different buffers, any 4-byte alignment); nothing outside
 * [0, L) of a row is read, nothing but the outputs is written.  One workgroup per (frame, clip), one complex FFT for both
 * signals, sums in one fixed order without atomics: bit-identical from run to run. */
long babe_lsd_num_frames(int L, int nfft, int hop);                       /* host only; -1 on bad arguments */
int babe_lsd_frames(const float* ref, long ref_bs, const float* est, long est_bs, int L, int B, int nfft, int hop,
                    int k_lo, int k_hi, float floor_pow, float* frame_lsd /* [B][T] */, float* clip_lsd /* [B], may be NULL */,
                    void* stream);

/* ---- sampler element-wise steps: testing/blind_bwe_sampler.py:503-516, :125-135, :701-761; edm.py:144-159 */
/* out = a*x + b*y + c*z (y, z optional) over n elements */
int babe_lincomb3(float* out, float a, const float* x, float b, const float* y, float c, const float* z, long n,
                  void* stream);
/* y[b] += sqrt(var(y[b]) / snr) * noise[b] in place, var = unbiased sample variance over the n samples of clip b; snr is the
 * LINEAR ratio 10^(SNR_observations / 10).  Replaces the observation-noise lines of get_rec_grads and fit_params
 * (testing/blind_bwe_sampler.py:80-86, :542-548; conf/tester/blind_bwe_2.yaml SNR_observations: 50). */
int babe_add_obs_noise(float* y, long y_bs, const float* noise, long noise_bs, float snr, int B, long n, void* stream);
/* out[b][i] = m[i]*a[b][i] + (1-m[i])*b_[b][i]; a or b_ may be NULL (= 0); mask stride mask_bs (0: shared).
 * Mask-mixed degradation and the replacement data-consistency step of predict_bwe_AR (blind_bwe_sampler.py:63-73,280-300) */
int babe_mask_blend(float* out, const float* mask, long mask_bs, const float* a, const float* b_, int B, long n,
                    void* stream);
/* part[b][blk] = sum of squares of g[b][blk-th slice] (double) */
int babe_sumsq_partial(const float* g, long g_bs, double* part, int nblk, int B, long n, void* stream);
/* STFT-domain guidance distances (get_rec_grads :105-115 -> utils/blind_bwe_utils.py:148-247; conf/tester/blind_bwe_2.yaml):
 * X = STFT(rec), R = STFT(y) as [B][frames][nbins] complex (babe_stft_fwd), w[nbins] = frequency weighting.  mode 0:
 * ||w (X - R)||_2, 1: ||w|X| - w|R|||_2, 2: ||log10(w|X| + 1e-8) - log10(w|R| + 1e-8)||_2.  babe_stft_dist_partial writes
 * partial sums of squares ([B][nblk] doubles), babe_stft_dist_grad G = dD/dX with ONE D over the batch (shared = 1, the
 * reference) or per item; d/d(rec) = STFT^T(G) = babe_ola(babe_spec_filter_istft(G, H = nfft * [1, 1/2, ..., 1/2, 1])).
 * babe_residual_seed_alt mode 3 multiplies such a ready gradient by the overlap-add normalisation. */
int babe_stft_dist_partial(const float* X, const float* R, const float* w, double* part, int nblk, int B, int nbins,
                           int frames, int mode, void* stream);
int babe_stft_dist_grad(const float* X, const float* R, const float* w, const double* part, int nblk, float* G, int B,
                        int nbins, int frames, int mode, int shared, void* stream);
/* Alternative guidance distances of get_rec_grads (testing/blind_bwe_sampler.py:99-103; conf/tester/blind_bwe_cossim.yaml):
 * seed = d(distance)/d(rec) [* post] from r = y - rec.  mode 1: smooth_l1_loss(y, rec, reduction='sum', beta):
 * -clamp(r / beta, -1, 1).  mode 2: clamp(1 - CosineSimilarity(rec, y), min 0) per batch item, with the three sums
 * (rec.rec, rec.y, y.y) from babe_cos_partial (part: [B][nblk][3] doubles).  mode 3: r is already the gradient: out = r * post. */
int babe_cos_partial(const float* r, long r_bs, const float* y, long y_bs, double* part, int nblk, int B, long n,
                     void* stream);
int babe_residual_seed_alt(const float* r, long r_bs, const float* y, long y_bs, const double* part, int nblk,
                           const float* post, float* out, long out_bs, int B, int L, int mode, float beta, void* stream);
/* mode 0 (blind_bwe_sampler.py:125-135,701): d = -t*((xden-xhat)/t^2 - s*g/t), s = xi/(||g||/sqrt(audio_len) + 1e-6)
 * mode 1 (edm_sampler.py:78-92):              d = -t*((xden-xhat)/t^2 - s*g),   s = xi/(||g||/sqrt(audio_len)*t + 1e-6)
 * shared_norm=1 uses the norm over the whole batch (reference semantics). */
int babe_score_direction(const float* xden, const float* xhat, const float* g, const double* part, int nblk,
                         float* d, float t, float xi, float audio_len, int shared_norm, int mode, int B, long n,
                         void* stream);

/* ---- one whole SCORE EVALUATION from plan handles (csrc/score_eval.hip, round 6): what BlindSampler.evaluate sequences from
 * Python (testing/blind_bwe_sampler.py:75-170, 503-595, 687-761; diff_params/edm.py:144-159), as one call for a non-Python host:
 * preconditioned denoiser (CQT.fwd -> UNet -> CQT.bwd) -> apply_hpf_DC -> STFT -> [filter fit] -> filter design -> residual
 * y - A(x_den) and the gradient of its norm through iSTFT o H o STFT, the high-pass and the network -> score direction.
 * Default configuration (L2 guidance norm, STFT-domain low-pass, no observation noise / FIR) and, with desc.mask, the AR
 * observation model over the known filter: residual y - (mask x_den + (1 - mask) A(x_den)), gradient mask s + A^T((1 - mask)
 * s_post), and with desc.dc_mask the replacement step on x0 = x - t d after the score direction.  Bit-identical to the Python
 * sequencer on both (tests/test_gpu_eval_c.py, tests/test_gpu_sample_ar_c.py).  specY may be NULL when blind = 0.  No allocation,
 * no synchronisation.
 * Known degradations (desc.obs_kind, below): FIR, IIR ('cheby1' / 'biquad'), mask (inpainting, compressed sensing) and clip
 * (declipping) take the place of the STFT filter - residual, block sums, seed and transpose as the degrade.py objects sequence
 * them -, the classic replacement step (desc.dc_classic) and the EDM sampler's no-guidance branch follow the score direction,
 * and y == NULL is unconditional sampling: d = (x - x_den) / t (STFT kind without mask only).  Bit-identical to the Python
 * sequencers BlindSampler.evaluate and edm_sampler.Sampler.evaluate (tests/test_gpu_obs_library.py).  Still with the Python
 * sequencer: 'resample' / 'decimate' and phase retrieval (the observation is not of the state's shape), the smooth-L1, cosine
 * and STFT-domain distances, observation noise, attention networks. */
typedef struct {
    const void* unet_plan; void* unet_state;      /* babe_unet_plan_create / babe_unet_state_create (one state per stream) */
    const void* cqt_plan;                         /* babe_cqt_plan_create for (fs, L) */
    int L;                                        /* exp.audio_len */
    /* noise embedding (RFF_MLP_Block cqtdiff+.py:184-211) and every FiLM Linear (:36-40) stacked into one matrix */
    const float* rff_freq; int rff_n;             /* embedding.RFF_freq [rff_n] */
    const float* emb_W[3]; const float* emb_b[3]; /* embedding.MLP.i weight [emb_dim[i+1]][emb_dim[i]], bias */
    int emb_dim[4];                               /* emb_dim[0] = 2 * rff_n */
    const float* film_W; const float* film_b; int film_J;   /* [film_J][emb_dim[3]]: affine / gate rows in the UNet plan's order */
    /* STFT-domain degradation model (utils/blind_bwe_utils.py): nfft, periodic-Hamming OLA envelope 1 / sum w^2
     * [nfft + hop (frames - 1)], exp(-2 pi i q / 4096) [2048] float2 */
    int nfft; float fs; const float* env_inv; const float* tw4096;
    int K;                                        /* break points of the piecewise filter (<= 8) */
    babe_fit_cfg fit;
    int blind;                                    /* 1: fit the filter parameters in this evaluation (predict_blind_bwe) */
    int shared;                                   /* 1: the reference's batch coupling (one filter, whole-batch norms); 0: per clip */
    int hpf;                                      /* tester.filter_out_cqt_DC_Nyq */
    float xi; int score_mode; float audio_len_norm;   /* babe_score_direction's xi, mode and audio_len */
    /* the observation model of predict_bwe_AR (blind_bwe_sampler.py:259-303), all NULL / 0 = off (babe_model_eval_desc sets that):
     * mask [L], or [B][L] at row stride mask_bs (0: one mask for every clip) - 1 where y is the known signal itself, 0 where it
     * is the filtered one; needs blind = 0.  dc_mask / dc_y (together, and only with mask; rows at the same stride): the
     * smoothed mask and dc_mask * y_masked of the replacement step x0 <- (1 - dc_mask) x0 + dc_y of inpaint_DC (:63-73). */
    const float* mask; long mask_bs;
    const float* dc_mask; const float* dc_y;
    /* the KNOWN observation model y = A(x) (babe_amd/degrade.py; all zero = BABE_OBS_STFT, the filter of `params`).  Every other
     * kind needs blind = 0 and reads neither params nor specY (both may be NULL); `mask` above combines with STFT and FIR only
     * (MaskMixDegradation over that filter: the observed part takes the plain seed).
     *   FIR:  taps [ntaps] (device): F.conv1d(padding="same"), babe_fir_same and its transpose.
     *   IIR:  b, a [order + 1] (device, float32, already divided by a[0]; babe_iir_check decides what degrade.prepare_iir decides),
     *         order 1..16; clamp = 1: lfilter's clamp to [-1, 1] ('biquad'), whose mask the transpose of the same call reads.
     *   MASK: A(x) = obs_mask x; obs_mask [L], or [B][L] at row stride obs_mask_bs (0: one row for every clip); self-adjoint.
     *   CLIP: A(x) = clip(x, -clip_value, clip_value), clip_value >= 0; the transpose multiplies by |x| <= clip_value.
     * dc_classic = 1 (STFT, FIR, IIR, MASK; not with dc_mask): after the score direction, the replacement step x0 <- y + x0 - A(x0)
     * on x0 = x - t d, then back to a direction (posterior_sampling.data_consistency; under `mask` A is the inner filter without
     * the mix, as in the Python sequencer).  With xi == 0 and score_mode == 1 it is the EDM sampler's no-guidance branch
     * (edm_sampler.Sampler.evaluate): the step on the denoised estimate itself, which then gets no high-pass. */
    int obs_kind;                                 /* BABE_OBS_* */
    const float* taps; int ntaps;
    const float* b; const float* a; int order; int clamp;
    const float* obs_mask; long obs_mask_bs;
    float clip_value;
    int dc_classic;
} babe_eval_desc;
enum { BABE_OBS_STFT = 0, BABE_OBS_FIR = 1, BABE_OBS_IIR = 2, BABE_OBS_MASK = 3, BABE_OBS_CLIP = 4 };
long babe_eval_workspace_bytes(const babe_eval_desc* desc, int B);
int babe_score_eval(const babe_eval_desc* desc, const float* x, float t, float cskip, float cout, float cin, float cnoise,
                    const float* y, const float* specY, float* params, float* d, float* x_den, int* n_iter, void* ws,
                    long ws_bytes, int B, void* stream);
int babe_fill(float* out, float v, int n, void* stream);            /* out[0..n) = v (the [B][1] cnoise input of the embedding) */

/* ---- counter-based Gaussian noise (csrc/randn.hip): Philox4x32-10 with the Random123 constants (multipliers 0xD2511F53,
 * 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; 10 rounds).  Element i of clip c, draw k, under seed s has ONE definition,
 * whatever the grid, the block size or the batch it is produced in:
 *   counter = (q & 0xffffffff, q >> 32, c, k) with q = i / 4;  key = (s & 0xffffffff, s >> 32);  output word i % 4
 *   u1 = ((r >> 9) + 0.5) * 2^-23 in (0, 1),  u2 = (r' >> 9) * 2^-23   (both exact in float32; r, r' = words (0,1) and (2,3))
 *   z  = sqrt(-2 ln u1) * (cospi(2 u2), sinpi(2 u2))                     (Box-Muller; |z| <= 5.78)
 * with logf / sqrtf / sincospif (not the fast intrinsics).  out rows may start at any 4-byte boundary (16-byte stores where a
 * row starts on a 16-byte one); out_bs >= n for B > 1; 1 <= B <= 65535; 0 <= clip0, clip0 + B <= 2^32; 0 <= draw < 2^32;
 * anything else returns BABE_ERR_ARG before a launch. */
/* host, no GPU: out[4] = philox4x32-10(ctr[4], key[2]) - the definition the kernel implements */
int babe_philox4x32(const int* ctr, const int* key, int* out);
/* out[b][i] (row stride out_bs) = draw `draw` of clip clip0 + b under `seed`, i in [0, n) */
int babe_randn(float* out, long out_bs, int B, long n, long seed, long clip0, long draw, void* stream);
/* the raw 32-bit words behind the same elements (tests pin these bit for bit) */
int babe_rand_bits(int* out, long out_bs, int B, long n, long seed, long clip0, long draw, void* stream);

/* ---- one whole SAMPLING RUN from plan handles (csrc/sample.hip): what BlindSampler._sample -> step -> _heun_first /
 * _heun_second sequence from Python (testing/blind_bwe_sampler.py:619-769, :509-516), as one call for a non-Python host:
 * specY = babe_stft_fwd(y) -> initial state -> per step: noise injection babe_lincomb3(1, x, inject, eps), babe_score_eval at
 * t_hat, then the Euler update x_hat + h d or the Heun pair (x' = x_hat + h d, babe_score_eval at t_next, x_hat + h/2 d + h/2 d').
 * Scope: exactly babe_score_eval's (blind or known fc_A filter, L2 guidance, the AR mask and its replacement step through
 * eval.mask / eval.dc_mask, the known degradations of eval.obs_kind, y == NULL for unconditional sampling; no observation noise,
 * no network with attention).  Like babe_score_eval the run contains no schedule formula: the
 * caller passes one row per step (babe_edm_steps fills them for a host without the Python EDM class).  Same kernels, order and
 * scalars as the Python loop: bit-identical to it (tests/test_gpu_sample_c.py).  No allocation, no synchronisation; a failing
 * inner call returns its code; every argument is checked on the host before the first launch.  Two runs on two streams, each
 * with its own unet_state and workspace over one plan, are legal.  Lanes are the caller's: two runs, two calls. */
typedef struct {
    float t_hat;              /* t_i + gamma_i t_i: noise level of the first evaluation                         */
    float inject;             /* sqrt(t_hat^2 - t_i^2) * Snoise:  x_hat = x + inject * eps_i                    */
    float t_next, h;          /* h = t_next - t_hat                                                             */
    int   heun;               /* 1: second evaluation at t_next + trapezoidal update; 0: Euler (t_next == 0 or order 1) */
    float c1[4], c2[4];       /* cskip, cout, cin, cnoise at t_hat / at t_next                                  */
} babe_sample_step;
typedef struct {
    babe_eval_desc eval;      /* as for babe_score_eval; K and blind are read from here                        */
    int T; const babe_sample_step* steps;   /* host memory, T rows                                             */
    float t0; int warm_start; /* x_0 = (warm_start ? y : 0) + t0 * eps_init                                    */
    int skip_zero_inject;     /* 1: a step whose inject == 0 evaluates the state as it is, no draw and no injection launch (the EDM
                                 sampler's rule for gamma == 0, edm_sampler.py:187-198).  Row i + 1 of `noise` and draw i + 1 of
                                 the generator still belong to step i: a skipped step shifts nothing                             */
} babe_sample_desc;
long babe_sample_workspace_bytes(const babe_sample_desc* d, int B);
/* y [B][L] observations; params [P][2][K] (P = B, or 1 with eval.shared): in the initial filter parameters, out the final ones
 * (updated in place on the device by every evaluation when eval.blind); x_out [B][L] the restored signal (it carries the state
 * during the run).  noise [T+1][B][L]: draw 0 is the initial state, draw i + 1 step i; NULL: the draws come from
 * babe_randn(seed, clip0, draw) into one workspace buffer, so that the run is a function of (weights, y, seed) alone.
 * rec_x_den [T][B][L] / rec_params [T][P][2][K] (each may be NULL): the FIRST evaluation's denoised estimate of every step and the
 * parameters after it - what predict_blind_bwe(rid=True) keeps -, copied device to device on the stream.
 * y == NULL (needs warm_start = 0, the STFT kind and no mask): unconditional sampling.  params may be NULL where no evaluation
 * reads it: a kind other than BABE_OBS_STFT, or y == NULL (rec_params must then be NULL too). */
int babe_sample_bwe(const babe_sample_desc* d, const float* y, float* params, float* x_out, const float* noise, long seed, long clip0,
                    float* rec_x_den, float* rec_params, void* ws, long ws_bytes, int B, void* stream);
/* host helper for hosts without the Python EDM class: fills steps[T] and *t0 from the tester's diff_params in double arithmetic
 * (diff_params/edm.py:38-75, :108-139): t_i = (s0^(1/ro) + i/(T-1) (sigma_min^(1/ro) - s0^(1/ro)))^ro, t_T = 0, s0 = start_sigma
 * (<= 0: sigma_max); gamma_i = min(Schurn/(T+1), sqrt 2 - 1) where Stmin < t_i < Stmax.  T >= 2, order 1 or 2.  Snoise scales the
 * injected noise (predict_blind_bwe injects with 1, predict_bwe with diff_params.Snoise: pass what the run you mirror uses).
 * The Python class evaluates the same formulas in float32, so its rows differ in the last bits ((ro + 4) 2^-23 relative). */
int babe_edm_steps(babe_sample_step* steps, float* t0, int T, int order, double sigma_min, double sigma_max, double ro,
                   double sigma_data, double Schurn, double Stmin, double Stmax, double Snoise, double start_sigma);
/* host helpers for hosts without scipy (no GPU call; csrc/sample.hip).
 * babe_firwin_kaiser: scipy.signal.firwin(numtaps, cutoff, width=width, window="kaiser", fs=fs[, pass_zero="highpass"]) in double -
 * what the reference's get_FIR_lowpass / get_FIR_high_pass compute with the config's "beta" as the width
 * (utils/bandwidth_extension.py): attenuation a = 2.285 (numtaps - 1) pi width / (fs / 2) + 7.95, Kaiser beta from a
 * (0.1102 (a - 8.7) above 50 dB, 0.5842 (a - 21)^0.4 + 0.07886 (a - 21) above 21 dB, else 0), h[n] = w[n] (r sinc(r m) - l sinc(l m))
 * over the band [l, r] = [0, c] or [c, 1], c = cutoff / (fs / 2), m = n - (numtaps - 1) / 2, scaled to unit gain at the band's
 * centre frequency (0, or 1 for the high-pass).  taps_out [numtaps] doubles (host).  Refused: numtaps < 1, cutoff outside
 * (0, fs / 2), width <= 0, an even numtaps for the high-pass. */
int babe_firwin_kaiser(int numtaps, double cutoff, double width, double fs, int highpass, double* taps_out);
/* babe_iir_check: 0 where degrade.prepare_iir accepts (b, a) [order + 1] (host, float32, after the division by a[0]): order in
 * 1..16, a[0] == 1, and every root of a inside the unit circle - the step-down (Schur-Cohn) recursion in double on the float32
 * coefficients: all reflection coefficients below 1 in modulus.  Anything else returns BABE_ERR_ARG with the reason. */
int babe_iir_check(const float* b, const float* a, int order);

/* ---- one WHOLE RECORDING from plan handles (csrc/recording.hip): what long_file.restore_recording_complete (without denoiser and
 * rate conversion: babe_restore_file below puts them in front) and restore_file_AR sequence from Python (BlindTester.test_real_blind_bwe_complete, testing/
 * blind_bwe_tester.py:710-867), as one call for a non-Python host: normalise the file to target_std, estimate the low-pass filter
 * blind on n_blind segments in one coupled batch (babe_sample_bwe with blind = 1, shared = 1), restore the first segment with that
 * filter, out-paint every following segment from the last `overlap` samples of the previous result (babe_sample_bwe with
 * eval.mask / eval.dc_mask), undo the normalisation.  Bit-identical to the Python flow on the same noise numbering
 * (tests/test_gpu_recording_c.py).  Tables and schedules come from the caller, the library holds no random policy: the host
 * picks the blind segments. */
/* the walk of restore_file_AR, host only: segment j starts at j (segL - overlap - discard_end); the last one is the first whose
 * start is not below Lrec - segL - discard_end and has Lrec - start samples (truncated to segL where that is more; always more
 * than overlap); a file of at most segL samples is one segment.  Fills starts / n_valid (each may be NULL) up to max_segments
 * entries and returns the number of segments, -1 unless 1 <= overlap < segL - discard_end and Lrec >= 1. */
long babe_recording_plan(long Lrec, long segL, long overlap, long discard_end, long* starts, long* n_valid, long max_segments);
typedef struct {
    babe_eval_desc eval;                  /* as for babe_score_eval (segL = eval.L); blind and the mask fields are set by the call;
                                             obs_kind must be BABE_OBS_STFT and dc_classic 0: the flow estimates its filter;
                                             eval.shared is that of the known-filter runs, the blind batch is always coupled */
    int T; float t0; int warm_start;      /* as in babe_sample_desc, for both tables */
    const babe_sample_step* steps_blind;  /* host, T rows: the blind loop injects with Snoise = 1 ...                        */
    const babe_sample_step* steps_known;  /* ... the known-filter loops with the tester's Snoise                              */
    int n_blind; long blind_starts[16];   /* 1..16 segments of the blind step, first samples in [0, max(Lrec - segL, 0)]    */
    const float* init_params;             /* device [2][K]: initial conditions of the filter fit                             */
    float target_std;                     /* complete_recording.std                                                          */
    long overlap, discard_end;            /* samples: known head of an AR segment; tail of a prediction that is not kept     */
    int inpaint_dc, dc_size;              /* complete_recording.inpaint_DC: the replacement step with a mask smoothed over   */
    const float* dc_window;               /* dc_size samples; device [2 dc_size]: the periodic Hann window of that length    */
    const float* std_dev;                 /* device [1]: the file's standard deviation, or NULL: computed by the call        */
} babe_recording_desc;
long babe_recording_workspace_bytes(const babe_recording_desc* d);         /* (does not depend on the file's length) */
/* rec [Lrec] the degraded file at the model's rate; out [Lrec] the restored file (zero past the last written sample: only a
 * last segment longer than segL leaves such a tail); filter_out [2][K] the estimated filter and blind_pred [n_blind][segL] the
 * blind step's restorations, in normalised units (each may be NULL).  Noise comes from babe_randn under `seed`: blind row b
 * draws as clip clip0 + b, segment j of the walk as clip clip0 + n_blind + j.  Normalisation: (target_std x) / s on the way in,
 * x (s (1 / target_std)) on the way out, s and the products read from device memory by the kernels.  Every argument is checked
 * on the host before the first device call; no allocation, no synchronisation, no host copy: all of it is enqueued on stream. */
int babe_restore_recording(const babe_recording_desc* d, const float* rec, long Lrec, float* out, float* filter_out,
                           float* blind_pred, long seed, long clip0, void* ws, long ws_bytes, void* stream);
/* the driver's own kernels as entries (tests pin them one by one):
 * out[b] = unbiased standard deviation of x[b][0..n) (row stride x_bs), n >= 2: double sums of x - x[b][0] and its square over 64
 * slices in a fixed order (part: [B][128] doubles of the caller), one rounding of the square root to float */
int babe_row_std(const float* x, long x_bs, int B, long n, float* out, double* part, void* stream);
/* dst[i] = i < n ? src[i] : 0 for i in [0, len), n <= len: a segment with a zero tail, or (n = len) a kept piece into the file */
int babe_segment_cut(const float* src, long n, float* dst, long len, void* stream);
/* by a scalar in device memory: mode 0: out = (a x) / s[0];  mode 1: out = x (s[0] a).  out may be x. */
int babe_scale_dev(float* out, const float* x, long n, float a, const float* s_dev, int mode, void* stream);
/* the masks of an edge at sample e, size <= e <= L: mask[i] = i < e; smooth[i] = 1 before e - size, window[size + i - (e - size)]
 * on [e - size, e), 0 from e on - BlindSampler.prepare_smooth_mask of that mask (:232-257).  smooth may be NULL. */
int babe_edge_masks(float* mask, float* smooth, long L, long e, int size, const float* window, void* stream);

/* ---- Denoiser pre-pass: networks/denoiser.py:232-321 (MultiStage_denoise, inference only) and
 * testing/denoise_and_bwe_tester.py:146-165 (STFT 1024/256 -> network -> inverse STFT).  csrc/denoiser.hip --------- */
/* General small-kernel Conv2d on [B][C][H][W] tensors with contiguous rows (replaces nn.Conv2d with
 * padding_mode='reflect' denoiser.py:40-46, the 4x4 stride-2 down conv :358-363 and, as four 2x2 parity kernels, the
 * ConvTranspose2d :383-388):  v = conv(in)[co][oh][ow] + bias[co];  act=1: v = ELU(v);  res: v += res[...];
 * out[b][co][oh*out_hstep + out_h0][ow*out_wstep + out_w0] = v  where that index lies inside [out_H][out_W]
 * (res is indexed like out).  Input index = o*stride - pad + k, reflected (pad_mode 1) or zero (0) outside. */
typedef struct {
    const float* in; long in_bs, in_cs; int IH, IW;
    const float* bias;           /* [Cout] or NULL */
    float* out; long out_bs, out_cs; int out_H, out_W, out_hstep, out_h0, out_wstep, out_w0;
    const float* res; long res_bs, res_cs;
    int B, Cin, Cout, OH, OW, KH, KW, stride, pad_t, pad_l, pad_mode, act;
    int ksplit;                  /* > 1: split the input channels over ksplit workgroups per tile (small planes); the */
    float* ws;                   /* partial sums go through ws [ksplit][B][Cout][OH][OW] and a finishing pass */
} babe_dnconv_args;
int babe_dn_conv2d(const babe_dnconv_args* a, const float* w_packed, void* stream);
/* mode 0: w [Cout][Cin][KH][KW] -> [KH][KW][ceil32(Cin)][ceil64(Cout)].  mode 1 (KH=KW=2): parity (ph,pw) of a
 * ConvTranspose2d weight [Cin][Cout][4][4] with stride 2: out[2m+p] = sum_a in[m-a] w[p+2a]. */
int babe_dn_pack_weights(const float* w, float* dst, int Cout, int Cin, int KH, int KW, int mode, int ph, int pw,
                         void* stream);
long babe_dn_packed_size(int Cout, int Cin, int KH, int KW);
/* out[b][c][h][w] += low[b][c][(h+dh)>>1][(w+dw)>>1]: nn.Upsample(2,'nearest') + CropAdd/CropConcat, denoiser.py:400-407 */
int babe_dn_upsample_add(float* out, long out_bs, long out_cs, const float* low, long low_bs, long low_cs, int B, int C,
                         int H, int W, int LH, int LW, int dh, int dw, void* stream);
/* out = x1 * sigmoid(m) + feats (SAM, denoiser.py:126-130); x1, m contiguous [B][C][hw] */
int babe_dn_sam_gate(const float* x1, const float* m, const float* feats, long f_bs, long f_cs, float* out, long out_bs,
                     long out_cs, int B, int C, long hw, void* stream);
/* out[B][2+nemb][T][F] = cat(X[B][2][T][F], femb[F][nemb] broadcast over b, t)  (AddFreqEncoding :159-169) */
int babe_dn_fill_input(const float* X, const float* femb, float* out, int B, int T, int F, int nemb, void* stream);
/* torch.stft(x, nfft, hop, hamming_window(nfft), center=False) as X[B][2][frames][nfft/2+1]; frames = 1+(L-nfft)/hop */
int babe_dn_stft(const float* x, long x_bs, int L, float* X, int B, int nfft, int hop, int frames, const float* tw4096,
                 void* stream);
/* torch.istft(P, nfft, hop, hamming_window(nfft), center=False)[..., :Lout]; frames_ws: [B][frames][nfft] scratch */
int babe_dn_istft(const float* P, float* frames_ws, float* y, long y_bs, int Lout, int B, int nfft, int hop, int frames,
                  const float* tw4096, void* stream);


/* ---- time attention of the CQTDiff+ ResnetBlock (csrc/attention.hip), fp32 MFMA.  Per batch item b and head h (H heads of F
 * features, F a multiple of 64 up to 448, any T >= 1), all tensors dense fp32 with T contiguous:
 *   qk  [B][2HF][T]  Conv1d output: Q = rows h*2F + f, K = rows h*2F + F + f;  qk_bias [2HF] added to both, or NULL
 *   a   [B][H][F][T] values V;  out [B][H][F][T];  lse [B][H][T] (log-sum-exp of each query's scores, for the VJP)
 *   S[n][m] = (Q[:,n].K[:,m] + emb[bucket[m - n + T - 1]][h]) * scale;  out[:,n] = sum_m softmax_m(S[n]) V[:,m]
 * bucket [2T-1] (babe_attn_buckets) and emb [num_buckets][H] (at most 64 buckets): both NULL without the relative bias. */
int babe_attn_buckets(int* out, int T, int num_buckets, int max_distance);   /* host function: T5 bidirectional buckets */
/* The same table written on the device, for a sequencer that may neither allocate nor copy (csrc/unet_engine.hip).  The bucket of
 * an offset d is non-decreasing in |d| and constant from max_distance on, so half - 1 thresholds describe it (half =
 * num_buckets / 2): thr[k - 1] = the smallest |d| whose bucket within its half is >= k.  babe_attn_bucket_thresholds is a host
 * function that derives them from babe_attn_buckets itself (no logarithm is evaluated anywhere else) and refuses what the table
 * kernel cannot take: num_buckets odd or outside 4..64, max_distance outside num_buckets / 4 + 1 .. 65536, a table that is not
 * monotone or does not reach its last bucket at max_distance.  babe_attn_bucket_table writes out[0 .. 2T-2] (device, int32) =
 * babe_attn_buckets(T, num_buckets, max_distance) entry for entry; the thresholds travel by value as the kernel's argument. */
typedef struct { int half, max_distance; int thr[32]; } babe_attn_bucket_thr;
int babe_attn_bucket_thresholds(babe_attn_bucket_thr* out, int num_buckets, int max_distance);
int babe_attn_bucket_table(const babe_attn_bucket_thr* thr, int T, int* out, void* stream);
int babe_attn_fwd(const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb, int num_buckets,
                  float* out, float* lse, int B, int H, int F, int T, float scale, void* stream);
/* input-VJP of babe_attn_fwd for the gradient dout of out: dqk [B][2HF][T] (dQ and dK, the gradients w.r.t. the qk rows) and
 * dv [B][H][F][T] (w.r.t. a through V), every element written once (no atomics: deterministic); D [B][H][T] is scratch. */
int babe_attn_vjp(const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb, int num_buckets,
                  const float* out, const float* lse, const float* dout, float* D, float* dqk, float* dv, int B, int H, int F,
                  int T, float scale, void* stream);
/* The same two passes on the bf16 MFMA pipe (csrc/attention_bf16.hip): same tensors (fp32 in HBM), same contract and refusals.
 * Q + bias, K + bias, V and dO are rounded once to bf16 (to nearest even) on their way into LDS, P and dS in registers as the
 * operand of the second product; accumulators, the relative bias, the online maximum and sum, lse and D stay fp32.  Four waves
 * per 32-row tile, the other side staged through LDS; every output element is written once (deterministic).  All pointers
 * 4-byte aligned.  babe_attn_vjp_bf16 takes the lse babe_attn_fwd_bf16 wrote. */
int babe_attn_fwd_bf16(const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb, int num_buckets,
                       float* out, float* lse, int B, int H, int F, int T, float scale, void* stream);
int babe_attn_vjp_bf16(const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb, int num_buckets,
                       const float* out, const float* lse, const float* dout, float* D, float* dqk, float* dv, int B, int H, int F,
                       int T, float scale, void* stream);


/* ---- training: parameter gradients of the CQTDiff+ UNet (csrc/wgrad.hip), fp32 (the conv weight gradient also with bf16
 * operands: babe_conv_wgrad_bf16_rows), no float atomics (every result is a
 * fixed-order sum: bit-identical run to run and independent of how batch rows are split between calls).
 *
 * Conv weight gradient (autograd's convolution_backward w.r.t. the weight of Conv2d "same", no bias):
 *   P_b[co][ci][kh][kw] = sum_{f,t} g[b][co][f][t] * X[b][ci][f + dil*(kh - KH/2)][t + kw - KW/2]   (zero outside [0,F) x [0,T))
 * X channels [0,cin_split) come from x, [cin_split,Cin) from x2 (the conv's two-source input); x, x2 and g are [B][C][F][T]
 * views with T contiguous and row stride T (batch / channel strides given: frequency sub-views need no copy).
 * KH x KW is 5x3 or 1x1; Cin, Cout <= 512; dil >= 1; any F, T. */
typedef struct {
    const float* x;  long x_bs,  x_cs;
    const float* x2; long x2_bs, x2_cs; int cin_split;      /* x2 NULL: single source (cin_split ignored) */
    const float* g;  long g_bs,  g_cs;
    int B, Cin, Cout, F, T, KH, KW, dil;
} babe_wgrad_args;
/* Workspace of babe_conv_wgrad_rows in floats (B * chunks * Cout * Cin * KH * KW, chunks a function of the shape only). */
long babe_conv_wgrad_workspace(const babe_wgrad_args* a);
/* rows[b*rows_bs + (co*Cin + ci)*KH*KW + kh*KW + kw] = alpha * oscale[b*Cout + co] * P_b[co][ci][kh][kw]   (oscale NULL: 1)
 * dgate (optional) [b*dgate_bs + co] = galpha * sum_k w[co][k] * P_b[co][k], w the conv's weights [Cout][Cin][KH][KW]: the FiLM
 * gate gradient of znew = rs2*(gate*conv(a) + z) without recomputing the conv (galpha = rs2 * upstream scale). */
int babe_conv_wgrad_rows(const babe_wgrad_args* a, float* ws, const float* oscale, float alpha, const float* w, float* dgate,
                         long dgate_bs, float galpha, float* rows, long rows_bs, void* stream);
/* The same weight gradient with bf16 operands (mixed-precision training; v_mfma_f32_32x32x16_bf16).  Arguments, shapes taken,
 * workspace layout and chunk count (a function of the shape only, not of B) are those of the fp32 pair; -1: shape not taken.
 * Arithmetic: g and X are read as fp32 and each rounded ONCE to bf16, round to nearest even (v_cvt_pk_bf16_f32), on the way into
 * LDS; the products of two bf16 values are exact in fp32 (8 x 8 significand bits); sums run in the MFMA's fp32 accumulators; the
 * chunks' partial tiles are fp32 in ws and are added in a fixed order by the fp32 entry's own tail, so oscale, alpha and the gate
 * dot galpha * <w, P_b> (w fp32, double sum) are exactly the fp32 entry's.  No float atomics: bit-identical run to run, and row b
 * does not depend on the other rows of the call.  Outside [0,F) x [0,T) of the VIEW the sum is zero (a sub-view's neighbouring
 * rows in memory are never read).  Rows that are 16-byte aligned (T % 4 == 0, aligned bases and strides) are staged with
 * 16-byte loads; anything else takes an element-wise path with the same arithmetic. */
long babe_conv_wgrad_bf16_workspace(const babe_wgrad_args* a);
int  babe_conv_wgrad_bf16_rows(const babe_wgrad_args* a, float* ws, const float* oscale, float alpha, const float* w,
                               float* dgate, long dgate_bs, float galpha, float* rows, long rows_bs, void* stream);
/* out[i] = beta*out[i] + sum_{b=0..B-1} rows[b*rows_bs + i], b in increasing order, i < n. */
int babe_rows_sum(const float* rows, long rows_bs, int B, long n, float* out, float beta, void* stream);
/* Per-channel GroupNorm * FiLM parameter gradient of a = gelu(z * scale), scale[b][c] = gamma[c]*(film_aff[b][c]+1)*r[b][g],
 * r = stats[(b*G+g)*3+2] (babe_gn_finalize), given da = dL/da (dense [B][C][hw]):
 *   dscale[b][c] = cs * sum_i da*gelu'(z*scale)*z    (double partial sums, fixed order)
 *   dgamma_rows[b*dg_bs + c] = dscale * (film_aff[b*film_bs + c] + 1) * r;   dfilm[b*dfilm_bs + c] = dscale * gamma[c] * r */
int babe_gn_param_grad(const float* z, const float* da, const float* scale, const float* stats, const float* gamma,
                       const float* film_aff, long film_bs, float cs, float* dgamma_rows, long dg_bs, float* dfilm,
                       long dfilm_bs, int B, int C, int G, long hw, void* stream);
/* Backward of babe_linear (y = x W^T + bias, optionally ReLU): dp = dy * (y > 0) (y NULL: no mask),
 *   dW[j][k] = beta*dW + sum_b dp[b][j] x[b][k];  db[j] = beta*db + sum_b dp[b][j];  dx[b][k] = sum_j dp[b][j] W[j][k] (dx may be NULL)
 * ws: babe_linear_bwd_workspace(B, K, J) floats. */
long babe_linear_bwd_workspace(int B, int K, int J);
int babe_linear_bwd(const float* dy, const float* y, const float* x, const float* W, float* dW, float* db, float* dx, float* ws,
                    int B, int K, int J, float beta, void* stream);


/* ---- frequency encodings of the UNet's init blocks (AddFreqEncodingRFF, cqtdiff+.py:213-263) folded into a bias (csrc/fenc.hip).
 * emb [64][64] = embeddings[j][f] (64 encoding channels x 64 bins of an octave); w [Cout][ld_w] the (1,1) conv weight over
 * cat(signal 2, encodings 64) channels (ld_w >= 66).
 *   fb[co*64 + f] = sum_{j<64} w[co*ld_w + 2 + j] * emb[j*64 + f], j ascending (one fused multiply-add chain per entry) */
int babe_fenc_bias(const float* w, const float* emb, float* fb, int Cout, int ld_w, void* stream);
/* The encoding columns of that conv's per-row weight gradient, for the output gradient alpha * g (g [B][Cout][F][T] view, rows
 * contiguous; F must be 64, anything else is an error):  rows[b*rows_bs + co*ld_row + 2 + j] = alpha * sum_f emb[j*64 + f] * (sum_t g[b][co][f][t]).
 * Fixed-order sums in double, no atomics; every (b, co) is written by one workgroup, so batch rows are independent. */
int babe_fenc_wgrad_rows(const float* g, long g_bs, long g_cs, const float* emb, float alpha, float* rows, long rows_bs, int ld_row,
                         int B, int Cout, int F, int T, void* stream);


/* ---- training: parameter gradients of the time-attention branch (csrc/attention_train.hip), fp32, fixed-order sums, no float
 * atomics.  Tensors as for babe_attn_fwd / babe_attn_vjp.
 *
 * qk Conv1d weight gradient, summed over the batch:
 *   dW[co*HF + ci] = alpha * sum_b sum_t dqk[b][co][t] * a1[b][ci][t] + beta * dW[co*HF + ci]     (beta == 0: dW is not read)
 * dqk [B][2HF][T], a1 [B][HF][T] dense, HF a multiple of 512 up to 3584, any T >= 1 (rows need no alignment).  K = (b, t) is
 * walked in ascending order; small HF splits it into chunks that a second pass adds in order (chunk count a function of
 * (B, HF, T) only).  ws: babe_attn_qk_wgrad_workspace floats (0: none needed; -1: unsupported shape). */
long babe_attn_qk_wgrad_workspace(int B, int HF, int T);
int babe_attn_qk_wgrad(const float* dqk, const float* a1, float* dW, float* ws, int B, int HF, int T, float alpha, float beta,
                       void* stream);
/* Per batch row, from the inputs of babe_attn_vjp (dS = P o (dP - D) recomputed; dqk is babe_attn_vjp's output):
 *   demb_rows[b*demb_bs + k*H + h] = sum_{n,m : bucket[m - n + T - 1] = k} scale * dS[b][h][n][m]   every k < num_buckets written,
 *                                    exactly 0 where no pair reaches the bucket        (NULL with bucket and emb NULL)
 *   dqkb_rows[b*dqkb_bs + r]       = sum_t dqk[b][r][t], r < 2HF                                    (NULL: not computed)
 * ws: babe_attn_param_vjp_workspace floats.  The wave's diagonals live in LDS next to its 16 query columns: 4*(32 F + T) bytes
 * plus 1.5 KB must fit in 64 KB (F = 448: T <= 1300; F = 64: any T up to 15000), anything larger is an argument error. */
long babe_attn_param_vjp_workspace(int B, int H, int T, int num_buckets);
int babe_attn_param_vjp(const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb,
                        int num_buckets, const float* out, const float* lse, const float* dout, const float* dqk, float* ws,
                        float* demb_rows, long demb_bs, float* dqkb_rows, long dqkb_bs, int B, int H, int F, int T, float scale,
                        void* stream);
/* The two calls above for a network whose attention core is babe_attn_fwd_bf16 / babe_attn_vjp_bf16 (mixed-precision training;
 * csrc/attention_bf16.hip, csrc/attention_train.hip).  Same arguments, layouts, fixed summation orders and refusals.
 *
 * babe_attn_param_vjp_bf16: out / lse / dout / dqk are those of the bf16 core.  The table gradient is a fourth mode of the
 * babe_attn_vjp_bf16 kernel: the dQ pass up to its fp32 dS = P o (dP - D) (same bf16 images, same MFMA order, same exponential,
 * D from the same row-dot pass), summed per diagonal before it would be rounded for the second product; the two waves of a
 * 16-query tile merge st = 0 then st = 1, key chunks ascend, query tiles are added in order by a last pass.  dqkb_rows is the
 * same row sum of dqk as above.  Four bf16 images of 32 time steps, four parked 16 x 16 tiles and four arrays of diagonals must
 * fit the 160 KiB of LDS: 256 (F + 8) + 4608 + 16 (ceil32(T) + 32) bytes (F = 448: T <= 2624; F = 64: T <= 8700); anything
 * larger is an argument error.
 *
 * babe_attn_qk_wgrad_bf16: dqk and a1 stay fp32 in memory and are rounded once, to nearest even, on their way into LDS; the
 * product runs on v_mfma_f32_32x32x16_bf16 with fp32 accumulators in ascending (b, t).  Chunk plan and workspace size are those
 * of babe_attn_qk_wgrad. */
long babe_attn_qk_wgrad_bf16_workspace(int B, int HF, int T);
int babe_attn_qk_wgrad_bf16(const float* dqk, const float* a1, float* dW, float* ws, int B, int HF, int T, float alpha, float beta,
                            void* stream);
long babe_attn_param_vjp_bf16_workspace(int B, int H, int T, int num_buckets);
int babe_attn_param_vjp_bf16(const float* qk, const float* qk_bias, const float* a, const int* bucket, const float* emb,
                             int num_buckets, const float* out, const float* lse, const float* dout, const float* dqk, float* ws,
                             float* demb_rows, long demb_bs, float* dqkb_rows, long dqkb_bs, int B, int H, int F, int T,
                             float scale, void* stream);
/* babe_gn_param_grad for a = z * scale WITHOUT the GELU (norm2 / affine2 of the attention branch): dscale = cs * sum_i da*z. */
int babe_gn_param_grad_nogelu(const float* z, const float* da, const float* stats, const float* gamma, const float* film_aff,
                              long film_bs, float cs, float* dgamma_rows, long dg_bs, float* dfilm, long dfilm_bs, int B, int C,
                              int G, long hw, void* stream);
/* out[b][c][i] = x[b][c][i] * scale[b*C + c], dense [B][C][hw] (out may be x): the input of the attention proj_in, rebuilt for
 * its weight gradient. */
int babe_scale_channels(const float* x, const float* scale, float* out, int B, int C, long hw, void* stream);


/* ---- a whole network from one weights file (csrc/model.hip; the format: csrc/model_file.h, written by babe_amd/model_file.py,
 * INTEGRATION.md section 2): what a host without Python calls instead of restating UnetEngine.__init__, ops.PackedConv, _FilmIndex,
 * STFTOps and CEval.  The loader packs every image with this library's own pack kernels from the raw weights, as the Python
 * engine does with its default forms, so babe_unet_fwd / _vjp, babe_score_eval and babe_sample_bwe on a loaded model are
 * bit-identical to the same calls on Python-built descriptors (tests/test_gpu_model_c.py, tests/test_gpu_bf16_library.py).
 * Precision is the HOST's choice at load time (the _ex forms; BABE_PRECISION_*), as --precision is for python -m babe_amd.restore:
 * the file always holds the fp32 master weights and says network.precision = f32.  Each conv's images follow
 * babe_conv_splits_for(shape, precision, 1): bf16 / bf16x3 images where bf16 MFMA gains, fp32 images for the 2-channel convs, the
 * narrow (1,1) convs and the folded frequency-encoding convs (so a use_fencoding file loads at any precision).  babe_model_load /
 * babe_model_create are the _ex forms at BABE_PRECISION_F32.
 * Ownership: THE exception to "the library never allocates / never synchronises".  create / load allocate one arena on the
 * CURRENT device (plus the CQT plan's tables), enqueue the upload and the pack kernels on `stream`, and wait on `stream` once
 * before they release their host staging; destroy frees.  No other entry point here allocates or waits.  The device is recorded:
 * babe_model_unet_plan / _cqt_plan / _eval_desc refuse while another device is current.  The handle outlives every plan pointer
 * and descriptor taken from it: destroy it last.
 * Refused with a message, before any device call, nothing allocated: a missing or empty file, a wrong magic, an unknown version, a
 * truncated file, tensor data that overlaps or leaves the file, a duplicate / missing / unexpected name, a shape that does not fit
 * the settings, attention flags (unless babe_model_load_opt / _create_opt opt in), a file whose network.precision is not f32, a requested precision outside 0..2, use_fencoding with
 * bins per octave != 64, an audio length the mixed-radix FFT plan does not cover. */
typedef struct { const char* name; int ndim; long shape[4]; const float* data; } babe_model_entry;   /* host fp32, state_dict name */
typedef struct { const char* key; const char* str; double num; } babe_model_kv;                       /* str != NULL: a string setting */
typedef struct {
    int L; float fs; int nocts, bpo; int Ns[8];
    long params;                 /* parameters and buffers of the network (the aux tables not counted) */
    long device_bytes;           /* the arena, exactly as allocated */
    long cqt_device_bytes;       /* the CQT plan's own tables (babe_cqt_plan_create_ex) */
    int device;                  /* the device the model lives on */
    double load_ms[3];           /* host wall time of create: read + parse + validate | staging + upload | pack + CQT plan + the wait */
} babe_model_summary;
void* babe_model_load(const char* path, void* stream);               /* NULL on failure: babe_last_error() */
/* the same from tables in host memory: entries = every tensor the file would hold (the two aux.* tables included), settings = its
 * settings block (dotted keys) */
void* babe_model_create(const babe_model_entry* entries, int n, const babe_model_kv* settings, int nsettings, void* stream);
/* the same with the conv arithmetic chosen: precision = BABE_PRECISION_F32 / _BF16 / _BF16X3 */
void* babe_model_load_ex(const char* path, int precision, void* stream);
void* babe_model_create_ex(const babe_model_entry* entries, int n, const babe_model_kv* settings, int nsettings, int precision,
                           void* stream);
/* the same with the attention core chosen as well.  attention = BABE_ATTENTION_REFUSE: a file with network.attention_layers set
 * is refused, as by every form above (they are these with REFUSE); _F32 / _BF16: such a file loads and its attention branches run
 * on babe_attn_fwd / _vjp or on the _bf16 pair, whatever `precision` is - the host's opt-in, as attention_precision is in Python.
 * The loader reads network.attention_layers.* and the network.attention_dict.* leaves num_heads, bias_qkv, use_rel_pos,
 * rel_pos_num_buckets, rel_pos_max_distance (defaults 8, 0, 1, 32, 64), expects the branch's tensors (norm2.gamma, affine2.*,
 * gate2.*, attn_block.proj_in / proj_out / qk.weight, qk.bias with bias_qkv, rel_pos.relative_attention_bias.weight with
 * use_rel_pos) and refuses what the kernels do not cover.  On a file without attention layers the choice does nothing.
 * reserved: zero. */
enum { BABE_ATTENTION_REFUSE = 0, BABE_ATTENTION_F32 = 1, BABE_ATTENTION_BF16 = 2 };
typedef struct { int precision; int attention; int reserved[6]; } babe_model_options;
void* babe_model_load_opt(const char* path, const babe_model_options* options, void* stream);
void* babe_model_create_opt(const babe_model_entry* entries, int n, const babe_model_kv* settings, int nsettings,
                            const babe_model_options* options, void* stream);
int babe_model_precision(const void* model);                         /* what it was loaded with; -1: null model */
int babe_model_attention(const void* model);                         /* the attention core it was loaded with (BABE_ATTENTION_*); -1: null model */
void babe_model_destroy(void* model);
int babe_model_info(const void* model, babe_model_summary* info);
int babe_model_setting(const void* model, const char* key, double* value);   /* a numeric setting of the file; strings and unknown keys: error */
const void* babe_model_unet_plan(const void* model);                 /* for babe_unet_workspace_bytes / babe_unet_fwd / babe_unet_vjp */
const void* babe_model_cqt_plan(const void* model);                  /* babe_cqt_plan_create_ex(fs, L, octaves, bins, beta, 8192) */
/* Fills EVERY field of desc: the plans, L, the embedding / FiLM pointers and dimensions, nfft, fs, env_inv, tw4096, and the sampler
 * fields from the file's defaults (K and fit from tester.blind_bwe, blind = 1, shared = 0, hpf, xi, score_mode 0, audio_len_norm = L).
 * unet_state: the caller's (babe_unet_state_create), one per concurrent stream.  The host overrides what it wants afterwards. */
int babe_model_eval_desc(const void* model, void* unet_state, babe_eval_desc* desc);


/* ---- a recording FILE: rate conversion and the denoiser pre-pass in front of babe_restore_recording (csrc/dn_engine.hip, host
 * parts in csrc/dn_host.h) - the flow of BlindTester.test_real_blind_bwe_complete with a denoiser (testing/
 * denoise_and_bwe_tester.py:248-411): file rate -> denoiser rate, apply_denoiser over the whole file, denoiser rate -> model rate,
 * then normalise / blind estimate / AR pass.  What long_file.restore_recording_complete(fs=..., denoiser=...) sequences from Python,
 * for a host without it; every piece is bit-identical to its Python counterpart (tests/test_gpu_dn_library.py). */
/* The table of babe_resample_sinc, host only (no GPU): babe_amd/resample.py::sinc_resample_kernel / _table for the two rates (any
 * common factor is divided out here), lowpass_filter_width 6, rolloff 0.99.  The builder follows the published float32 operation
 * sequence, one rounding per operation, no contraction - evaluating the formulas in double and rounding once gives another table
 * (up to 2.1e-5 of the largest tap for 441:320).  width, orig, new_ and krange (the support |t| < 6) are exactly Python's; a tap
 * differs from Python's only through the sine / cosine implementation.  _size returns the number of floats of kernel
 * (new_ (2 width + orig); krange has 2 new_ ints), -1 for rates outside 1..2^20. */
long babe_resample_sinc_table_size(long orig_freq, long new_freq, int* width, int* orig, int* new_);
int babe_resample_sinc_table(long orig_freq, long new_freq, float* kernel, int* krange);
/* ceil(new L / orig) as the published code computes it (the quotient passes through float32): resample.py::resampled_length */
long babe_resampled_length(long L, long orig_freq, long new_freq);

/* The denoiser from one weights file: the container of babe_model_load (csrc/model_file.h) with the string setting kind =
 * "denoiser", the leaves of the configuration's tester.denoiser node (depth, num_tfc, num_stages, use_SAM, use_fencoding, f_dim,
 * sample_rate_denoiser, segment_size, stft_win_size, stft_hop_size) under tester.denoiser.*, the reference state_dict
 * (freq_encoding.fembeddings included) and two tables whose bits the Python host defines: aux.tw4096 [2048][2] and aux.fade
 * [2048], the Hamming window of apply_denoiser's cross-fade.  babe_amd/model_file.py::export_denoiser writes it.
 * Ownership is babe_model_load's: create / load allocate ONE arena on the current device, upload, pack every convolution with
 * babe_dn_pack_weights (mode 0; the four parity images of a transposed one) on `stream`, and wait on `stream` once; destroy frees;
 * nothing else here allocates or waits.  Refused with a message before any device call: a file that is no denoiser file (a UNet
 * file), a missing / duplicate / unexpected / wrong-shape tensor, use_csff / use_cam / use_fam / use_tdf / use_alttdfs set, a depth
 * outside 1..6, a number of stages outside {1, 2}, use_fencoding with f_dim != stft_win_size / 2 + 1. */
typedef struct {
    int depth, num_tfc, num_stages, use_SAM, use_fencoding, f_dim;
    int sample_rate, win, hop;
    long segment;                /* samples: int(sample_rate_denoiser * segment_size) */
    long params;                 /* parameters and buffers of the network (the aux tables not counted) */
    long device_bytes;           /* the arena, exactly as allocated */
    int device;
    double load_ms[3];           /* as babe_model_summary */
} babe_denoiser_summary;
void* babe_denoiser_load(const char* path, void* stream);           /* NULL on failure: babe_last_error() */
void* babe_denoiser_create(const babe_model_entry* entries, int n, const babe_model_kv* settings, int nsettings, void* stream);
void babe_denoiser_destroy(void* denoiser);
int babe_denoiser_info(const void* denoiser, babe_denoiser_summary* info);
/* The split-K rule of the denoiser's convolutions, host only: the number of input-channel splits networks/denoiser.py::_split_k
 * gives a launch of these shapes (1: none).  Reads B, Cin, Cout, OH, OW, KH, KW. */
int babe_dn_ksplit(const babe_dnconv_args* a);
/* MultiStage_denoise.forward from the handle: X [B][2][T][F] dense -> pred2, pred1 [B][2][T][F] dense (one stage: pred1 alone,
 * pred2 is not looked at; two stages: pred1 may be NULL).  The launch sequence of networks/denoiser.py::DenoiserEngine.forward -
 * same kernels, order and arguments, so the same bits.  Buffers are carved from ws (babe_denoiser_workspace_bytes, -1 on bad
 * arguments); no allocation, no synchronisation.  F must be f_dim when the network has frequency encodings. */
long babe_denoiser_workspace_bytes(const void* denoiser, int B, int T, int F);
int babe_denoiser_fwd(const void* denoiser, const float* X, float* pred2, float* pred1, void* ws, long ws_bytes, int B, int T, int F,
                      void* stream);
/* The walk of DenoiserPrepass.apply_denoiser, host only: full segments while start + segment < n, hopping by segment - overlap,
 * then one zero-padded remainder.  Fills starts up to max entries and returns the number of segments; -1 where the reference fails
 * (after a first full segment the remainder is longer than segment - overlap) and unless n >= 1, overlap >= 1, segment >= 2 overlap. */
long babe_denoise_signal_plan(long n, long segment, long overlap, long* starts, long max);
/* DenoiserPrepass.apply_denoiser: x [B][n] (row stride x_bs) -> out [B][n], at the denoiser's rate.  Per segment of the walk:
 * babe_dn_segment_pad (cut, zero tail of one STFT window) -> babe_dn_stft -> babe_denoiser_fwd -> babe_dn_istft ->
 * babe_dn_fade_add.  Everything is checked before the first launch; no allocation, no synchronisation. */
long babe_denoise_signal_workspace_bytes(const void* denoiser, int B, long n);
int babe_denoise_signal(const void* denoiser, const float* x, long x_bs, float* out, long out_bs, int B, long n, void* ws,
                        long ws_bytes, void* stream);
/* its two element-wise kernels as entries (tests pin them one by one):
 * dst[b][i] = i < n ? x[b][i] : 0 for i in [0, len), n <= len */
int babe_dn_segment_pad(const float* x, long x_bs, long n, float* dst, long dst_bs, long len, int B, void* stream);
/* out[b][i] = out[b][i] + y[b][i] w(i) for i in [0, n), n <= seg: w = fade[i] on [0, size) with fade_in, fade[size + i - (seg - size)]
 * on [seg - size, seg) with fade_out, 1 elsewhere (fade: device [2 size], seg >= 2 size).  One rounded product, one rounded sum,
 * in the order of `y[:, :size] *= wl; y[:, -size:] *= wr; out += y`. */
int babe_dn_fade_add(const float* y, long y_bs, float* out, long out_bs, int B, long n, long seg, const float* fade, int size,
                     int fade_in, int fade_out, void* stream);

/* long_file.rate_plan, host only.  fs_denoiser 0: no denoiser.  lengths = {Lfile, samples the denoiser sees, samples handed to
 * the model}.  Returns bit 0: conv[0] runs (file rate -> denoiser rate; without a denoiser file rate -> model rate), bit 1:
 * conv[1] runs (denoiser rate -> model rate); -1 on bad arguments.  With a denoiser both hang on fs_file != fs_denoiser, as in the
 * reference: a file already at the denoiser's rate reaches the model unconverted. */
int babe_restore_file_plan(long Lfile, long fs_file, long fs_denoiser, long fs_model, long* lengths);
typedef struct { const float* kernel; const int* krange; int width, orig, new_; } babe_sinc_table;   /* device tables, the caller's */
typedef struct {
    babe_recording_desc rec;     /* as for babe_restore_recording; blind_starts refer to lengths[2]                         */
    const void* denoiser;        /* babe_denoiser_load handle, or NULL: no pre-pass                                          */
    babe_sinc_table conv[2];     /* the conversion before / after the denoiser; kernel NULL: that conversion does not run    */
    long lengths[3];             /* babe_restore_file_plan's                                                                 */
} babe_file_desc;
long babe_restore_file_workspace_bytes(const babe_file_desc* d);
/* rec [Lfile] at the file's rate -> conv[0] -> babe_denoise_signal -> conv[1] -> exactly babe_restore_recording on the result:
 * out [lengths[2]], filter_out, blind_pred as there; pre_out [lengths[2]] (may be NULL) receives the signal handed to that last
 * step.  rec.std_dev NULL: the converted file's standard deviation is computed by the call (babe_row_std).  Every argument is
 * checked on the host before the first device call; no allocation, no synchronisation. */
int babe_restore_file(const babe_file_desc* d, const float* rec, long Lfile, float* out, float* filter_out, float* blind_pred,
                      float* pre_out, long seed, long clip0, void* ws, long ws_bytes, void* stream);

/* ---- Training: the fused optimizer tail (csrc/optim.hip).  Gradient norm, clipping, Adam and the EMA of the weights over a TABLE
 * of tensors in device memory - a network has hundreds of them, too many for kernel arguments.  Entry: fp32 arrays of n
 * elements, 4-byte aligned (16-byte accesses are used where every pointer of the entry allows them).  g NULL: an EMA-only
 * entry - p is read, ema = ema ema_s + p ema_1ms, nothing else is touched (a parameter without a gradient this step, a frozen
 * parameter).  ema NULL: no EMA for that entry.  Both NULL: the entry is skipped. */
typedef struct { float* p; const float* g; float* m; float* v; float* ema; long n; } babe_opt_tensor;
/* One workgroup's share: elements [off, off + n) of tensor t of the table. */
typedef struct { long off; int t; int n; } babe_opt_chunk;
/* Host only: cuts nt tensors of n[i] elements into chunks of at most `chunk` elements (a positive multiple of 4), tensor by
 * tensor in table order, every element in exactly one chunk and no chunk across two tensors.  Writes out[0 .. count) and returns
 * the count; out NULL: counts only.  -1: nt <= 0, an n[i] <= 0, a bad chunk size, or more than cap chunks. */
long babe_opt_chunks(const long* n, long nt, long chunk, babe_opt_chunk* out, long cap);
/* partials[c] = sum of g^2 over chunk c in double (0 for an entry without g), then norm_out[0] = sqrt(sum of the partials), a
 * double in device memory: two launches, the second one workgroup.  Fixed summation order, no atomics: the same bits every run. */
int babe_grad_sqnorm(const babe_opt_tensor* table, const babe_opt_chunk* chunks, long nchunks, double* partials, double* norm_out,
                     void* stream);
/* Per element of every chunk, with coef = norm ? min(1, max_norm / (norm[0] + 1e-6)) : 1 read from device memory:
 *   g' = coef g;  m += (1 - beta1) (g' - m);  v = beta2 v + (1 - beta2) g' g';  p -= lr_over_bc1 (m / (sqrt(v) / bc2_sqrt + eps));
 *   ema = ema ema_s + p ema_1ms  (the new p)
 * i.e. clip_grad_norm_ + torch.optim.Adam (no amsgrad / weight decay / maximize) + the trainer's EMA; g itself is NOT rewritten.
 * g', m and v in fp32 with the roundings of torch's kernels (its bits from equal inputs); the update of p and the EMA in double
 * from the stored moments, rounded once.
 * lr_over_bc1 = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step), formed by the caller in double.  One launch.
 * BABE_ERR_ARG before any launch: NULL table or chunks, nchunks <= 0, a beta outside [0, 1), eps <= 0, a negative lr_over_bc1. */
int babe_adam_ema_step(const babe_opt_tensor* table, const babe_opt_chunk* chunks, long nchunks, const double* norm, double max_norm,
                       double lr_over_bc1, double bc2_sqrt, double beta1, double beta2, double eps, double ema_s, double ema_1ms,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
