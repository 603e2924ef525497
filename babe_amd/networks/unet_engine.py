"""CQTDiff+ UNet body on the babe_hip kernels: forward and hand-wired input-VJP.

Mirrors the wiring of /root/reference/networks/cqtdiff+.py:746-839 (forward) and
ResnetBlock.forward :452-493; the VJP replaces torch.autograd through the UNet
(/root/reference/testing/blind_bwe_sampler.py:120).  No torch compute ops are used on
the data path: torch only allocates buffers; every tensor op is a C-ABI call (ops.py).

Layout: activations are [B, C, F, T] fp32, T contiguous.  Octave/skip concatenations are
never materialised as copies of big tensors: producers write straight into frequency
sub-views of the consumer's buffer and channel concatenation is a two-source conv input.
Each dilation layer keeps exactly one tensor (its input) for the VJP; GroupNorm / FiLM /
GELU are recomputed in the backward kernels.

Plan and state, as in csrc/unet_engine.hip: _Block / _Attn / _FilmIndex hold weights only and are shared by every engine handle;
what an evaluation leaves between forward and vjp is one _State per handle (UnetEngine.clone_state makes another).
"""
import copy
import math

import torch

from .. import ops
from ..forms import FORMS
from .unet_c import CPlan, CUnet, c_block

RS2 = 1.0 / math.sqrt(2.0)


class _Attn:
    """The time-attention branch of a ResnetBlock (reference ResnetBlock.forward with attention_dict, TimeAttentionBlock):
        a1  = proj_in(z * scale2)                        scale2 = norm2.gamma * (affine2(emb) + 1) / (std_g(z) + eps)  (no GELU)
        qk  = Conv1d(a1.view(B, H*F, T))                 a (1,1) conv on the [B, H*F, 1, T] view
        o   = attention(qk, V = a1)                      csrc/attention.hip, or csrc/attention_bf16.hip (attention_precision)
        z'  = (gate2(emb) * proj_out(o) + z) / sqrt2
    z is the block's proj_in output, z' feeds the dilated conv stack.  Weights only, shared by every engine handle.
    The three convs are packed at the network's precision, each under the rule of every other conv (babe_conv_splits_for): the
    wide qk conv runs on the bf16 kernels under 'bf16'; proj_in and proj_out have 8 channels on one side and stay on the fp32
    (1,1) kernels at any precision, as does qk under 'bf16x3'."""

    def __init__(self, g, Fdim, N, film_index, opts, prefix="", precision="f32"):
        self.H, self.bias_qkv, self.rel_pos, self.nbk, self.maxd = opts
        self.F = Fdim
        self.p = prefix
        self.scale = float(Fdim) ** -0.5
        self.gamma = g("norm2.gamma").reshape(-1).contiguous()
        self.film_off = (film_index.add(g("affine2.weight"), g("affine2.bias"), prefix + "affine2"),
                         film_index.add(g("gate2.weight"), g("gate2.bias"), prefix + "gate2"))
        self.proj_in = ops.PackedConv(g("attn_block.proj_in.weight"), precision)
        self.proj_out = ops.PackedConv(g("attn_block.proj_out.weight"), precision)
        self.proj_out_w = g("attn_block.proj_out.weight").contiguous()             # raw weights (the gate2 gradient)
        w = g("attn_block.qk.weight")
        self.qk = ops.PackedConv(w.reshape(w.shape[0], w.shape[1], 1, 1), precision)
        self.qk_bias = g("attn_block.qk.bias").contiguous() if self.bias_qkv else None
        self.emb = g("attn_block.rel_pos.relative_attention_bias.weight").contiguous() if self.rel_pos else None


class _Block:
    """One ResnetBlock: its packed weights, shared by every engine handle and written after __init__ by UnetEngine.refresh alone.
    idx: the block's position in UnetEngine.blocks(), which is where a _State keeps what an evaluation saves for it."""

    FOLDED = ("proj_in", "res_conv")      # the convs of an init block with frequency encodings that see all 66 input channels

    def __init__(self, sd, prefix, num_dils, film_index, proj_after=False, precision="f32", attn=None, fenc=None, idx=None):
        """attn: (Fdim, attention options) if the block carries a time-attention layer.
        fenc: the [64, 64] frequency-encoding table of an init block built with use_fencoding.  Its proj_in / res_conv weights
        are [N, 66, 1, 1] over cat(signal 2, encodings 64): the convs are packed from the 2 signal columns and the encodings'
        share, constant over batch and time, is the bias table fb_* [N, 64] the conv adds in its epilogue (ops.fenc_bias)."""
        self.idx = idx
        self.p = prefix
        self.nd = num_dils
        self.proj_after = proj_after
        g = lambda k: sd.get(prefix + k)
        PC = lambda w: ops.PackedConv(w, precision)
        self.fenc = fenc
        if fenc is not None:
            for name in self.FOLDED:
                w = g(name + ".weight")
                assert w is not None and w.shape[1:] == (66, 1, 1), f"{prefix}{name}.weight: expected [N, 66, 1, 1] with frequency encodings"
                if ops.PackedConv.splits_for((w.shape[0], 2, 1, 1), precision):
                    raise NotImplementedError(f"use_fencoding with precision={precision!r}: the init block's (1,1) convs would run on "
                                              "the bf16 kernels, which have no frequency bias")
                setattr(self, name, PC(w[:, :2].contiguous()))
                setattr(self, "fb_" + name, ops.fenc_bias(w.reshape(w.shape[0], 66), fenc, torch.empty(w.shape[0], 64, device=w.device)))
        else:
            self.fb_proj_in = self.fb_res_conv = None
            self.proj_in = PC(g("proj_in.weight")) if g("proj_in.weight") is not None else None
            self.res_conv = PC(g("res_conv.weight")) if g("res_conv.weight") is not None else None
        self.proj_out = PC(g("proj_out.weight")) if (proj_after and g("proj_out.weight") is not None) else None
        self.H = [PC(g(f"H.{d}.weight")) for d in range(num_dils)]
        self.Hw = [g(f"H.{d}.weight").contiguous() for d in range(num_dils)]       # raw weights (the FiLM gate gradient)
        self.gamma = [g(f"norm.{d}.gamma").reshape(-1).contiguous() for d in range(num_dils)]
        self.N = self.H[0].Cout
        self.k53 = self.H[0].KH > 1
        self.film_off = []            # (affine offset, gate offset) into the batched FiLM output
        for d in range(num_dils):
            self.film_off.append((film_index.add(g(f"affine.{d}.weight"), g(f"affine.{d}.bias"), prefix + f"affine.{d}"),
                                  film_index.add(g(f"gate.{d}.weight"), g(f"gate.{d}.bias"), prefix + f"gate.{d}")))
        self.attn = _Attn(g, attn[0], self.N, film_index, attn[1], prefix, precision) if attn else None
        self._cblk = None

    def c_block(self):
        """The library's descriptor of this block (babe_unet_block), made on first use: the fused (1,1) block passes take it."""
        if self._cblk is None:
            self._cblk = c_block(self)
        return self._cblk

    def dil(self, d):
        return 2 ** d if self.k53 else 1


class _State:
    """What one evaluation leaves between forward and vjp.  Every engine handle has one of its own (UnetEngine.clone_state), so two
    handles over the same weights can be in flight together.  The per-block records are lists over _Block.idx; all of it lives
    until vjp consumes it or the next forward of this state replaces it."""

    def __init__(self, nblocks):
        self.B = self.Ts = None           # batch rows and the time length of every level
        self.train = False                # forward(train=True): inp / zpo / pyrs / film are kept as well
        self.film = None                  # training: the FiLM vectors
        self.hs = self.pyrs = None        # the encoder's skip tensors; training: the pyramid convs' inputs
        self.saved = [None] * nblocks     # per dilation layer (z, stats, scale, gate)
        self.attn = [None] * nblocks      # the attention branch's (z, stats, scale, gate, a1, qk, o, lse)
        self.inp = [None] * nblocks       # training: the block's input(s) ...
        self.zpo = [None] * nblocks       # ... and proj_out's input, for the weight gradients
        self.scratch = {}                 # name -> flat buffer, grown on demand
        self.cunet = None                 # BABE_UNET_C: the library-side state and workspace (unet_c.CUnet) ...
        self.c_fwd = False                # ... and whether the last forward ran there


class _FilmIndex:
    """Collects every FiLM Linear (affine/gate of every dilation layer) into one [J,emb] matrix."""

    def __init__(self):
        self.W, self.b, self.J = [], [], 0
        self.keys = []                 # (state_dict prefix of the Linear, row offset, rows)

    def add(self, W, b, key=None):
        off = self.J
        self.W.append(W)
        self.b.append(b)
        self.J += W.shape[0]
        self.keys.append((key, off, W.shape[0]))
        return off

    def finalize(self):
        self.Wcat = torch.cat(self.W, 0).contiguous()
        self.bcat = torch.cat(self.b, 0).contiguous()
        self._parts = (self.W, self.b)
        self.W = self.b = None

    def refresh(self, sd=None):
        """Rebuild Wcat / bcat in place after an optimizer step: from sd (the current parameters) where the pieces have keys,
        from the (parameter-aliasing) pieces themselves otherwise."""
        W, b = self._parts
        if sd is not None:
            W = [sd[k + ".weight"] if k is not None else w for (k, _, _), w in zip(self.keys, W)]
            b = [sd[k + ".bias"] if k is not None else v for (k, _, _), v in zip(self.keys, b)]
        torch.cat(W, 0, out=self.Wcat)
        torch.cat(b, 0, out=self.bcat)


class ParamGrads:
    """Per-call parameter-gradient buffers of a training step, shared by the clip lanes: every lane writes only its own batch
    rows, and one fixed-order reduction over the rows after the join (UnetEngine.param_grads) makes the result independent of
    the lane count.  rows [B, n]: per-row weight gradients of every conv and GroupNorm gamma, flat (layout: key -> (offset,
    shape)); dfilm [B, J]: gradient w.r.t. the concatenated FiLM Linear output.
    qk {block prefix: (dqk [B, 2HF, T], a1 [B, HF, T])}: the operands of the attention blocks' qk weight gradients.  Those are
    [2HF, HF] matrices of up to 25.7 M floats, far too large for a per-row copy: the lanes leave their rows of both operands here
    (allocated on the caller's stream before the lanes fork, so they outlive the lanes' buffer recycling) and param_grads
    forms each gradient in one batch-summed launch after the join."""

    def __init__(self, layout, rows, dfilm, qk=None, wgrad="f32"):
        self.layout, self.rows, self.dfilm, self.qk = layout, rows, dfilm, qk or {}
        self.wgrad = wgrad                           # conv weight-gradient arithmetic of this step (UnetEngine.wgrad), every lane's

    @classmethod
    def new(cls, eng, B):
        rows = torch.zeros(B, eng.grad_numel, device=eng.dev, dtype=torch.float32)
        dfilm = torch.zeros(B, eng.film_idx.J, device=eng.dev, dtype=torch.float32)
        qk = {}
        for blk, level in eng.attn_blocks:
            HF, T = blk.attn.H * blk.attn.F, eng._state.Ts[level]
            qk[blk.p] = (torch.empty(B, 2 * HF, T, device=eng.dev, dtype=torch.float32),
                         torch.empty(B, HF, T, device=eng.dev, dtype=torch.float32))
        return cls(eng.grad_layout, rows, dfilm, qk, eng.wgrad)

    def lane(self, b0, b1):
        return ParamGrads(self.layout, self.rows[b0:b1], self.dfilm[b0:b1], {k: (d[b0:b1], a[b0:b1]) for k, (d, a) in self.qk.items()},
                          self.wgrad)

    def row(self, key):
        off, shape = self.layout[key]
        n = 1
        for v in shape:
            n *= v
        return self.rows[:, off:off + n]


class UnetEngine:
    def __init__(self, sd, Ns, num_dils, num_octs=7, bins_per_oct=64, precision="f32", attention_layers=None, attention_dict=None,
                 attention_precision=None):
        """sd: dict of DEVICE fp32 tensors with the reference's state_dict key names.
        precision: conv arithmetic, 'f32' (exact fp32 MFMA, the parity path), 'bf16x3' or 'bf16'.
        attention_layers / attention_dict: the reference's time-attention flags (one per octave + the bottleneck).
        attention_precision: arithmetic of the attention core.  None: fp32, and a network of another precision refuses attention
        layers; 'f32' / 'bf16': the core on babe_attn_fwd / _vjp or on babe_attn_fwd_bf16 / _vjp_bf16, in a network of any
        precision.  Does nothing without attention layers."""
        from .cqtdiff_plus import attention_options, check_attention_precision
        check_attention_precision(attention_precision)
        att = [int(bool(v)) for v in (attention_layers or [0] * (num_octs + 1))]
        self.has_attention = any(att)
        if self.has_attention and precision != "f32" and attention_precision is None:
            raise NotImplementedError(f"attention layers run in fp32 only (precision={precision!r}) unless attention_precision "
                                      "('f32' | 'bf16') opts in")
        self.attn_core = (attention_precision or "f32") if self.has_attention else None      # what attn_fwd / attn_vjp launch
        opts = attention_options(attention_dict)
        A = lambda flag, Fd: (Fd, opts) if flag else None
        self.precision = precision
        # training: arithmetic of the UNet body's conv weight gradients, 'f32' or 'bf16' (ops.conv_wgrad_rows).  A training step
        # reads it once, into its ParamGrads, so the lane clones of this engine always agree
        self.wgrad = "f32"
        self.Ns, self.num_dils, self.nocts, self.bpo = list(Ns), list(num_dils), num_octs, bins_per_oct
        self.dev = sd["embedding.RFF_freq"].device
        fi = _FilmIndex()
        n = num_octs                                 # blocks() order: init, main, mid_blk, mid_out, up_out, up_blk
        self.emb_W = [(sd[f"embedding.MLP.{i}.weight"].contiguous(), sd[f"embedding.MLP.{i}.bias"].contiguous()) for i in range(3)]
        self.rff_freq = sd["embedding.RFF_freq"].reshape(-1).contiguous()
        self.init_blk, self.main_blk, self.pyr_conv = [], [], []
        for i in range(num_octs):
            fe = sd.get(f"freq_encodings.{i}.embeddings")
            self.init_blk.append(_Block(sd, f"downs.{i}.0.", 1, fi, idx=i, precision=precision,
                                        fenc=fe.reshape(64, bins_per_oct).contiguous() if fe is not None else None))
            self.pyr_conv.append(ops.PackedConv(sd[f"downs.{i}.1.weight"], precision))
            self.main_blk.append(_Block(sd, f"downs.{i}.2.", num_dils[i], fi, idx=n + i, precision=precision, attn=A(att[i], (i + 1) * bins_per_oct)))
        self.mid_blk = _Block(sd, "middle.0.1.", num_dils[-1], fi, idx=2 * n, precision=precision, attn=A(att[-1], num_octs * bins_per_oct))
        self.mid_out = _Block(sd, "middle.0.0.", 1, fi, idx=2 * n + 1, proj_after=True, precision=precision)
        self.up_out, self.up_blk = [], []
        for i in range(num_octs):
            j = num_octs - 1 - i
            self.up_out.append(_Block(sd, f"ups.{i}.0.", 1, fi, idx=2 * n + 2 + i, proj_after=True, precision=precision))
            self.up_blk.append(_Block(sd, f"ups.{i}.1.", num_dils[j], fi, idx=3 * n + 2 + i, precision=precision, attn=A(att[j], (j + 1) * bins_per_oct)))
        fi.finalize()
        self.film_idx = fi
        assert all(b.idx == k for k, b in enumerate(self.blocks()))
        self._buckets = {}                           # T -> the relative-position bucket table (shape only), every handle's
        self._plan = CPlan()                         # the library-side plan over these weights, every handle's (c_plan)
        self._state = _State(len(self.blocks()))
        # training: flat per-row layout of the conv weights and GroupNorm gammas (ParamGrads), the convs the refresh repacks
        self.grad_layout, self.grad_numel, self.packs = {}, 0, []
        for blk in self.blocks():
            for name in ("proj_in", "res_conv", "proj_out"):
                if getattr(blk, name) is not None:
                    folded = blk.fenc is not None and name != "proj_out"       # the parameter has all 66 input columns
                    self._add_grad(blk.p + name + ".weight", getattr(blk, name), (blk.N, 66, 1, 1) if folded else None)
            for d in range(blk.nd):
                self._add_grad(blk.p + f"H.{d}.weight", blk.H[d])
                self._add_grad(blk.p + f"norm.{d}.gamma", None, (1, blk.N, 1, 1))
            if blk.attn is not None:
                at = blk.attn
                self.packs += [(blk.p + "attn_block.proj_in.weight", at.proj_in), (blk.p + "attn_block.proj_out.weight", at.proj_out),
                               (blk.p + "attn_block.qk.weight", at.qk)]
                # per-row gradients of the attention branch; qk.weight is batch-summed after the join instead (ParamGrads.qk)
                self._add_grad(blk.p + "norm2.gamma", None, (1, blk.N, 1, 1))
                self._add_grad(blk.p + "attn_block.proj_in.weight", None, (at.H, blk.N, 1, 1))
                self._add_grad(blk.p + "attn_block.proj_out.weight", None, (blk.N, at.H, 1, 1))
                if at.bias_qkv:
                    self._add_grad(blk.p + "attn_block.qk.bias", None, (2 * at.H * at.F,))
                if at.rel_pos:
                    self._add_grad(blk.p + "attn_block.rel_pos.relative_attention_bias.weight", None, (at.nbk, at.H))
        for i, pc in enumerate(self.pyr_conv):
            self._add_grad(f"downs.{i}.1.weight", pc)
        # (block, level whose time length it runs at) of every block with attention
        self.attn_blocks = [(b, i) for i, b in enumerate(self.main_blk) if b.attn is not None]
        self.attn_blocks += [(self.mid_blk, n - 1)] if self.mid_blk.attn is not None else []
        self.attn_blocks += [(b, n - 1 - i) for i, b in enumerate(self.up_blk) if b.attn is not None]

    def _add_grad(self, key, pc, shape=None):
        if pc is not None:
            shape = shape or (pc.Cout, pc.Cin, pc.KH, pc.KW)
            self.packs.append((key, pc))
        n = 1
        for v in shape:
            n *= v
        self.grad_layout[key] = (self.grad_numel, tuple(shape))
        self.grad_numel += n

    def blocks(self):
        return self.init_blk + self.main_blk + [self.mid_blk, self.mid_out] + self.up_out + self.up_blk

    def refresh(self, sd):
        """After an optimizer step: repack every conv IN PLACE from sd (the current parameters) and rebuild Wcat / bcat.  The
        GroupNorm gammas and the embedding MLP are views of the parameters already."""
        for key, pc in self.packs:
            w = sd[key]
            if w.shape[1] == 66 and (pc.Cin, pc.KH, pc.KW) == (2, 1, 1):    # a folded init-block conv: the signal columns of the [N, 66] weight
                w = w[:, :2].contiguous()
            pc.repack(w.reshape(pc.Cout, pc.Cin, pc.KH, pc.KW))
        for i, blk in enumerate(self.init_blk):           # ... and the encoding columns, into the SAME bias tables
            if blk.fenc is not None:
                blk.fenc.copy_(sd[f"freq_encodings.{i}.embeddings"].reshape(blk.fenc.shape))
                for name in blk.FOLDED:
                    ops.fenc_bias(sd[blk.p + name + ".weight"].reshape(blk.N, 66), blk.fenc, getattr(blk, "fb_" + name))
        for blk, _ in self.attn_blocks:                   # the attention branch's plain tensors (no-ops while they alias the parameters)
            at, p = blk.attn, blk.p
            pairs = [(at.gamma, sd[p + "norm2.gamma"].reshape(-1)), (at.proj_out_w, sd[p + "attn_block.proj_out.weight"])]
            if at.qk_bias is not None:
                pairs.append((at.qk_bias, sd[p + "attn_block.qk.bias"]))
            if at.emb is not None:
                pairs.append((at.emb, sd[p + "attn_block.rel_pos.relative_attention_bias.weight"]))
            for dst, src in pairs:
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src.reshape(dst.shape))
        self.film_idx.refresh(sd)

    def clone_state(self):
        """A second handle over the SAME weight objects (blocks, packed convs, FiLM index, library-side plan) with a fresh _State,
        so that two batch items can run on two streams at once."""
        c = copy.copy(self)
        c._state = _State(len(self._state.saved))
        return c

    # ------------------------------------------------------------------ helpers
    def buf(self, *shape):
        return torch.empty(*shape, device=self.dev, dtype=torch.float32)

    def scratch(self, name, numel, dtype=torch.float32):
        sc = self._state.scratch
        t = sc.get(name)
        if t is None or t.numel() < numel:
            t = sc[name] = torch.empty(numel, device=self.dev, dtype=dtype)
        return t[:numel]

    def _bucket(self, at, T):
        """The relative-position bucket table of attention branch `at` at time length T (None without rel_pos)."""
        if not at.rel_pos:
            return None
        t = self._buckets.get(T)
        if t is None:
            t = self._buckets[T] = ops.attn_buckets(T, at.nbk, at.maxd).to(self.dev)
        return t

    def embed(self, cnoise, keep=None):
        """cnoise [B,1] -> FiLM vectors for every layer [B, J] (RFF_MLP_Block + all affine/gate Linears).
        keep: a list that receives the MLP's input and layer outputs (training)."""
        h = ops.rff(cnoise, self.rff_freq)
        if keep is not None:
            keep.append(h)
        for W, b in self.emb_W:
            h = ops.linear(h, W, b, relu=True)
            if keep is not None:
                keep.append(h)
        return ops.linear(h, self.film_idx.Wcat, self.film_idx.bcat, relu=False)

    def _film(self, film, off, N):
        return film[:, off:off + N]

    # ------------------------------------------------------------------ ResnetBlock
    def block_fwd(self, blk, x, film, out, x2=None, fold=None):
        """out <- ResnetBlock(cat(x,x2)); out may be a strided frequency sub-view.
        fold (an output head): the caller's next step is fold <- RS2*out + RS2*fold.  A block that runs as the fused pass
        (ops.pw_block_fwd) does that itself: it writes fold instead of out and returns fold."""
        B, _, Fq, T = x.shape
        N = blk.N
        st = self._state
        if st.train:
            st.inp[blk.idx] = (x, x2)
        if blk.proj_in is not None:
            z = ops.conv2d(x, blk.proj_in, self.buf(B, N, Fq, T), x2=x2, fbias=blk.fb_proj_in)
        else:
            assert x2 is None
            z = x if x.is_contiguous() else ops.axpby(x, self.buf(B, N, Fq, T))
        if blk.attn is not None:
            z = self.attn_fwd(blk, z, film)
        if blk.nd == 1 and not blk.k53 and x2 is None and blk.attn is None:
            # a k = (1,1) block: GroupNorm sums, then ONE pass for the rest of the block where the library's rule takes it
            gate = self._film(film, blk.film_off[0][1], N).contiguous()
            ss = ops.pw_block_fwd(blk.c_block(), z, film, gate, out if fold is None else fold,
                                  x=x if blk.proj_in is not None else None, add=fold, train=st.train, precision=self.precision)
            if ss is not None:
                st.saved[blk.idx] = [(z, ss[0], ss[1], gate)]
                return out if fold is None else fold
        saved = []
        # precision='bf16': the GELU output goes to the conv as bf16 units (half the bytes, both conv operands by LDS-DMA)
        units = blk.nd > 0 and ops.units_ok(blk.H[0], N, N, T) and z.is_contiguous()
        if units:
            au = self.scratch("au", B * ops.lib().babe_units_size(N, Fq, T) * 8, torch.int16)
        zsum = None                                          # (part, S): GroupNorm sums of z formed by the conv that wrote it
        for d in range(blk.nd):
            aoff, goff = blk.film_off[d]
            gate = self._film(film, goff, N).contiguous()
            znew = self.buf(B, N, Fq, T)
            ua = ops.units_args(au, blk.H[d], znew, N, dil=blk.dil(d), res=z, oscale=gate, alpha=RS2, rbeta=RS2) if units else None
            if ua is not None and ops.units_supported(ua):       # the library's verdict, not a Python guess
                stats, scale = ops.gn_scale(z, blk.gamma[d], self._film(film, aoff, N))
                ops.scale_gelu_units(z, scale, au)
                ops.conv2d_units(au, blk.H[d], znew, N, args=ua)
                zsum = None
            else:
                a = self.scratch("a", B * N * Fq * T).view(B, N, Fq, T)
                stats, scale = ops.gn_scale_gelu(z, blk.gamma[d], self._film(film, aoff, N), a, fused=zsum)  # (finalize inside the GELU launch)
                # the next layer's GroupNorm reads znew: its sums come out of this conv's epilogue when the F(4,5) kernel runs it
                zsum = ops.conv2d(a, blk.H[d], znew, dil=blk.dil(d), res=z, oscale=gate, alpha=RS2, rbeta=RS2,
                                  fwd_stat=(N // 8) if d + 1 < blk.nd else None)
                if d + 1 >= blk.nd:
                    zsum = None
            saved.append((z, stats, scale, gate))
            z = znew
        if blk.proj_out is not None:
            if st.train:
                st.zpo[blk.idx] = z
            z = ops.conv2d(z, blk.proj_out, self.buf(B, blk.proj_out.Cout, Fq, T))
        if blk.res_conv is not None:
            ops.conv2d(x, blk.res_conv, out, x2=x2, res=z, alpha=RS2, rbeta=RS2, fbias=blk.fb_res_conv)
        else:
            ops.axpby2(z, x, out, RS2, RS2)                  # (x + h)/sqrt2 in one pass
        st.saved[blk.idx] = saved
        return out

    def attn_fwd(self, blk, z, film):
        """z' = (gate2 * proj_out(attention(...)) + z)/sqrt2 (class _Attn); keeps what attn_vjp needs in the state's attention record."""
        at = blk.attn
        B, N, Fq, T = z.shape
        H = at.H
        assert Fq == at.F, f"attention layer built for F={at.F}, got F={Fq}"
        stats, scale = ops.gn_scale(z, at.gamma, self._film(film, at.film_off[0], N))
        a1 = ops.conv2d(z, at.proj_in, self.buf(B, H, Fq, T), in_scale=scale)          # proj_in(norm2(z) * (affine2 + 1))
        qk = ops.conv2d(a1.view(B, H * Fq, 1, T), at.qk, self.buf(B, 2 * H * Fq, 1, T))
        o = self.buf(B, H, Fq, T)
        lse = self.buf(B, H, T)
        ops.attn_fwd(qk, a1, o, lse, at.scale, qk_bias=at.qk_bias, bucket=self._bucket(at, T), emb=at.emb, precision=self.attn_core)
        gate = self._film(film, at.film_off[1], N).contiguous()
        zn = ops.conv2d(o, at.proj_out, self.buf(B, N, Fq, T), res=z, oscale=gate, alpha=RS2, rbeta=RS2)
        self._state.attn[blk.idx] = (z, stats, scale, gate, a1, qk, o, lse)
        return zn

    def attn_vjp(self, blk, gz, c, pg=None):
        """gz <- gradient w.r.t. the attention branch's input z, given c*gz = gradient w.r.t. its output z' (in place).
        pg: ParamGrads of a training step: also the branch's parameter gradients (per row into pg.rows / pg.dfilm; the qk weight
        gradient's operands into pg.qk, for param_grads).  On a bf16 core the table gradient comes from babe_attn_param_vjp_bf16
        and the qk-bias gradient from the row sum of the bf16 core's dqk; everything else of the branch stays fp32."""
        at = blk.attn
        st = self._state
        z, stats, scale, gate, a1, qk, o, lse = st.attn[blk.idx]
        B, N, Fq, T = z.shape
        H = at.H
        p = blk.p
        if pg is not None:                                   # z' = rs2*(gate2 * proj_out(o) + z), before gz is overwritten
            goff = at.film_off[1]
            self._wg(pg, p + "attn_block.proj_out.weight", o, gz, at.proj_out, RS2 * c, oscale=gate, w=at.proj_out_w,
                     dgate=pg.dfilm[:, goff:goff + N], galpha=RS2 * c, precision="f32")
        do = ops.conv2d(gz, at.proj_out, self.buf(B, H, Fq, T), transpose=True, in_scale=gate, alpha=RS2 * c)
        # training: dqk goes straight into this lane's rows of the buffer the qk weight gradient reads after the join
        dqk = self.buf(B, 2 * H * Fq, 1, T) if pg is None else pg.qk[p][0].view(B, 2 * H * Fq, 1, T)
        dv = self.buf(B, H, Fq, T)
        bucket = self._bucket(at, T)
        ops.attn_vjp(qk, a1, o, lse, do, dqk, dv, at.scale, qk_bias=at.qk_bias, bucket=bucket, emb=at.emb, precision=self.attn_core)
        if pg is not None:
            ops.axpby(a1.view(B, H * Fq, 1, T), pg.qk[p][1].view(B, H * Fq, 1, T))
            if at.rel_pos or at.bias_qkv:
                ops.attn_param_vjp(qk, a1, o, lse, do, dqk, at.scale, qk_bias=at.qk_bias, bucket=bucket, emb=at.emb,
                                   demb_rows=pg.row(p + "attn_block.rel_pos.relative_attention_bias.weight") if at.rel_pos else None,
                                   dqkb_rows=pg.row(p + "attn_block.qk.bias") if at.bias_qkv else None, precision=self.attn_core)
        da1 = ops.conv2d(dqk, at.qk, self.buf(B, H * Fq, 1, T), transpose=True, res=dv.view(B, H * Fq, 1, T), rbeta=1.0)
        da0 = ops.conv2d(da1.view(B, H, Fq, T), at.proj_in, self.buf(B, N, Fq, T), transpose=True)
        if pg is not None:                                   # a0 = z * scale2 (no GELU), a1 = proj_in(a0); da0, da1 are unscaled
            aoff = at.film_off[0]
            ops.gn_param_grad_nogelu(z, da0, stats, at.gamma, self._film(st.film, aoff, N), pg.row(p + "norm2.gamma"),
                                     pg.dfilm[:, aoff:aoff + N])
            a0 = ops.scale_channels(z, scale, self.scratch("a", B * N * Fq * T).view(B, N, Fq, T))
            self._wg(pg, p + "attn_block.proj_in.weight", a0, da1.view(B, H, Fq, T), at.proj_in, 1.0, precision="f32")
        ops.gn_bwd_nogelu(z, da0, gz, scale, stats, gz, RS2 * c)
        st.attn[blk.idx] = None
        return gz

    # ------------------------------------------------------------------ training: parameter gradients
    def _wg(self, pg, key, x, g, pc, alpha, x2=None, dil=1, fenc=None, precision=None, **kw):
        """pg.row(key) <- per-row weight gradient of conv `pc` (input cat(x, x2), output gradient alpha * oscale * g), in the
        step's weight-gradient precision pg.wgrad ('f32' | 'bf16') unless `precision` names one (the attention branch: fp32).
        fenc: the encoding table of a folded init-block conv, whose rows have the parameter's [N, 66] layout: the 2 signal
        columns from the ordinary per-row weight gradient on Cin = 2 (into scratch, then a small strided copy), the 64 encoding
        columns from ops.fenc_wgrad_rows; both always in fp32."""
        prec = "f32" if fenc is not None else (precision or pg.wgrad)
        ws = self.scratch("wg", ops.conv_wgrad_workspace(x, g, pc.KH, pc.KW, dil, x2, prec))
        rows = pg.row(key)
        if fenc is None:
            assert rows.shape[1] == pc.Cout * pc.Cin * pc.KH * pc.KW, key
            return ops.conv_wgrad_rows(x, g, pc.KH, pc.KW, rows, dil=dil, x2=x2, alpha=alpha, ws=ws, precision=prec, **kw)
        assert x2 is None and dil == 1 and not kw and (pc.Cin, pc.KH, pc.KW) == (2, 1, 1) and rows.shape[1] == pc.Cout * 66, key
        B = g.shape[0]
        sig = self.scratch("wg2", B * pc.Cout * 2).view(B, pc.Cout * 2)
        ops.conv_wgrad_rows(x, g, 1, 1, sig, alpha=alpha, ws=ws)
        ops.copy_cols(sig, rows, 2, 66, 2)
        ops.fenc_wgrad_rows(g, fenc, rows, alpha)

    def _layer_wgrad(self, pg, blk, d, G, c):
        """Dilation layer d, znew = rs2*(gate*H(a) + z), a = gelu(z*scale) recomputed into the "a" scratch (the transposed conv
        overwrites it with da next): H's weight gradient and the gate gradient, for the output gradient c*G."""
        z, stats, scale, gate = self._state.saved[blk.idx][d]
        B, N, Fq, T = z.shape
        a = self.scratch("a", B * N * Fq * T).view(B, N, Fq, T)
        ops.scale_gelu(z, scale, a)
        goff = blk.film_off[d][1]
        self._wg(pg, blk.p + f"H.{d}.weight", a, G, blk.H[d], c * RS2, dil=blk.dil(d), oscale=gate, w=blk.Hw[d],
                 dgate=pg.dfilm[:, goff:goff + N], galpha=c * RS2)

    def _layer_gn_grad(self, pg, blk, d, da, c):
        """gamma / affine gradients of layer d from da = (dL/da)/c, the transposed conv's output."""
        st = self._state
        z, stats, scale, gate = st.saved[blk.idx][d]
        N = blk.N
        aoff = blk.film_off[d][0]
        ops.gn_param_grad(z, da, scale, stats, blk.gamma[d], self._film(st.film, aoff, N), pg.row(blk.p + f"norm.{d}.gamma"),
                          pg.dfilm[:, aoff:aoff + N], cs=c)

    def _block_out_wgrad(self, pg, blk, g_out):
        """res_conv / proj_out weight gradients (both see rs2*g_out): before the VJP consumes g_out."""
        x, x2 = self._state.inp[blk.idx]
        if blk.res_conv is not None:
            self._wg(pg, blk.p + "res_conv.weight", x, g_out, blk.res_conv, RS2, x2=x2, fenc=blk.fenc)
        if blk.proj_out is not None:
            self._wg(pg, blk.p + "proj_out.weight", self._state.zpo[blk.idx], g_out, blk.proj_out, RS2)

    def param_grads(self, pg, emb_keep):
        """After the (joined) reverse sweep: {state_dict key: gradient} of every trainable parameter.  One fixed-order sum over
        the batch rows of pg.rows, then the FiLM Linear and embedding-MLP backward from pg.dfilm (emb_keep: embed(keep=))."""
        flat = ops.rows_sum(pg.rows, self.buf(self.grad_numel))
        grads = {}
        for key, (off, shape) in self.grad_layout.items():
            n = 1
            for v in shape:
                n *= v
            grads[key] = flat[off:off + n].view(shape)
        # the qk weight gradients: one launch per block over all batch rows.  Their GEMM follows the step's weight-gradient
        # arithmetic on a bf16 attention core only; on the fp32 core it stays fp32 whatever pg.wgrad says
        qk_prec = "bf16" if self.attn_core == "bf16" and pg.wgrad == "bf16" else "f32"
        for blk, _ in self.attn_blocks:
            dqk, a1 = pg.qk[blk.p]
            HF = a1.shape[1]
            grads[blk.p + "attn_block.qk.weight"] = ops.attn_qk_wgrad(dqk, a1, self.buf(2 * HF, HF, 1), precision=qk_prec)
        h0, h1, h2, h3 = emb_keep
        B = h3.shape[0]
        fi = self.film_idx
        dWcat, dbcat = self.buf(fi.J, h3.shape[1]), self.buf(fi.J)
        dh = self.buf(B, h3.shape[1])
        ops.linear_bwd(pg.dfilm, h3, fi.Wcat, dWcat, dbcat, dx=dh)
        for key, off, n in fi.keys:
            grads[key + ".weight"] = dWcat[off:off + n]
            grads[key + ".bias"] = dbcat[off:off + n]
        hs = [h0, h1, h2, h3]
        for i in (2, 1, 0):
            W, _ = self.emb_W[i]
            dW, db = self.buf(*W.shape), self.buf(W.shape[0])
            dx = self.buf(B, W.shape[1]) if i > 0 else None
            ops.linear_bwd(dh, hs[i], W, dW, db, dx=dx, y=hs[i + 1])
            grads[f"embedding.MLP.{i}.weight"], grads[f"embedding.MLP.{i}.bias"] = dW, db
            dh = dx
        return grads

    def _layer_vjp(self, blk, d, g, da, out, c, pg, merge=None):
        """Dilation layer d backwards: out <- gradient / c w.r.t. the layer's input, given g = gradient / c w.r.t. its output (the
        chain is linear, the scalar c rides along; out may be g).  da: scratch the transposed conv writes.  With pg the layer's
        parameter gradients as well.  merge: ops.gn_bwd's, the tail of an N -> N block."""
        z, stats, scale, gate = self._state.saved[blk.idx][d]
        if pg is not None:
            self._layer_wgrad(pg, blk, d, g, c)
        fs = ops.conv2d(g, blk.H[d], da, dil=blk.dil(d), transpose=True, in_scale=gate, alpha=RS2, vjp_stat=(z, scale, blk.N // 8))
        if pg is not None:
            self._layer_gn_grad(pg, blk, d, da, c)
        return ops.gn_bwd(z, da, g, scale, stats, out, RS2, merge=merge, fused=fs)

    def _block_done(self, blk):
        st = self._state
        st.saved[blk.idx] = st.inp[blk.idx] = st.zpo[blk.idx] = None

    def block_vjp(self, blk, g_out, g_in, accumulate=False, consume=False, pg=None):
        """g_in (+)= VJP of the block w.r.t. its (concatenated) input. g_out: [B,Cout,F,T] (may be strided).
        consume=True: g_out is a dense buffer owned by the caller that may be overwritten (saves a full copy).
        pg: ParamGrads of a training step (the block's parameter gradients go to its rows), None otherwise."""
        B, _, Fq, T = g_out.shape
        N = blk.N
        beta = 1.0 if accumulate else 0.0
        if pg is not None:
            self._block_out_wgrad(pg, blk, g_out)
        if (blk.res_conv is None and blk.proj_out is None and blk.proj_in is None and not accumulate and blk.nd > 0
                and g_out.is_contiguous() and FORMS.axpby2 and blk.attn is None):
            # N -> N block (every main block of the encoder, the middle block): the residual path's RS2*g_out and the main path's
            # c*gz are merged in ONE pass at the end (12 instead of 8 + 12 bytes per element).  For that g_out has to survive the
            # chain: the first layer's gn_bwd reads it as its residual input and writes into a buffer of its own (same traffic),
            # the later layers update that buffer in place.  Same arithmetic, same rounding as the two-pass form.
            gz = self.buf(B, N, Fq, T) if blk.nd > 1 else None
            da = self.scratch("a", B * N * Fq * T).view(B, N, Fq, T)
            src = g_out
            merged = g_in.is_contiguous() and FORMS.merge_tail
            for d in reversed(range(blk.nd)):            # src is the output gradient / rs2 throughout this chain
                if d == 0 and merged:
                    # the last layer's VJP pass writes g_in = RS2*g_out + RS2*gz itself (gz is never stored)
                    self._layer_vjp(blk, d, src, da, g_in, RS2, pg, merge=(g_out, RS2, RS2))
                else:
                    if gz is None:
                        gz = self.buf(B, N, Fq, T)
                    src = self._layer_vjp(blk, d, src, da, gz, RS2, pg)
            if not merged:
                ops.axpby2(g_out, gz, g_in, RS2, RS2)
            self._block_done(blk)
            return g_in
        # residual path
        if blk.res_conv is not None:
            ops.conv2d(g_out, blk.res_conv, g_in, transpose=True, alpha=RS2, rbeta=beta, res=g_in if accumulate else None)
        else:
            ops.axpby(g_out, g_in, alpha=RS2, beta=beta)
        # main path: gradient w.r.t. z_last.  The chain below is linear in gz, so the 1/sqrt2 of the block's
        # output merge is carried as a scalar `c` and applied once at the end instead of scaling a copy.
        c = 1.0
        if blk.proj_out is not None:
            gz = ops.conv2d(g_out, blk.proj_out, self.buf(B, N, Fq, T), transpose=True, alpha=RS2)
        elif consume and g_out.is_contiguous():
            gz, c = g_out, RS2
        else:
            gz = ops.axpby(g_out, self.buf(B, N, Fq, T), alpha=RS2)
        da = self.scratch("a", B * N * Fq * T).view(B, N, Fq, T)
        for d in reversed(range(blk.nd)):
            self._layer_vjp(blk, d, gz, da, gz, c, pg)
        if blk.attn is not None:
            self.attn_vjp(blk, gz, c, pg)
            c = 1.0
        if pg is not None and blk.proj_in is not None:
            x, x2 = self._state.inp[blk.idx]
            self._wg(pg, blk.p + "proj_in.weight", x, gz, blk.proj_in, c, x2=x2, fenc=blk.fenc)
        if blk.proj_in is not None:
            ops.conv2d(gz, blk.proj_in, g_in, transpose=True, res=g_in, alpha=c, rbeta=1.0)
        else:
            ops.axpby(gz, g_in, alpha=c, beta=1.0)
        self._block_done(blk)
        return g_in

    # ------------------------------------------------------------------ forward
    def c_plan(self, attention=False):
        """The library-side plan over this engine's packed weights (networks/unet_c.py), made on first use.  Every handle and
        every library-side state - the BABE_UNET_C path's and testing/eval_c.py's - shares this one.
        attention=True: the opt-in for an engine with time-attention layers, whose plan carries its _Attn objects and attn_core;
        without it such an engine raises (the Python routing, _c_engine, never asks for one)."""
        return self._plan.get(self, attention=attention)

    def _c_engine(self):
        """The library-side sequencer of this handle's state (its own library-side state and workspace over c_plan()), or None:
        fp32 without attention only, BABE_UNET_C=0 switches it off, the measurement hook's per-launch events work with either."""
        if not FORMS.unet_c or self.precision != "f32" or self.has_attention:
            return None
        st = self._state
        if st.cunet is None:
            st.cunet = CUnet(self)
        return st.cunet

    def forward(self, C_list, film, train=False):
        """C_list[j]: planar [B,2,bpo,T_j], index 0 = lowest octave. Returns same structure.
        train=True: also keep what the parameter gradients need (vjp(pg=...)); always on this Python sequencer."""
        st = self._state
        st.train = bool(train)
        st.film = film if train else None
        cu = None if train else self._c_engine()
        st.c_fwd = cu is not None
        if cu is not None:
            return cu.fwd([c.contiguous() for c in C_list], film)
        n, bpo, Ns = self.nocts, self.bpo, self.Ns
        B = C_list[0].shape[0]
        Ts = [C_list[n - 1 - i].shape[-1] for i in range(n)]      # level i time length
        st.Ts, st.B = Ts, B
        hs, pyrs = [], []
        XC = self.buf(B, Ns[0], bpo, Ts[0])
        for i in range(n):
            C = C_list[n - 1 - i]
            Fi = bpo * (i + 1)
            self.block_fwd(self.init_blk[i], C, film, XC[:, :, :bpo, :])
            # pyramid side path
            if i == 0:
                pyr = ops.resample(C, self.buf(B, 2, bpo, Ts[0] // 2), 0)
            elif i < n - 1:
                pyr_new = self.buf(B, 2, Fi, Ts[i] // 2)
                ops.resample(C, pyr_new[:, :, :bpo, :], 0)
                ops.resample(pyrs[-1], pyr_new[:, :, bpo:, :], 0)
                pyr = pyr_new
            else:
                pyr_new = self.buf(B, 2, Fi, Ts[i])
                ops.axpby(C, pyr_new[:, :, :bpo, :])
                ops.axpby(pyrs[-1], pyr_new[:, :, bpo:, :])
                pyr = pyr_new
            pyrs.append(pyr)
            if train:
                st.pyrs = pyrs
            H = self.block_fwd(self.main_blk[i], XC, film, self.buf(B, Ns[i], Fi, Ts[i]))
            hs.append(H)
            if i < n - 1:
                XCn = self.buf(B, Ns[i], Fi + bpo, Ts[i + 1])
                sub = XCn[:, :, bpo:, :]
                ops.resample(H, sub, 0)
                ops.conv2d(pyr, self.pyr_conv[i], sub, res=sub, alpha=RS2, rbeta=RS2)
                XC = XCn
            else:
                X = ops.conv2d(pyr, self.pyr_conv[i], self.buf(B, Ns[i], Fi, Ts[i]), res=H, alpha=RS2, rbeta=RS2)
        st.hs = hs
        X = self.block_fwd(self.mid_blk, X, film, self.buf(*X.shape))
        Xout = self.block_fwd(self.mid_out, X, film, self.buf(B, 2, bpo * n, Ts[-1]))
        outs = [None] * n
        for i in range(n):
            j = n - 1 - i
            Fj = bpo * (j + 1)
            Nout = Ns[max(j - 1, 0)]
            R = self.block_fwd(self.up_blk[i], X, film, self.buf(B, Nout, Fj, Ts[j]), x2=hs[j])
            O = self.block_fwd(self.up_out[i], R, film, self.buf(B, 2, Fj, Ts[j]), fold=Xout)
            if O is not Xout:                                     # (the fused head has added itself into Xout)
                ops.axpby(O, Xout, alpha=RS2, beta=RS2)           # Xout <- (Xout + O)/sqrt2
            outs[i] = ops.axpby(Xout[:, :, :bpo, :], self.buf(B, 2, bpo, Ts[j]))
            if j > 0:
                X = ops.resample(R[:, :, bpo:, :], self.buf(B, Nout, Fj - bpo, Ts[j - 1]), 1)
                Xout = ops.resample(Xout[:, :, bpo:, :], self.buf(B, 2, Fj - bpo, Ts[j - 1]), 1)
        return outs

    # ------------------------------------------------------------------ input-VJP
    def vjp(self, gouts, pg=None):
        """gouts[i]: gradient w.r.t. outs[i] (index 0 = lowest octave). Returns gradients w.r.t. C_list.
        pg: ParamGrads (rows of this call's batch items) after a forward(train=True): also every conv / GroupNorm parameter
        gradient and the FiLM output gradient."""
        st = self._state
        assert pg is None or st.train, "parameter gradients need forward(..., train=True)"
        if st.c_fwd:
            return st.cunet.vjp([g.contiguous() for g in gouts])
        n, bpo, Ns, Ts, B = self.nocts, self.bpo, self.Ns, st.Ts, st.B
        gH = [None] * n
        gX_prev = gXO_prev = None          # gradients w.r.t. X_{j-1}, XO_{j-1} (outputs of the up-samplers)
        for j in range(n):                  # reverse of the decoder order (which ran j = n-1 .. 0)
            i = n - 1 - j
            Fj = bpo * (j + 1)
            Nout = Ns[max(j - 1, 0)]
            gXOp = self.buf(B, 2, Fj, Ts[j])
            ops.axpby(gouts[i], gXOp[:, :, :bpo, :])
            gR = self.buf(B, Nout, Fj, Ts[j])
            if j > 0:
                ops.resample(gXO_prev, gXOp[:, :, bpo:, :], 3)
                gR[:, :, :bpo, :].zero_()
                ops.resample(gX_prev, gR[:, :, bpo:, :], 3)
                accumulate = True
            else:
                accumulate = False
            # O_j = up_out(R_j) entered Xout as rs2*O_j
            gO = ops.axpby(gXOp, self.buf(B, 2, Fj, Ts[j]), alpha=RS2)
            self.block_vjp(self.up_out[i], gO, gR, accumulate=accumulate, consume=True, pg=pg)
            gXO_prev = ops.axpby(gXOp, self.buf(B, 2, Fj, Ts[j]), alpha=RS2)
            gcat = self.buf(B, 2 * Ns[j], Fj, Ts[j])
            self.block_vjp(self.up_blk[i], gR, gcat, consume=True, pg=pg)
            gX_prev = gcat[:, :Ns[j]]
            gH[j] = gcat[:, Ns[j]:]
        # middle: Xout_6 = mid_out(M); X_6 = M
        gM = self.buf(B, Ns[-1], bpo * n, Ts[-1])
        ops.axpby(gX_prev, gM)
        self.block_vjp(self.mid_out, gXO_prev, gM, accumulate=True, consume=True, pg=pg)
        gXm = self.block_vjp(self.mid_blk, gM, self.buf(*gM.shape), consume=True, pg=pg)
        # encoder
        gC = [None] * n
        gpyr_next = None                   # gradient flowing into pyr_i from level i+1
        gP = None
        for i in reversed(range(n)):
            Fi = bpo * (i + 1)
            if pg is not None:                 # pyramid conv: its output entered as rs2 * pconv(pyr)
                self._wg(pg, f"downs.{i}.1.weight", st.pyrs[i], gXm if i == n - 1 else gP, self.pyr_conv[i], RS2)
            if i == n - 1:
                gHi = ops.axpby2(gH[i], gXm, self.buf(B, Ns[i], Fi, Ts[i]), 1.0, RS2)
                gpyr = ops.conv2d(gXm, self.pyr_conv[i], self.buf(B, 2, Fi, Ts[i]), transpose=True, alpha=RS2)
            else:
                # P_i = (down(H_i) + pconv_i(pyr_i)) * rs2 lives in XC_{i+1}[:, :, bpo:, :]
                gHi = ops.resample(gP, self.buf(B, Ns[i], Fi, Ts[i]), 2, alpha=RS2, beta=1.0, res=gH[i])   # g_skip + rs2 down^T(g_P), one pass
                gpyr = self.buf(B, 2, Fi, Ts[i] // 2)
                ops.conv2d(gP, self.pyr_conv[i], gpyr, transpose=True, alpha=RS2,
                           res=gpyr_next if gpyr_next is not None else None, rbeta=1.0 if gpyr_next is not None else 0.0)
            Nin = Ns[max(i - 1, 0)]
            gXC = self.block_vjp(self.main_blk[i], gHi, self.buf(B, Nin, Fi, Ts[i]), consume=True, pg=pg)
            gCi = self.buf(B, 2, bpo, Ts[i])
            self.block_vjp(self.init_blk[i], gXC[:, :, :bpo, :], gCi, pg=pg)
            gP = gXC[:, :, bpo:, :] if i > 0 else None
            # pyramid
            if i == n - 1:
                ops.axpby(gpyr[:, :, :bpo, :], gCi, beta=1.0)
                gpyr_next = gpyr[:, :, bpo:, :]
            elif i > 0:
                ops.resample(gpyr[:, :, :bpo, :], gCi, 2, beta=1.0)
                gpyr_next = ops.resample(gpyr[:, :, bpo:, :], self.buf(B, 2, Fi - bpo, Ts[i]), 2)
            else:
                ops.resample(gpyr, gCi, 2, beta=1.0)
            gC[n - 1 - i] = gCi
        st.hs = None
        if pg is not None:
            st.pyrs = st.film = None
            st.train = False
        return gC
