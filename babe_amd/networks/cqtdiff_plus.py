"""CQTDiff+ denoiser (HIP-backed), drop-in for the reference's
``networks.cqtdiff+.Unet_CQT_oct_with_attention`` (/root/reference/networks/cqtdiff+.py:583-845).

Same constructor ``(args, device)``, same ``state_dict`` key names / shapes so the
reference's checkpoints load with ``load_state_dict(state['ema'])``; ``net(x[B,L], cnoise[B,1]) ->
[B,L]``; ``net.CQTransform.apply_hpf_DC``.  The forward is autograd-transparent w.r.t. ``x`` (a
``torch.autograd.Function`` whose backward is the hand-wired HIP input-VJP), so the reference's own
sampler code - which calls ``torch.autograd.grad`` through the model - runs on it unchanged.
There is no CPU path: device must be a GPU and libbabe_hip.so must be present.

Time-attention layers (``attention_layers`` / ``attention_dict``, TimeAttentionBlock) run on the Python sequencer, in fp32
(csrc/attention.hip) unless ``attention_precision`` opts in: 'f32' keeps the fp32 core inside a network of any precision, 'bf16'
runs it on bf16 MFMA (csrc/attention_bf16.hip); without the option precision 'bf16' / 'bf16x3' refuse them.  Their parameter
gradients are opt-in: on the fp32 core ``set_trainable(True, attention=True)`` (csrc/attention_train.hip); a network on the bf16 core trains under the explicit
``set_trainable(True, attention='bf16')``: table gradient from the bf16 core's own P (babe_attn_param_vjp_bf16), qk weight gradient
on fp32 MFMA or, with ``wgrad='bf16'``, on bf16 MFMA (babe_attn_qk_wgrad_bf16), at bf16 bars instead of the reference's 2e-4.

Frequency encodings (``use_fencoding``, AddFreqEncodingRFF) are never materialised as channels: the 64 encoding channels are
constant over batch and time and feed only the init blocks' two (1,1) convs, so their share is folded into a bias table per conv
and octave that the conv kernel adds in its epilogue (csrc/fenc.hip).  ``freq_encodings.{i}.RFF_freq`` and
``.embeddings`` are non-trainable parameters under the reference's names; the loaded ``embeddings`` is what the network uses.
Not implemented: ``use_norm=False``.
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn

from ..cqt import CQT_nsgt
from .unet_engine import UnetEngine


def attention_options(attention_dict):
    """(num_heads, bias_qkv, use_rel_pos, num_buckets, max_distance) of a reference attention_dict (its defaults where absent)."""
    d = attention_dict or {}
    g = (lambda k, v: d.get(k, v)) if hasattr(d, "get") else (lambda k, v: getattr(d, k, v))
    return (int(g("num_heads", 8)), bool(g("bias_qkv", False)), bool(g("use_rel_pos", True)), int(g("rel_pos_num_buckets", 32)),
            int(g("rel_pos_max_distance", 64)))


N_FREQ_ENCODING = 32                     # RFF frequencies per octave (networks/cqtdiff+.py:627): 64 sin / cos encoding channels


ATTENTION_PRECISIONS = (None, "f32", "bf16")


def check_attention_precision(v):
    """The attention core's arithmetic: None (fp32; a bf16 / bf16x3 network refuses attention layers), 'f32' or 'bf16'."""
    if v not in ATTENTION_PRECISIONS:
        raise ValueError(f"attention_precision must be None, 'f32' or 'bf16', got {v!r}")
    return v


def freq_embedding(rff_freq, f_dim):
    """AddFreqEncodingRFF.build_RFF_embedding: [1, 2N, f_dim] = sin | cos of (2 pi n) * freq, every step in float32 as in the
    reference (the arguments reach 1e4, so the order of the roundings is part of the result)."""
    n = torch.arange(0, f_dim).unsqueeze(0).unsqueeze(0)
    table = (2 * np.pi * n) * rff_freq.float().unsqueeze(-1)
    return torch.cat([torch.sin(table), torch.cos(table)], dim=1)


def param_specs(Ns, num_dils, emb_dim=256, num_octs=7, attention_layers=None, attention_dict=None, bins_per_oct=64,
                use_fencoding=False):
    """[(key, shape, init)] for every parameter/buffer of the reference module, init in {'w','gate','ones','rff','buf','randn',
    'femb'}.  use_fencoding: the per-octave freq_encodings.{i} tables (after the embedding MLP, as in the reference's
    named_parameters) and 66-input-channel init blocks.
    attention_layers: one flag per octave plus the bottleneck (reference ResnetBlock attention_dict); the attention keys of a
    block come after all of its other keys, so an attention-off net has exactly the keys (and init order) it always had."""
    att = list(attention_layers or [0] * (num_octs + 1))
    heads, bias_qkv, rel_pos, nbk, _ = attention_options(attention_dict)
    out = [("embedding.RFF_freq", (1, 32), "rff")]
    for i, (o, k) in enumerate([(128, 64), (256, 128), (emb_dim, 256)]):
        out += [(f"embedding.MLP.{i}.weight", (o, k), "w"), (f"embedding.MLP.{i}.bias", (o,), "zero")]
    if use_fencoding:
        for i in range(num_octs):
            out += [(f"freq_encodings.{i}.RFF_freq", (1, N_FREQ_ENCODING), "rff"),
                    (f"freq_encodings.{i}.embeddings", (1, 2 * N_FREQ_ENCODING, bins_per_oct), "femb")]
    nin = 2 + 2 * N_FREQ_ENCODING if use_fencoding else 2
    out += [("downsamplerT.kernel", (8,), "buf"), ("upsamplerT.kernel", (8,), "buf")]

    def block(p, dim, dim_out, nd, k, after, Fdim=0):
        N = dim if after else dim_out
        r = []
        if after and N != dim_out:
            r.append((p + "proj_out.weight", (dim_out, N, 1, 1), "w"))
        if dim != dim_out:
            r.append((p + "res_conv.weight", (dim_out, dim, 1, 1), "w"))
        if dim != N:
            r.append((p + "proj_in.weight", (N, dim, 1, 1), "w"))
        for d in range(nd):
            r += [(p + f"norm.{d}.gamma", (1, N, 1, 1), "ones"),
                  (p + f"affine.{d}.weight", (N, emb_dim), "w"), (p + f"affine.{d}.bias", (N,), "zero"),
                  (p + f"gate.{d}.weight", (N, emb_dim), "gate"), (p + f"gate.{d}.bias", (N,), "zero"),
                  (p + f"H.{d}.weight", (N, N, k[0], k[1]), "w")]
        if Fdim:
            hF = heads * Fdim
            r += [(p + "norm2.gamma", (1, N, 1, 1), "ones"),
                  (p + "affine2.weight", (N, emb_dim), "w"), (p + "affine2.bias", (N,), "zero"),
                  (p + "gate2.weight", (N, emb_dim), "gate"), (p + "gate2.bias", (N,), "zero"),
                  (p + "attn_block.qk.weight", (2 * hF, hF, 1), "w")]
            if bias_qkv:
                r.append((p + "attn_block.qk.bias", (2 * hF,), "zero"))
            r += [(p + "attn_block.proj_in.weight", (heads, N, 1, 1), "w"), (p + "attn_block.proj_out.weight", (N, heads, 1, 1), "w")]
            if rel_pos:
                r.append((p + "attn_block.rel_pos.relative_attention_bias.weight", (nbk, heads), "randn"))
        return r

    for i in range(num_octs):
        din, dout = (Ns[0], Ns[0]) if i == 0 else (Ns[i - 1], Ns[i])
        out += block(f"downs.{i}.0.", nin, din, 1, (1, 1), False)
        out.append((f"downs.{i}.1.weight", (dout, 2, 5, 3), "w"))
        out += block(f"downs.{i}.2.", din, dout, num_dils[i], (5, 3), False, (i + 1) * bins_per_oct if att[i] else 0)
    out += block("middle.0.0.", Ns[-1], 2, 1, (1, 1), True)
    out += block("middle.0.1.", Ns[-1], Ns[-1], num_dils[-1], (5, 3), False, num_octs * bins_per_oct if att[-1] else 0)
    for ii, i in enumerate(range(num_octs - 1, -1, -1)):
        din, dout = (Ns[0] * 2, Ns[0]) if i == 0 else (Ns[i] * 2, Ns[i - 1])
        out += block(f"ups.{ii}.0.", dout, 2, 1, (1, 1), True)
        out += block(f"ups.{ii}.1.", din, dout, num_dils[i], (5, 3), False, (i + 1) * bins_per_oct if att[i] else 0)
    return out


CUBIC = [-0.01171875, -0.03515625, 0.11328125, 0.43359375, 0.43359375, 0.11328125, -0.03515625, -0.01171875]


def init_state_dict(Ns, num_dils, emb_dim=256, seed=0, gate_scale=1e-7, attention_layers=None, attention_dict=None,
                    use_fencoding=False):
    """Random weights with the reference's init rule (kaiming_uniform * sqrt(1/3); gates * 1e-7, cqtdiff+.py:599-600).
    gate_scale=1 gives O(1) gates (an untrained net with 1e-7 gates has numerically dead residual branches).
    Attention layers (param_specs) draw after everything else of their block; the relative-position tables are N(0,1)
    (nn.Embedding)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape, kind in param_specs(Ns, num_dils, emb_dim, attention_layers=attention_layers, attention_dict=attention_dict,
                                        use_fencoding=use_fencoding):
        if kind in ("w", "gate"):
            fan_in = int(np.prod(shape[1:]))
            w = math.sqrt(3.0 / fan_in) * (torch.rand(shape, generator=g) * 2 - 1)
            sd[key] = w * (math.sqrt(1 / 3) if kind == "w" else gate_scale)
        elif kind == "zero":
            sd[key] = torch.zeros(shape)
        elif kind == "ones":
            sd[key] = torch.ones(shape)
        elif kind == "rff":
            sd[key] = 16 * torch.randn(shape, generator=g)
        elif kind == "randn":
            sd[key] = torch.randn(shape, generator=g)
        elif kind == "femb":                  # built from the RFF_freq drawn just before it, by the reference's formula
            sd[key] = freq_embedding(sd[key[:-len("embeddings")] + "RFF_freq"], shape[2])
        else:
            sd[key] = torch.tensor(CUBIC)
    return sd


# The reference trains every parameter except embedding.RFF_freq (requires_grad=False, networks/cqtdiff+.py:176) and the frequency
# encodings' RFF_freq / embeddings (:222-228); the resampler kernels are buffers.
NOT_TRAINABLE = ("embedding.RFF_freq",)


def is_trainable(key):
    """True for the parameters the reference's optimizer updates."""
    return key not in NOT_TRAINABLE and not key.startswith("freq_encodings.")


class _Node(nn.Module):
    """Anonymous container so that parameter paths reproduce the reference's dotted names."""


def _attach(root, key, tensor, is_buffer):
    parts = key.split(".")
    node = root
    for p in parts[:-1]:
        if p not in node._modules:
            node.add_module(p, _Node())
        node = node._modules[p]
    if is_buffer:
        node.register_buffer(parts[-1], tensor)
    else:
        node.register_parameter(parts[-1], nn.Parameter(tensor, requires_grad=False))


class _UnetFn(torch.autograd.Function):
    """net(x, cnoise) with the hand-wired HIP backward.  Extra inputs: the parameters that require grad (net._grad_keys order);
    their gradients are formed only if autograd asks for one of them."""

    @staticmethod
    def forward(ctx, x, cnoise, net, *params):
        ctx.net = net
        ctx.train = any(ctx.needs_input_grad[3:])
        if ctx.train:
            ctx.keys = net._grad_keys
        return net.fwd_nograd(x, cnoise, train=ctx.train)

    @staticmethod
    def backward(ctx, g):
        if not ctx.train:
            return ctx.net.vjp(g.contiguous()), None, None
        gx, grads = ctx.net._vjp_train(g.contiguous())
        return (gx if ctx.needs_input_grad[0] else None, None, None) + tuple(grads[k] for k in ctx.keys)


class Unet_CQT_oct_with_attention(nn.Module):
    def __init__(self, args, device, precision=None, attention_precision=None):
        super().__init__()
        self.args = args
        nw = args.network
        # conv arithmetic: 'f32' (default, the parity path), 'bf16x3', 'bf16' (csrc/conv_bf16.hip); can also be
        # given as args.network.precision
        self.precision = precision or nw.get("precision", "f32")
        # the attention core's arithmetic, whatever the network's: None (fp32, and a network of another precision refuses attention
        # layers), 'f32' (csrc/attention.hip) or 'bf16' (csrc/attention_bf16.hip); also args.network.attention_precision.  Does
        # nothing on a network without attention layers
        self.attention_precision = check_attention_precision(
            attention_precision if attention_precision is not None else nw.get("attention_precision", None))
        self.use_fencoding = bool(nw.get("use_fencoding", False))
        self.attention_layers = [int(bool(v)) for v in (nw.get("attention_layers", None) or [0] * 8)]
        self.attention_dict = nw.get("attention_dict", None) if any(self.attention_layers) else None
        if any(self.attention_layers):
            if len(self.attention_layers) != 8:
                raise ValueError(f"attention_layers needs one flag per octave plus the bottleneck (8), got {self.attention_layers}")
            if self.precision != "f32" and self.attention_precision is None:
                raise NotImplementedError(f"attention layers run in fp32 only (precision={self.precision!r}) unless "
                                          "attention_precision ('f32' | 'bf16') opts in")
        if not nw.get("use_norm", True):
            raise NotImplementedError("use_norm=False")
        self.Ns, self.num_dils = list(nw.Ns), list(nw.num_dils)
        self.num_octs, self.bins_per_oct = nw.cqt.num_octs, nw.cqt.bins_per_oct
        assert self.num_octs == 7 and len(self.Ns) == 7
        self.emb_dim = nw.emb_dim
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("babe_amd networks run on the GPU only (no CPU fallback); use device='cuda'")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        win = ("kaiser", nw.cqt.beta) if nw.cqt.window == "kaiser" else nw.cqt.window
        self.CQTransform = CQT_nsgt(self.num_octs, self.bins_per_oct, mode="oct", window=win,
                                    fs=args.exp.sample_rate, audio_len=args.exp.audio_len, device=self.device)
        if self.use_fencoding and self.bins_per_oct != 64:
            raise NotImplementedError(f"use_fencoding needs 64 bins per octave (got {self.bins_per_oct}): csrc/fenc.hip")
        for key, t in init_state_dict(self.Ns, self.num_dils, self.emb_dim, attention_layers=self.attention_layers,
                                      attention_dict=self.attention_dict, use_fencoding=self.use_fencoding).items():
            _attach(self, key, t.to(self.device), is_buffer=key.endswith(".kernel"))
        self._train_attention = False         # set_trainable(True, attention=True)
        self._wgrad = None                    # set_trainable(True, wgrad=...): conv weight-gradient arithmetic (None: 'f32')
        self._grad_keys = None                # keys of the parameters handed to _UnetFn by the last training forward
        self.register_load_state_dict_post_hook(lambda m, k: m._reset_params())
        self._reset_params()

    def _reset_params(self):
        """Drop the engine, with every state over it, and re-read the Parameter objects (load_state_dict(assign=True) and _apply
        may replace them): the version check and the parameters handed to autograd are always the module's current ones."""
        self._engine = None
        self._lanes = None                    # [(stream, engine state)] of the lane=None evaluations (_get_lanes)
        self._lane_engines = None             # engine states of the lane=k evaluations (lane_engine)
        self._train_keep = None               # the embedding MLP's activations between a training forward and its backward
        self._params = list(self.named_parameters())
        self._versions = None

    @property
    def has_attention(self):
        """True if any ResnetBlock carries a time-attention layer (the library-side sequencers do not support those)."""
        return any(self.attention_layers)

    # ---------------------------------------------------------------- engine
    def _engine_sd(self):
        return {k: v.detach().to(self.device, torch.float32).contiguous() for k, v in self.state_dict().items()}

    def engine(self):
        if self._engine is None:
            sd = self._engine_sd()
            self._engine = UnetEngine(sd, self.Ns, self.num_dils, self.num_octs, self.bins_per_oct, self.precision,
                                      attention_layers=self.attention_layers, attention_dict=self.attention_dict,
                                      attention_precision=self.attention_precision)
            self._engine.wgrad = self._wgrad or "f32"
            self._versions = self._param_versions()
        return self._engine

    def _param_versions(self):
        return tuple(p._version for _, p in self._params)

    def _refresh_weights(self):
        """The engine packs the weights once; a parameter changed in place since then (optimizer.step(), a no_grad copy_)
        shows as a new _version: repack every conv IN PLACE (every engine state and the library-side plan share those objects) and
        rebuild the concatenated FiLM matrix.  Costs nothing on the GPU while the parameters stay as they are."""
        if self._engine is None:
            return
        v = self._param_versions()
        if v != self._versions:
            self._engine.refresh(self._engine_sd())
            self._versions = v

    # ---------------------------------------------------------------- training
    def set_trainable(self, flag=True, attention=False, wgrad=None):
        """requires_grad on exactly the reference's trainable set (is_trainable), so torch.optim.Adam(net.parameters()) updates
        what the reference's Adam updates.  Parameter gradients run in fp32, under the plain and the A-weighted EDM loss alike
        (diff_params/edm.py::loss_fn).
        attention=True opts in to the parameter gradients of the time-attention branch (norm2 / affine2 / gate2 and attn_block.*,
        csrc/attention_train.hip); without it a network with attention layers raises on the forward while a parameter requires
        grad.  The opt-in is about memory: a qk weight is a [16 F, 8 F] matrix per attention block (25.7 M floats at F = 448), and
        the attention_layers [0,0,0,0,1,1,1,1] layout carries about 141 M of them - weights, gradients and the two Adam moments
        come to about 2 GB on top of the attention-free network.  On a network without attention layers the flag does nothing.
        A network whose attention core runs in bf16 (attention_precision='bf16') refuses attention=True, which promises gradients
        that hold the reference's 2e-4 bar.  attention='bf16' is the opt-in for such a network (and raises on an fp32 core): the
        forward and input-VJP of the training step are the sampler's, bit for bit; the relative-position table gradient comes
        from the same bf16 P (babe_attn_param_vjp_bf16), the qk-bias gradient from the bf16 core's dqk, the qk weight gradient
        from babe_attn_qk_wgrad, or from babe_attn_qk_wgrad_bf16 under wgrad='bf16'; norm2 / affine2 / gate2 and proj_in /
        proj_out stay fp32.  The gradients then carry the bf16 bars (tests/attention_bf16_train_cases.py), not 2e-4.
        wgrad: arithmetic of the UNet body's conv weight gradients (H.*, res_conv, proj_in / proj_out, the pyramid convs): None,
        'f32' or 'bf16'.  'bf16' is mixed-precision training: both operands rounded once to bf16, fp32 accumulation, fp32 master
        weights and gradients (babe_conv_wgrad_bf16_rows).  The signal columns of a folded frequency-encoding conv, the
        encoding columns, the attention branch (but for the qk weight gradient of a bf16 core under attention='bf16') and the
        GroupNorm / FiLM / Linear reductions stay in fp32.  None means 'f32' on a
        precision='f32' network (bit for bit what it always was); a precision='bf16' / 'bf16x3' network keeps refusing parameter
        gradients unless wgrad is given: then its forward and input-VJP run on its own conv kernels and the weight gradients
        on the kernel named here, from the fp32 activations the forward saved."""
        if wgrad not in (None, "f32", "bf16"):
            raise ValueError(f"set_trainable: wgrad must be None, 'f32' or 'bf16', got {wgrad!r}")
        if not isinstance(attention, bool) and not (isinstance(attention, str) and attention == "bf16"):
            raise ValueError(f"set_trainable: attention must be False, True or 'bf16', got {attention!r}")
        if flag and attention is True and self.bf16_attention:
            raise NotImplementedError("set_trainable(True, attention=True): the attention branch's parameter gradients need the "
                                      "fp32 attention core; this network was built with attention_precision='bf16' "
                                      "(opt in with attention='bf16')")
        if flag and attention == "bf16" and self.has_attention and not self.bf16_attention:
            raise NotImplementedError("set_trainable(True, attention='bf16') is for a network whose attention core runs in bf16 "
                                      "(attention_precision='bf16'); on the fp32 core use attention=True")
        self._train_attention = bool(flag) and bool(attention)
        self._wgrad = wgrad if flag else None
        eng = getattr(self, "_engine", None)
        if eng is not None:
            eng.wgrad = self._wgrad or "f32"
        for k, p in self.named_parameters():
            p.requires_grad_(bool(flag) and is_trainable(k))
        return self

    def _grad_params(self):
        """[(key, parameter)] that require grad, in named_parameters order; raises where parameter gradients are not built."""
        ps = [(k, p) for k, p in self._params if p.requires_grad]
        if not ps:
            return ps
        if self.has_attention and not self._train_attention:
            raise NotImplementedError("parameter gradients of networks with attention layers are not implemented "
                                      "(opt in with set_trainable(True, attention=True))")
        if self.precision != "f32" and self._wgrad is None:
            raise NotImplementedError(f"parameter gradients run in fp32 only (precision={self.precision!r}); opt in with "
                                      "set_trainable(True, wgrad='f32' | 'bf16')")
        bad = [k for k, _ in ps if not is_trainable(k)]
        if bad:
            raise NotImplementedError(f"{bad} is not trainable (fixed in the reference); use set_trainable()")
        return ps

    # Batch items are independent, so they run on separate HIP streams (one engine state each, shared packed weights):
    # the HBM-bound passes of one item (GroupNorm / GELU / resampling, (1,1) convs) then overlap the MFMA-bound (5,3)
    # convolutions of another, and the 1.75-round grids of the 7x64-bin layers interleave.  BABE_UNET_STREAMS=1 keeps
    # everything on the caller's stream.
    MAX_LANES = int(os.environ.get("BABE_UNET_STREAMS", "2"))

    def _get_lanes(self, B):
        n = min(B, self.MAX_LANES) if self.concurrent_lanes_ok else 1      # (bf16: one stream if BABE_BF16_LANES=0)
        if n <= 1:
            return None
        if self._lanes is None or len(self._lanes) != n:
            eng = self.engine()
            self._lanes = [(torch.cuda.Stream(device=self.device), eng if i == 0 else eng.clone_state()) for i in range(n)]
        return self._lanes

    def _run_lanes(self, B, fn):
        """fn(engine, b0, b1) -> list of tensors for batch rows [b0, b1); rows are dealt to the lanes in contiguous blocks.
        Returns the per-lane results after making the caller's stream wait for every lane."""
        lanes = self._get_lanes(B)
        main = torch.cuda.current_stream(self.device)
        ready = torch.cuda.Event()
        ready.record(main)
        per = -(-B // len(lanes))
        results = []
        for i, (st, eng) in enumerate(lanes):
            b0, b1 = i * per, min(B, (i + 1) * per)
            if b0 >= b1:
                continue
            with torch.cuda.stream(st):
                st.wait_event(ready)
                out = fn(eng, b0, b1)
                for t in out:
                    t.record_stream(main)              # consumed on the caller's stream after the join below
                done = torch.cuda.Event()
                done.record(st)
            results.append((out, done))
        for _, done in results:
            main.wait_event(done)
        return [r for r, _ in results]

    def _run(self, fn, tensors, eng=None):
        """fn(engine state, tensors, b0, b1) -> list of tensors, for all batch rows of `tensors`.  eng: the state to run on, on the
        caller's stream (a lane=k evaluation).  None: the module's own stream lanes, each with its rows [b0, b1) of every tensor,
        the results concatenated; with one lane the engine itself on the caller's stream."""
        B = tensors[0].shape[0]
        if eng is not None or self._get_lanes(B) is None:
            return fn(self.engine() if eng is None else eng, tensors, 0, B)
        parts = self._run_lanes(B, lambda e, b0, b1: fn(e, [t[b0:b1] for t in tensors], b0, b1))
        return [torch.cat([p[j] for p in parts], 0) for j in range(len(parts[0]))]

    def _apply(self, fn, *a, **k):
        self._engine = None
        out = super()._apply(fn, *a, **k)
        self._reset_params()
        return out

    # ---------------------------------------------------------------- raw (no autograd) interface
    supports_lanes = True
    # precision='bf16' and clip lanes.  Kernels that contain the packed-fp32 form v_pk_{mul,add,fma}_f32 ... op_sel:[0,1] read the
    # HIGH word of their second source as 0 while another kernel's waves execute bf16 MFMA on the same CU (reduced in round 4:
    # tools/erratum/pk_opsel_min.hip, DESIGN.md "Co-residency finding").  THIS library contains no packed-fp32 instruction
    # (babe_amd/build.py, tests/test_no_packed_fp32.py), but what ELSE runs beside conv_bf16p is outside its control: PyTorch's own
    # kernels (device-side noise: bench.py's noise_device='cuda'), RCCL, a second process on the same GPU (two ranks on one
    # device), a host application's hipcc-default kernels.  So a bf16 network keeps its batch items on ONE stream by default;
    # BABE_BF16_LANES=1 opts in to two clip lanes (measured +13 %, profiles/r04_bench_bf16_two_lanes.json) for a host that knows
    # what else it launches - and even then a live torch.distributed process group or device-side noise falls back to one
    # stream (BlindSampler asks lanes_ok_for()).  The fp32 network has no bf16 MFMA anywhere and always runs two lanes.
    # The same holds for a network of any conv precision whose attention core runs on bf16 MFMA (attention_precision='bf16').
    @property
    def bf16_attention(self):
        """True if this network launches the bf16 attention core (csrc/attention_bf16.hip)."""
        return self.has_attention and self.attention_precision == "bf16"

    @property
    def runs_bf16_mfma(self):
        """True if any kernel of this network executes bf16 MFMA with single-split operands: the lane rule's condition."""
        return self.precision == "bf16" or self.bf16_attention

    @property
    def concurrent_lanes_ok(self):
        return not self.runs_bf16_mfma or os.environ.get("BABE_BF16_LANES", "0") == "1"

    def lanes_ok_for(self, noise_device="cpu"):
        """concurrent_lanes_ok narrowed by what the CALLER will launch beside the lanes: with precision='bf16' two lanes also
        need host-side noise (torch.randn on the device is an ATen kernel inside the lane loop) and no live process group."""
        if not self.runs_bf16_mfma:
            return True
        if not self.concurrent_lanes_ok:
            return False
        import torch.distributed as dist
        return str(noise_device) == "cpu" and not (dist.is_available() and dist.is_initialized())

    def lane_engine(self, lane):
        """Engine state number `lane` (saved activations + scratch of its own over the shared packed weights): a caller that
        pipelines independent clips on its own streams (BlindSampler) passes lane=k to fwd_nograd / vjp, which then run
        entirely on the CALLER's current stream with that state instead of forking streams themselves.  Also the entry of the
        library-side evaluation (testing/eval_c.py), so the weight refresh runs here too."""
        self._refresh_weights()
        eng = self.engine()
        if self._lane_engines is None:
            self._lane_engines = [eng]
        while len(self._lane_engines) <= lane:
            self._lane_engines.append(eng.clone_state())
        return self._lane_engines[lane]

    def fwd_nograd(self, x, cnoise, lane=None, train=False):
        """x [B,L], cnoise [B,1] -> [B,L]; keeps what vjp() needs until the next call (of the same lane).
        train=True: also what the parameter gradients need (_vjp_train); fp32, the module's own lanes."""
        assert x.device == self.device, f"input on {x.device}, network on {self.device}"
        assert lane is None or not train
        with torch.cuda.device(self.device):       # every launch below goes to THIS device's current stream
            if lane is None:
                self._refresh_weights()            # (the lane path refreshes in lane_engine)
            state = None if lane is None else self.lane_engine(lane)
            eng = self.engine() if state is None else state
            x = x.detach().contiguous().float()
            assert x.shape[-1] == self.CQTransform.Ls, "input length must equal exp.audio_len (the CQT is built for it)"
            keep = [] if train else None
            film = eng.embed(cnoise.detach().reshape(-1, 1).contiguous().float(), keep=keep)
            co = self.CQTransform.fwd_planar(x)
            if train:
                self._train_keep = keep
            outs = self._run(lambda e, t, b0, b1: e.forward(t[:-1], t[-1], train=train), list(co) + [film], state)
            return self.CQTransform.bwd_planar(outs)

    def vjp(self, g, lane=None):
        """Gradient of <net(x), g> w.r.t. x for the last fwd_nograd call (of the same lane)."""
        assert g.device == self.device, f"gradient on {g.device}, network on {self.device}"
        return self._vjp(g, lane)[0]

    def _vjp_train(self, g):
        """(gradient w.r.t. x, {key: gradient of every parameter}) of <net(x), g> for the last fwd_nograd(train=True)."""
        return self._vjp(g, train=True)

    def _vjp(self, g, lane=None, train=False):
        from .unet_engine import ParamGrads
        with torch.cuda.device(self.device):
            state = None if lane is None else self.lane_engine(lane)
            eng = self.engine()
            # training: the buffers the lanes write their rows of, made on the caller's stream before the lanes fork
            pg = ParamGrads.new(eng, g.shape[0]) if train else None
            gouts = self.CQTransform.bwd_adjoint(g.contiguous())
            gC = self._run(lambda e, t, b0, b1: e.vjp(t, pg=pg.lane(b0, b1) if train else None), list(gouts), state)
            gx = self.CQTransform.fwd_adjoint(gC)
            if not train:
                return gx, None
            grads = eng.param_grads(pg, self._train_keep)
            self._train_keep = None
            return gx, grads

    # ---------------------------------------------------------------- nn.Module call
    def forward(self, inputs, sigma):
        if torch.is_grad_enabled():
            ps = self._grad_params()
            if ps:
                self._grad_keys = [k for k, _ in ps]
                return _UnetFn.apply(inputs, sigma, self, *[p for _, p in ps])
            if inputs.requires_grad:
                return _UnetFn.apply(inputs, sigma, self)
        return self.fwd_nograd(inputs, sigma)
