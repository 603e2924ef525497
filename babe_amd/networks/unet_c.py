"""ctypes binding of the library-side UNet engine (csrc/unet_engine.hip: babe_unet_plan_* / babe_unet_fwd / babe_unet_vjp).

`CPlan` describes a `UnetEngine`'s packed weights to the library once (a plan handle, owned by the engine); a `CUnet` is one
library-side state and workspace over it, whose `fwd` / `vjp` are ONE C call per direction instead of ~1100 op-level calls from
Python.  Results are bit-identical to the Python-sequenced engine
(tests/test_gpu_unet_c.py; tests/test_gpu_bf16_library.py for a 'bf16' / 'bf16x3' engine, whose images the library sequences as
they are).  Workspace and outputs are torch allocations (the library never allocates)."""
import ctypes as C

import torch

from .._cabi import ATTN_CORES, CAttn, CBlock, CPackedConv, CPlanDesc
from .._lib import check, lib, ptr, stream, workspace


def _pc(dst, pc):
    """PackedConv -> CPackedConv: a copy of its descriptor (absent layer: Cout stays 0)."""
    if pc is not None:
        C.memmove(C.addressof(dst), C.addressof(pc.desc), C.sizeof(CPackedConv))


def fill_block(dst, b):
    """_Block -> babe_unet_block: copies of its convs' descriptors, pointers to its gammas (the images repack in place)."""
    dst.N, dst.nd, dst.k53 = b.N, b.nd, int(b.k53)
    _pc(dst.proj_in, b.proj_in)
    _pc(dst.res_conv, b.res_conv)
    _pc(dst.proj_out, b.proj_out)
    for d in range(b.nd):
        _pc(dst.H[d], b.H[d])
        dst.gamma[d] = ptr(b.gamma[d])
        dst.film_aff[d], dst.film_gate[d] = b.film_off[d]
    if b.fenc is not None:                                # folded frequency encodings: the tables are rewritten in place by refresh
        dst.fb_proj_in, dst.fb_res_conv = ptr(b.fb_proj_in), ptr(b.fb_res_conv)


def c_attn(at):
    """_Attn -> babe_unet_attn: copies of its three convs' descriptors, pointers to its gamma, qk bias and table."""
    dst = CAttn()
    dst.H, dst.F, dst.scale = at.H, at.F, at.scale
    _pc(dst.proj_in, at.proj_in)
    _pc(dst.qk, at.qk)
    _pc(dst.proj_out, at.proj_out)
    dst.gamma = ptr(at.gamma)
    dst.film_aff, dst.film_gate = at.film_off
    dst.qk_bias, dst.emb = ptr(at.qk_bias), ptr(at.emb)
    if at.emb is not None:
        dst.num_buckets, dst.max_distance = at.nbk, at.maxd
    return dst


def c_block(b):
    """A _Block as a babe_unet_block of its own: what the fused (1,1) block passes take from the Python sequencer."""
    dst = CBlock()
    fill_block(dst, b)
    return dst


class CPlan:
    """The library's description of one engine's packed weights (babe_unet_plan): immutable, made on first use, shared by every
    library-side state over that engine and destroyed with the last of them.  An engine with time-attention layers gets one only
    on request (get(eng, attention=True)): its blocks' _Attn objects as babe_unet_attn, eng.attn_core as the plan's attn_core."""

    handle = None

    def get(self, eng, attention=False):
        if self.handle is None:
            if eng.has_attention and not attention:
                raise NotImplementedError("the library-side UNet sequencer does not support time-attention layers "
                                          "(such networks run on the Python sequencer)")
            d = CPlanDesc()
            d.nocts, d.bpo = eng.nocts, eng.bpo
            attns = []                                   # (the library copies them at plan creation)
            if eng.has_attention:
                d.attn_core = ATTN_CORES[eng.attn_core]
            for i, v in enumerate(eng.Ns):
                d.Ns[i] = v
            for i in range(eng.nocts):
                fill_block(d.init_blk[i], eng.init_blk[i])
                fill_block(d.main_blk[i], eng.main_blk[i])
                fill_block(d.up_out[i], eng.up_out[i])
                fill_block(d.up_blk[i], eng.up_blk[i])
                _pc(d.pyr_conv[i], eng.pyr_conv[i])
            fill_block(d.mid_blk, eng.mid_blk)
            fill_block(d.mid_out, eng.mid_out)
            for dst, blk in [(d.main_blk[i], eng.main_blk[i]) for i in range(eng.nocts)] + [(d.mid_blk, eng.mid_blk)] + \
                    [(d.up_blk[i], eng.up_blk[i]) for i in range(eng.nocts)]:
                if blk.attn is not None:
                    attns.append(c_attn(blk.attn))
                    dst.attn = C.pointer(attns[-1])
            self.handle = lib().babe_unet_plan_create(C.byref(d))
            if not self.handle:
                raise RuntimeError("babe_unet_plan_create: " + lib().babe_last_error().decode())
            self._keep = eng                             # the plan points into the engine's weight buffers
        return self.handle

    def __del__(self):
        try:
            if self.handle:
                lib().babe_unet_plan_destroy(self.handle)
        except Exception:
            pass


class CUnet:
    """One library-side state and workspace over an engine's plan (UnetEngine.c_plan): one per engine state on the BABE_UNET_C
    path, one per lane for testing/eval_c.py.  Belongs to one stream at a time."""

    def __init__(self, eng, attention=False):
        """attention=True: also for an engine with time-attention layers (UnetEngine.c_plan(attention=True)); without it such an
        engine raises."""
        self.plan = eng.c_plan(attention=True) if attention else eng.c_plan()
        self._owner = eng._plan                          # keeps the plan alive as long as this state
        self.n = eng.nocts
        self.state = lib().babe_unet_state_create()
        self._ws = {}
        self.ws = None                                   # the workspace of the latest call

    def __del__(self):
        try:
            if getattr(self, "state", None):
                lib().babe_unet_state_destroy(self.state)
        except Exception:
            pass

    def fwd(self, C_list, film):
        L = lib()
        n = self.n
        B = C_list[0].shape[0]
        Ts = [int(c.shape[-1]) for c in C_list]
        assert all(c.is_contiguous() and c.dtype == torch.float32 for c in C_list) and film.stride(1) == 1
        T_oct = (C.c_int * n)(*Ts)
        ws = self.ws = workspace(self._ws, (B, tuple(Ts)), lambda: L.babe_unet_workspace_bytes(self.plan, B, T_oct), C_list[0].device, "unet")
        outs = [torch.empty_like(c) for c in C_list]
        cin = (C.c_void_p * n)(*[ptr(c) for c in C_list])
        cout = (C.c_void_p * n)(*[ptr(o) for o in outs])
        self._keep = (C_list, film)              # inputs are read again by nothing after the call, but keep them until the VJP
        check(L.babe_unet_fwd(self.plan, self.state, cin, ptr(film), film.stride(0), B, T_oct, ptr(ws), ws.numel(), cout,
                              stream()), "unet_fwd")
        return outs

    def vjp(self, gouts):
        L = lib()
        n = self.n
        assert all(g.is_contiguous() and g.dtype == torch.float32 for g in gouts)
        gC = [torch.empty_like(g) for g in gouts]
        gin = (C.c_void_p * n)(*[ptr(g) for g in gouts])
        gout = (C.c_void_p * n)(*[ptr(g) for g in gC])
        check(L.babe_unet_vjp(self.plan, self.state, gin, gout, stream()), "unet_vjp")
        self._keep = None
        return gC
