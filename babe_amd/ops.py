"""Python views of the babe_hip C-ABI ops (UNet building blocks).  Device tensors only."""
import ctypes as C
import functools
import math

import torch

from . import _lib
from ._cabi import IMAGE_SLOTS, ConvArgs, CPackedConv, PackedConvLayout, PwArgs, WgradArgs
from .forms import FORMS
from ._lib import check, lib, ptr, stream

RSQRT2 = 1.0 / math.sqrt(2.0)


def _view(t):
    """(ptr, batch stride, channel stride) of a [B,C,F,T] tensor whose rows are contiguous."""
    assert t.dim() == 4 and t.dtype == torch.float32
    assert t.stride(3) == 1 and t.stride(2) == t.shape[3], f"rows must be contiguous, got strides {t.stride()}"
    return ptr(t), t.stride(0), t.stride(1)


def _fill_out(a, pc, out, Cin, dil, res, oscale, alpha, rbeta):
    """The output side of a ConvArgs - out, residual, output scale, alpha / rbeta - and the problem's shape."""
    B, Cout, F, T = out.shape
    a.out, a.out_bs, a.out_cs = _view(out)
    if res is not None:
        assert res.shape == out.shape
        a.res, a.res_bs, a.res_cs = _view(res)
    else:
        a.res, a.res_bs, a.res_cs = None, 0, 0
    if oscale is not None:
        assert oscale.is_contiguous() and oscale.shape == (B, Cout)
    a.oscale = ptr(oscale)
    a.alpha, a.rbeta = alpha, rbeta
    a.B, a.Cin, a.Cout, a.F, a.T = B, Cin, Cout, F, T
    a.KH, a.KW, a.dil = pc.KH, pc.KW, dil


PRECISIONS = {"f32": 0, "bf16": 1, "bf16x3": 2}


# bit i of babe_packed_conv_plan's form mask (BABE_CONV_FORM_* of include/babe_hip.h): the attribute of FORMS that switches it
_FORM_BITS = ("winograd", "winograd4", "winograd45", "winograd85", "fewco")


_DESC_FIELDS = frozenset(k for k, _ in CPackedConv._fields_)


class PackedConv:
    """Conv2d weights packed for babe_conv2d, forward and input-VJP (flipped/transposed) versions.
    precision: 'f32' (exact fp32 MFMA), 'bf16' or 'bf16x3' (bf16 MFMA, see csrc/conv_bf16.hip).
    `desc` is the C descriptor (babe_packed_conv) babe_conv2d_auto picks the kernel from: every shape and image attribute is
    written through to it, so assigning None to an image after construction takes its kernel out of the dispatch.
    Which images exist, how large each is, nt and whether the raw weights are kept is the library's rule (babe_packed_conv_plan,
    include/babe_hip.h).  The forms it is asked with (forms.py: the Winograd families and fewco as its mask, conv11_nt for nt,
    bf16_hbm_f32 for splits_for) are read when the object is CONSTRUCTED: selecting another form later does not repack it."""

    def __init__(self, w, precision="f32", nt=0):
        """nt: row tiles (x32 output channels) per workgroup of the direct kernel, 0 = default (include/babe_hip.h)."""
        assert w.is_cuda and w.dtype == torch.float32 and w.dim() == 4
        w = w.contiguous()
        self.desc = CPackedConv()
        self.precision = precision
        self.Cout, self.Cin, self.KH, self.KW = w.shape
        lay = PackedConvLayout()
        forms = sum(1 << i for i, name in enumerate(_FORM_BITS) if getattr(FORMS, name))
        check(lib().babe_packed_conv_plan(*w.shape, self.splits_for(w.shape, precision), nt, FORMS.conv11_nt, forms, C.byref(lay)),
              "packed_conv_plan")
        self.nt, self.splits = lay.nt, lay.splits
        dtype, size = (torch.int16, 2) if lay.splits else (torch.float32, 4)
        for name, nbytes in zip(IMAGE_SLOTS, lay.bytes):
            setattr(self, name, torch.empty(nbytes // size, device=w.device, dtype=dtype) if nbytes else None)
        # raw weights for the few-output-channel kernel (the input-VJP of a 2..4-input-channel conv, csrc/conv_fewco.hip): the
        # caller's tensor itself
        self.w_raw = w if lay.raw else None
        self.repack(w)

    @staticmethod
    def splits_for(shape, precision):
        """bf16 products per multiply a conv of this weight shape runs with under `precision`; 0 = the fp32 kernels.  The
        library's rule (babe_conv_splits_for, csrc/conv_auto.hip: which shapes stay fp32 whatever the precision), asked with this
        process's bf16_hbm_f32 form."""
        splits = lib().babe_conv_splits_for(int(shape[0]), int(shape[1]), int(shape[2]), int(shape[3]), PRECISIONS[precision],
                                            int(bool(FORMS.bf16_hbm_f32)))
        if splits < 0:
            raise _lib.BabeHipError("conv_splits_for: " + lib().babe_last_error().decode())
        return splits

    def __setattr__(self, k, v):
        object.__setattr__(self, k, v)
        if k in _DESC_FIELDS:
            setattr(self.desc, k, ptr(v) if torch.is_tensor(v) else v)

    def repack(self, w):
        """Pack new weights of the same shape IN PLACE into the existing images, so that every pointer to them (this `desc`, the
        descriptors of the library-side plan, engine states sharing this object) stays valid: the refresh after an optimizer
        step.  Construction packs through this function too, so the images are exactly those a freshly built PackedConv holds."""
        assert w.is_cuda and w.dtype == torch.float32 and tuple(w.shape) == (self.Cout, self.Cin, self.KH, self.KW)
        w = w.contiguous()
        if self.w_raw is not None and self.w_raw.data_ptr() != w.data_ptr():
            self.w_raw.copy_(w)
        check(lib().babe_packed_conv_pack(C.byref(self.desc), ptr(w), stream()), "packed_conv_pack")


def conv2d(x, pc, out, *, dil=1, transpose=False, x2=None, res=None, in_scale=None, oscale=None, alpha=1.0, rbeta=0.0,
           force_nested=False, force_f45=False, vjp_stat=None, fwd_stat=None, fbias=None):
    """out = alpha*conv(x[,x2]; W)*oscale + rbeta*res   (transpose=True: input-VJP weights), on the kernel the library picks
    from pc.desc (babe_conv2d_auto).
    fbias [Cout, F]: out = alpha*oscale*(conv + fbias[co, f]) + rbeta*res, the folded frequency encodings (fp32 (1,1) kernels; any
    other kernel raises).
    force_nested: take the nested-Winograd F(2,5) x F(4,3) kernel whenever it CAN run the problem (tests), not only when it is
    preferred; force_f45: the same for the F(4,5) x F(4,3) kernel.
    vjp_stat=(z, scale, cg): if the launch takes the F(4,5) kernel, its epilogue also forms the partial sums of the GroupNorm /
    FiLM / GELU input-VJP for the gradient `out` it writes (z: the layer's saved input, dense like out; scale [B,C]; cg channels
    per group) and (part, S) is RETURNED for gn_bwd(part=, S=); otherwise None is returned and gn_bwd runs its own pass.
    fwd_stat=cg: likewise the sums of the output itself - the next layer's GroupNorm partial sums - for gn_scale_gelu(fused=);
    (part, S) or None is returned.  Either only under its form (FORMS.fuse_gn / FORMS.fuse_gn_fwd, forms.py)."""
    a = ConvArgs()
    B, C1, F, T = x.shape
    Cin = pc.Cout if transpose else pc.Cin
    Cout = pc.Cin if transpose else pc.Cout
    a.in_, a.in_bs, a.in_cs = _view(x)
    if x2 is not None:
        assert x2.shape[0] == B and x2.shape[2:] == x.shape[2:]
        a.in2, a.in2_bs, a.in2_cs = _view(x2)
        a.cin_split = C1
        assert C1 + x2.shape[1] == Cin
    else:
        a.in2, a.in2_bs, a.in2_cs, a.cin_split = None, 0, 0, Cin
        assert C1 == Cin, (C1, Cin)
    wq = pc.bwd if transpose else pc.fwd
    a.w_packed = None if pc.splits else ptr(wq)
    assert out.shape == (B, Cout, F, T), (out.shape, (B, Cout, F, T))
    _fill_out(a, pc, out, Cin, dil, res, oscale, alpha, rbeta)
    if in_scale is not None:
        assert in_scale.is_contiguous() and in_scale.shape == (B, Cin)
    a.in_scale = ptr(in_scale)
    if fbias is not None:
        assert fbias.is_contiguous() and fbias.dtype == torch.float32 and fbias.shape == (Cout, F)
        a.fbias = ptr(fbias)
    L = lib()
    w85 = getattr(pc, "bwd_wino85" if transpose else "fwd_wino85", None)
    f45 = w85 is not None and x2 is None and not force_nested         # the F(4,5) kernel may run: it alone fuses the sums
    if f45 and vjp_stat is not None and FORMS.fuse_gn:
        z, scale, cg = vjp_stat
        assert z.is_contiguous() and out.is_contiguous() and z.shape == out.shape and scale.is_contiguous()
        a.stat_mode, a.stat_cg, a.stat_x, a.stat_scale = 2, cg, ptr(z), ptr(scale)
    elif f45 and fwd_stat is not None and FORMS.fuse_gn_fwd and out.is_contiguous():
        a.stat_mode, a.stat_cg = 1, fwd_stat
    if a.stat_mode:                                                     # (mode 1: two sums per slot, mode 2: one)
        S = L.babe_conv2d_wino85_stat_slots(C.byref(a))
        part = torch.empty(B * (Cout // a.stat_cg) * S * (3 - a.stat_mode), device=x.device, dtype=torch.float64)
        a.stat_part = ptr(part)
    w45 = getattr(pc, "bwd_wino45" if transpose else "fwd_wino45", None)
    if force_nested and w45 is not None and L.babe_conv2d_wino45_supported(C.byref(a)):
        check(L.babe_conv2d_wino45(C.byref(a), ptr(w45), stream()), "conv2d_wino45")
    elif force_f45 and f45 and L.babe_conv2d_wino85_supported(C.byref(a)):
        check(L.babe_conv2d_wino85(C.byref(a), ptr(w85), stream()), "conv2d_wino85")
    else:
        desc = pc.desc
        if force_nested:                                                # a forced nested conv never takes the F(4,5) kernel
            desc = CPackedConv.from_buffer_copy(desc)
            desc.fwd_wino85 = desc.bwd_wino85 = None
        check(L.babe_conv2d_auto(C.byref(a), C.byref(desc), int(transpose), stream()), "conv2d_auto")
    if vjp_stat is None and fwd_stat is None:
        return out
    return (part, S) if a.stat_mode else None


@functools.lru_cache(maxsize=None)
def _splits(n):
    """Split count of a GroupNorm group of n elements: the library's rule (babe_gn_splits), cached - this is on the per-launch
    path and a network has a handful of group sizes."""
    return int(lib().babe_gn_splits(int(n)))


def _gn_buffers(x, G, fused=None, vjp=False):
    """(n, S, part, stats, scale) of a GroupNorm pass over x [B,C,F,T]: the group size, the split count, the float64 partial sums
    (S pairs per group; S values for the VJP) and, for the forward, new stats [B,G,3] and scale [B,C].  fused=(part, S): the
    partial sums a conv already formed."""
    B, Cc, F, T = x.shape
    n = (Cc // G) * F * T
    if fused is not None:
        part, S = fused
    else:
        S = _splits(n)
        part = torch.empty(B * G * S * (1 if vjp else 2), device=x.device, dtype=torch.float64)
    if vjp:
        return n, S, part, None, None
    stats = torch.empty(B, G, 3, device=x.device, dtype=torch.float32)
    scale = torch.empty(B, Cc, device=x.device, dtype=torch.float32)
    return n, S, part, stats, scale


_GN_TICKETS = {}


def _gn_ticket(dev, n):
    """Zero-initialised ticket buffer of the fused statistics kernel, one per (device, current stream): calls on different
    streams may run concurrently and must not share tickets; every call leaves its tickets at zero."""
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream)
    t = _GN_TICKETS.get(key)
    if t is None or t.numel() < n:
        t = torch.zeros(max(n, 1024), device=dev, dtype=torch.int32)
        _GN_TICKETS[key] = t
    return t


def gn_scale(x, gamma, film, G=8, eps=1e-7):
    """Returns (stats [B,G,3], scale [B,C]) with scale = gamma*(film+1)/(std+eps).  x dense [B,C,F,T].
    Two launches (partial sums, finalize); BABE_GN_FUSED=1 = one launch (csrc/norm.hip gn_partial_kernel<true>: the last
    workgroup of a group finalises it; bit-identical, measured slower on the whole job - see gn_fused in forms.py)."""
    assert x.is_contiguous()
    B, Cc, F, T = x.shape
    n, S, part, stats, scale = _gn_buffers(x, G)
    L = lib()
    assert film.stride(1) == 1
    if FORMS.gn_fused:
        check(L.babe_gn_stats(ptr(x), ptr(part), ptr(_gn_ticket(x.device, B * G)), ptr(gamma), ptr(film), film.stride(0),
                              ptr(stats), ptr(scale), B, Cc, G, n, S, eps, stream()), "gn_stats")
        return stats, scale
    check(L.babe_gn_partial(ptr(x), ptr(part), B, G, n, S, stream()), "gn_partial")
    check(L.babe_gn_finalize(ptr(part), ptr(gamma), ptr(film), film.stride(0), ptr(stats), ptr(scale), B, Cc, G, n, S,
                             eps, stream()), "gn_finalize")
    return stats, scale


def gn_scale_gelu(x, gamma, film, out, G=8, eps=1e-7, fused=None):
    """gn_scale + scale_gelu with the finalize folded into the GELU kernel's prologue: out = gelu(x * scale); returns
    (stats [B,G,3], scale [B,C]) for the VJP.  Bit-identical to gn_scale followed by scale_gelu (BABE_GELU_FIN=0).
    fused=(part, S): the partial sums of x already formed by the conv that wrote it (conv2d(fwd_stat=)): no pass over x for them."""
    if fused is None and not FORMS.gelu_fin:
        stats, scale = gn_scale(x, gamma, film, G, eps)
        scale_gelu(x, scale, out)
        return stats, scale
    assert x.is_contiguous() and out.is_contiguous() and out.shape == x.shape and film.stride(1) == 1
    B, Cc, F, T = x.shape
    n, S, part, stats, scale = _gn_buffers(x, G, fused)
    L = lib()
    if fused is None:
        check(L.babe_gn_partial(ptr(x), ptr(part), B, G, n, S, stream()), "gn_partial")
    check(L.babe_scale_gelu_fin(ptr(x), ptr(part), ptr(gamma), ptr(film), film.stride(0), ptr(stats), ptr(scale), ptr(out),
                                B, Cc, G, F * T, S, eps, stream()), "scale_gelu_fin")
    return stats, scale


def pw_block_enable(on):
    """Sets the library's switch of the fused (1,1) ResnetBlock passes (BABE_PW_BLOCK); returns the previous value."""
    return bool(lib().babe_pw_block_enable(int(bool(on))))


def pw_block_fwd(cblk, z, film, gate, out, x=None, add=None, train=False, precision="f32", G=8):
    """A k = (1,1) ResnetBlock forward as one fused pass (csrc/pw_block.hip) if the library's rule takes it
    (babe_pw_block_supported: the one statement of that rule): babe_gn_partial over z, then the pass.  Returns (stats, scale) as
    gn_scale_gelu does, or None - nothing launched - when the block has to run layer by layer.
    cblk: the block's babe_unet_block; z [B,N,F,T] the GroupNorm input; film [B,J] the FiLM rows; gate [B,N] contiguous;
    out: the head's 2-channel or the init block's N-channel output view; x: the init block's 2-channel input;
    add: the head's running sum, out = RS2*(block) + RS2*add (may be out); precision: the network's (fp32 networks only)."""
    if not z.is_contiguous():
        return None
    B, N, F, T = z.shape
    n, S, part, stats, scale = _gn_buffers(z, G)
    a = PwArgs()
    a.B, a.F, a.T, a.S, a.plan_splits = B, F, T, S, PRECISIONS[precision]
    a.z, a.z_bs, a.z_cs = _view(z)
    if x is not None:
        a.x, a.x_bs, a.x_cs = _view(x)
    a.out, a.out_bs, a.out_cs = _view(out)
    if add is not None:
        a.add, a.add_bs, a.add_cs = _view(add)
    assert film.stride(1) == 1 and gate.is_contiguous() and gate.shape == (B, N)
    a.part, a.film, a.film_bs, a.gate, a.stats, a.scale = ptr(part), ptr(film), film.stride(0), ptr(gate), ptr(stats), ptr(scale)
    L = lib()
    if not L.babe_pw_block_supported(C.byref(cblk), C.byref(a), int(bool(train))):
        return None
    check(L.babe_gn_partial(ptr(z), ptr(part), B, G, n, S, stream()), "gn_partial")
    check(L.babe_pw_block_fwd(C.byref(cblk), C.byref(a), stream()), "pw_block_fwd")
    return stats, scale


def scale_gelu(x, scale, out):
    B, Cc, F, T = x.shape
    assert x.is_contiguous() and out.is_contiguous() and out.shape == x.shape
    check(lib().babe_scale_gelu(ptr(x), ptr(scale), ptr(out), B, Cc, F * T, stream()), "scale_gelu")
    return out


def units_ok(pc, Cin, Cout, T):
    """True if the forward of this (5,3) conv can take its input as bf16 units (csrc/conv_bf16p.hip, UNITS variant)."""
    assert (Cin, Cout) == (pc.Cin, pc.Cout)
    return bool(FORMS.units and lib().babe_conv2d_bf16_units_shape(C.byref(pc.desc), int(T)))


def scale_gelu_units(x, scale, au):
    """GroupNorm-scale * GELU of x [B,C,F,T], written as bf16 units into the int16 buffer `au` (>= B*units_size*8)."""
    B, Cc, F, T = x.shape
    assert x.is_contiguous() and au.dtype == torch.int16 and au.is_contiguous()
    assert au.numel() >= B * lib().babe_units_size(Cc, F, T) * 8
    check(lib().babe_scale_gelu_units(ptr(x), ptr(scale), ptr(au), B, Cc, F, T, stream()), "scale_gelu_units")
    return au


def units_args(au, pc, out, Cin, dil=1, res=None, oscale=None, alpha=1.0, rbeta=1.0):
    """ConvArgs of out = alpha * conv(units, w) * oscale + rbeta * res with the input given as bf16 units."""
    B, Cout, F, T = out.shape
    a = ConvArgs()
    nu = lib().babe_units_size(Cin, F, T)
    assert au.dtype == torch.int16 and au.numel() >= B * nu * 8, "units buffer too small for this (Cin, F, T)"
    a.in_, a.in_bs, a.in_cs = ptr(au), nu, nu // (Cin // 8)
    a.in2, a.in2_bs, a.in2_cs, a.cin_split = None, 0, 0, Cin
    a.w_packed = None
    a.in_scale = None
    _fill_out(a, pc, out, Cin, dil, res, oscale, alpha, rbeta)
    return a


def units_supported(a):
    """The library's own verdict (alignment, 2 GiB descriptor limits, BABE_CONV_BF16U): ask BEFORE writing units."""
    return bool(lib().babe_conv2d_bf16_units_supported(C.byref(a)))


def conv2d_units(au, pc, out, Cin, dil=1, res=None, oscale=None, alpha=1.0, rbeta=1.0, args=None):
    a = args if args is not None else units_args(au, pc, out, Cin, dil, res, oscale, alpha, rbeta)
    check(lib().babe_conv2d_bf16_units(C.byref(a), ptr(pc.fwd), stream()), "conv2d_bf16_units")
    return out


def gn_bwd(x, da, gy, scale, stats, gx, rbeta, G=8, eps=1e-7, merge=None, fused=None, gelu=True):
    """gx = rbeta*gy + GN/FiLM/GELU input-VJP of da (gx may alias gy; da is only read).
    merge=(acc, ca, cb): gx = ca*acc + cb*(that result) in the same pass (a block's VJP tail, babe_gn_bwd_apply_merge).
    fused=(part, S): the partial sums already formed by the conv that wrote da (conv2d(..., vjp_stat=)): no babe_gn_bwd_partial.
    gelu=False: the VJP of a = x*scale, the babe_gn_bwd_*_nogelu entry points (gn_bwd_nogelu; neither merge nor fused)."""
    B, Cc, F, T = x.shape
    assert x.is_contiguous() and da.is_contiguous() and gx.is_contiguous() and (gy is None or gy.is_contiguous())
    assert gelu or (merge is None and fused is None)
    n, S, part, _, _ = _gn_buffers(x, G, fused, vjp=True)
    L = lib()
    partial, apply = (L.babe_gn_bwd_partial, L.babe_gn_bwd_apply) if gelu else (L.babe_gn_bwd_partial_nogelu, L.babe_gn_bwd_apply_nogelu)
    if fused is None:
        check(partial(ptr(x), ptr(da), ptr(scale), ptr(part), B, Cc, G, F * T, S, stream()), "gn_bwd_partial")
    if merge is not None:
        acc, ca, cb = merge
        assert acc.is_contiguous() and acc.shape == x.shape
        check(L.babe_gn_bwd_apply_merge(ptr(x), ptr(da), ptr(gy), ptr(scale), ptr(stats), ptr(part), ptr(gx), rbeta, B, Cc, G,
                                        F * T, S, eps, stream(), ptr(acc), ca, cb), "gn_bwd_apply_merge")
        return gx
    check(apply(ptr(x), ptr(da), ptr(gy), ptr(scale), ptr(stats), ptr(part), ptr(gx), rbeta, B, Cc, G, F * T, S, eps, stream()),
          "gn_bwd_apply")
    return gx


def resample(x, out, mode, alpha=1.0, beta=0.0, res=None):
    """mode 0 down, 1 up, 2 down^T, 3 up^T. T argument is the forward op's input length.
    out = alpha*R(x) + beta*out, or with res: out = alpha*R(x) + beta*res (one pass; unaligned views: copy, then accumulate)."""
    B, Cc, F, Tin = x.shape
    T = {0: Tin, 1: Tin, 2: Tin * 2, 3: Tin // 2}[mode]
    Tout = {0: T // 2, 1: 2 * T, 2: T, 3: T}[mode]
    assert out.shape == (B, Cc, F, Tout), (out.shape, (B, Cc, F, Tout))
    xp, xbs, xcs = _view(x)
    op, obs, ocs = _view(out)
    if res is not None:
        assert res.shape == out.shape
        rp, rbs, rcs = _view(res)
        if FORMS.axpby2 and all(v % 4 == 0 for v in (rbs, rcs, obs, ocs)) and res.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0:
            check(lib().babe_resample_res(xp, xbs, xcs, rp, rbs, rcs, op, obs, ocs, B, Cc, F, T, mode, alpha, beta, stream()),
                  "resample_res")
            return out
        axpby(res, out)
    check(lib().babe_resample(xp, xbs, xcs, op, obs, ocs, B, Cc, F, T, mode, alpha, beta, stream()), "resample")
    return out


def axpby(x, out, alpha=1.0, beta=0.0):
    assert x.shape == out.shape
    B, Cc, F, T = x.shape
    xp, xbs, xcs = _view(x)
    op, obs, ocs = _view(out)
    check(lib().babe_axpby4d(xp, xbs, xcs, op, obs, ocs, B, Cc, F, T, alpha, beta, stream()), "axpby4d")
    return out


def axpby2(x, y, out, alpha, beta):
    """out = alpha*x + beta*y in one pass over [B,C,F,T] views (falls back to two axpby calls for unaligned views)."""
    assert x.shape == out.shape and y.shape == out.shape
    B, Cc, F, T = x.shape
    xp, xbs, xcs = _view(x)
    yp, ybs, ycs = _view(y)
    op, obs, ocs = _view(out)
    aligned = (F * T) % 4 == 0 and all(v % 4 == 0 for v in (xbs, xcs, ybs, ycs, obs, ocs)) and \
        all(t.data_ptr() % 16 == 0 for t in (x, y, out))
    if not (aligned and FORMS.axpby2):
        axpby(x, out, alpha=alpha)
        return axpby(y, out, alpha=beta, beta=1.0)
    check(lib().babe_axpby2_4d(xp, xbs, xcs, yp, ybs, ycs, op, obs, ocs, B, Cc, F, T, alpha, beta, stream()), "axpby2_4d")
    return out


def linear(x, W, bias, relu=False, out=None):
    B, K = x.shape
    J = W.shape[0]
    assert x.is_contiguous() and W.is_contiguous()
    if out is None:
        out = torch.empty(B, J, device=x.device, dtype=torch.float32)
    check(lib().babe_linear(ptr(x), ptr(W), ptr(bias), ptr(out), B, K, J, int(relu), stream()), "linear")
    return out


def rff(cnoise, freq):
    B = cnoise.shape[0]
    R = freq.numel()
    out = torch.empty(B, 2 * R, device=cnoise.device, dtype=torch.float32)
    check(lib().babe_rff(ptr(cnoise.contiguous()), ptr(freq.contiguous()), ptr(out), B, R, stream()), "rff")
    return out


def gn_bwd_nogelu(x, da, gy, scale, stats, gx, rbeta, G=8, eps=1e-7):
    """gx = rbeta*gy + input-VJP of a = x*scale (BiasFreeGroupNorm * FiLM, no GELU: the attention branch's norm2) for da."""
    return gn_bwd(x, da, gy, scale, stats, gx, rbeta, G, eps, gelu=False)


def attn_buckets(T, num_buckets=32, max_distance=64):
    """int32 [2T-1] host tensor: T5 bidirectional bucket of every key-minus-query offset d = -(T-1) .. T-1 (entry d + T - 1),
    bit-exact with the reference's float32 evaluation."""
    out = torch.empty(2 * T - 1, dtype=torch.int32)
    check(lib().babe_attn_buckets(C.c_void_p(out.data_ptr()), T, num_buckets, max_distance), "attn_buckets")
    return out


def attn_fwd(qk, a, out, lse, scale, qk_bias=None, bucket=None, emb=None, precision="f32"):
    """Time attention forward.  qk [B,2HF,T], a/out [B,H,F,T], lse [B,H,T], all dense; bucket int32 [2T-1] and emb [nb,H]
    (device) or both None.  precision: 'f32' (babe_attn_fwd, exact fp32 MFMA) or 'bf16' (babe_attn_fwd_bf16: operands rounded
    once to bf16, fp32 accumulation and softmax; csrc/attention_bf16.hip)."""
    B, H, F, T = a.shape
    for t in (qk, a, out, lse):
        assert t.is_contiguous() and t.dtype == torch.float32
    assert qk.numel() == B * 2 * H * F * T and out.shape == a.shape and lse.numel() == B * H * T
    nb = 0
    if bucket is not None:
        assert bucket.dtype == torch.int32 and bucket.numel() == 2 * T - 1 and emb.is_contiguous() and emb.shape[1] == H
        nb = emb.shape[0]
    args = (ptr(qk), ptr(qk_bias), ptr(a), ptr(bucket), ptr(emb), nb, ptr(out), ptr(lse), B, H, F, T, scale, stream())
    if precision == "bf16":
        check(lib().babe_attn_fwd_bf16(*args), "attn_fwd_bf16")
    else:
        assert precision == "f32", precision
        check(lib().babe_attn_fwd(*args), "attn_fwd")
    return out, lse


def attn_vjp(qk, a, out, lse, dout, dqk, dv, scale, qk_bias=None, bucket=None, emb=None, precision="f32"):
    """Input-VJP of attn_fwd for the gradient dout: writes dqk [B,2HF,T] and dv [B,H,F,T] (deterministic, no atomics).
    precision as for attn_fwd; out and lse are those the forward of the same precision wrote."""
    B, H, F, T = a.shape
    for t in (qk, a, out, lse, dout, dqk, dv):
        assert t.is_contiguous() and t.dtype == torch.float32
    assert dout.shape == a.shape and dv.shape == a.shape and dqk.numel() == qk.numel()
    nb = 0 if bucket is None else emb.shape[0]
    D = torch.empty(B, H, T, device=a.device, dtype=torch.float32)
    args = (ptr(qk), ptr(qk_bias), ptr(a), ptr(bucket), ptr(emb), nb, ptr(out), ptr(lse), ptr(dout), ptr(D), ptr(dqk), ptr(dv), B, H,
            F, T, scale, stream())
    if precision == "bf16":
        check(lib().babe_attn_vjp_bf16(*args), "attn_vjp_bf16")
    else:
        assert precision == "f32", precision
        check(lib().babe_attn_vjp(*args), "attn_vjp")
    return dqk, dv


# ---------------------------------------------------------------------------------------------------- training (csrc/wgrad.hip)
def _wgrad_args(x, g, KH, KW, dil=1, x2=None):
    B, Cout, F, T = g.shape
    xp, xbs, xcs = _view(x)
    gp, gbs, gcs = _view(g)
    a = WgradArgs()
    a.x, a.x_bs, a.x_cs = xp, xbs, xcs
    Cin = x.shape[1]
    if x2 is not None:
        a.x2, a.x2_bs, a.x2_cs = _view(x2)
        a.cin_split = x.shape[1]
        Cin += x2.shape[1]
        assert x2.shape[0] == B and x2.shape[2:] == (F, T)
    assert x.shape[0] == B and x.shape[2:] == (F, T), (x.shape, g.shape)
    a.g, a.g_bs, a.g_cs = gp, gbs, gcs
    a.B, a.Cin, a.Cout, a.F, a.T, a.KH, a.KW, a.dil = B, Cin, Cout, F, T, KH, KW, dil
    return a


WGRAD_PRECISIONS = ("f32", "bf16")


def _wgrad_fns(precision):
    """(workspace, rows) entry points of the conv weight gradient: 'f32' (fp32 MFMA) or 'bf16' (operands rounded once to bf16,
    fp32 accumulation: babe_conv_wgrad_bf16_rows)."""
    if precision not in WGRAD_PRECISIONS:
        raise ValueError(f"conv_wgrad: precision must be one of {WGRAD_PRECISIONS}, got {precision!r}")
    L = lib()
    return (L.babe_conv_wgrad_workspace, L.babe_conv_wgrad_rows) if precision == "f32" else \
        (L.babe_conv_wgrad_bf16_workspace, L.babe_conv_wgrad_bf16_rows)


def conv_wgrad_workspace(x, g, KH, KW, dil=1, x2=None, precision="f32"):
    """Floats of workspace conv_wgrad_rows needs for these operands."""
    n = _wgrad_fns(precision)[0](C.byref(_wgrad_args(x, g, KH, KW, dil, x2)))
    if n < 0:
        raise _lib.BabeHipError(f"conv_wgrad: unsupported shape x{tuple(x.shape)} g{tuple(g.shape)} k=({KH},{KW})")
    return n


def conv_wgrad_rows(x, g, KH, KW, rows, *, dil=1, x2=None, oscale=None, alpha=1.0, w=None, dgate=None, galpha=1.0, ws=None,
                    precision="f32"):
    """Per-batch-row conv weight gradient (babe_conv_wgrad_rows): rows[b] (a [B, Cout*Cin*KH*KW] view, any row stride) <-
    alpha * oscale[b, co] * sum_{f,t} g[b, co] * shifted cat(x, x2)[b, ci]; dgate[b, co] <- galpha * <w[co], that sum without
    oscale>.  x, x2, g: [B, C, F, T] views with contiguous rows (frequency sub-views allowed); ws: workspace (allocated if None).
    precision='bf16': x and g rounded once to bf16 (nearest even), fp32 accumulation, everything after the sum as in fp32
    (babe_conv_wgrad_bf16_rows)."""
    a = _wgrad_args(x, g, KH, KW, dil, x2)
    n = conv_wgrad_workspace(x, g, KH, KW, dil, x2, precision)
    if ws is None:
        ws = torch.empty(n, device=g.device, dtype=torch.float32)
    assert ws.numel() >= n and ws.is_contiguous()
    assert rows.dim() == 2 and rows.shape[0] == a.B and rows.shape[1] == a.Cout * a.Cin * KH * KW and rows.stride(1) == 1
    if oscale is not None:
        assert oscale.is_contiguous() and oscale.shape == (a.B, a.Cout)
    if dgate is not None:
        assert w is not None and w.is_contiguous() and w.numel() == a.Cout * a.Cin * KH * KW
        assert dgate.shape == (a.B, a.Cout) and dgate.stride(1) == 1
    check(_wgrad_fns(precision)[1](C.byref(a), ptr(ws), ptr(oscale), alpha, ptr(w), ptr(dgate),
                                   dgate.stride(0) if dgate is not None else 0, galpha, ptr(rows), rows.stride(0), stream()),
          "conv_wgrad_rows")
    return rows


def fenc_bias(w, emb, fb):
    """fb[co, f] <- sum_j w[co, 2 + j] * emb[j, f] (babe_fenc_bias), in place: the frequency encodings' share of a (1,1) conv over
    cat(signal, encodings) channels, as a bias per channel and frequency row.  w [Cout, 66] (row stride >= 66), emb [64, 64]."""
    assert w.dim() == 2 and w.shape[1] == 66 and w.stride(1) == 1 and w.dtype == torch.float32
    assert emb.is_contiguous() and emb.shape == (64, 64) and fb.is_contiguous() and fb.shape == (w.shape[0], 64)
    check(lib().babe_fenc_bias(ptr(w), ptr(emb), ptr(fb), w.shape[0], w.stride(0), stream()), "fenc_bias")
    return fb


def fenc_wgrad_rows(g, emb, rows, alpha=1.0):
    """rows[b, co*66 + 2 + j] <- alpha * sum_f emb[j, f] * sum_t g[b, co, f, t] (babe_fenc_wgrad_rows): the encoding columns of the
    per-row weight gradient of a folded conv; g [B, Cout, 64, T] view with contiguous rows, rows [B, Cout*66] (any row stride)."""
    B, Cout, F, T = g.shape
    gp, gbs, gcs = _view(g)
    assert emb.is_contiguous() and emb.shape == (64, 64)          # (F != 64 is the library's error)
    assert rows.dim() == 2 and rows.shape == (B, Cout * 66) and rows.stride(1) == 1
    check(lib().babe_fenc_wgrad_rows(gp, gbs, gcs, ptr(emb), alpha, ptr(rows), rows.stride(0), 66, B, Cout, F, T, stream()),
          "fenc_wgrad_rows")
    return rows


def copy_cols(src, dst, ld_src, ld_dst, n):
    """dst[b, r*ld_dst + c] <- src[b, r*ld_src + c] for c < n (babe_axpby4d on [B][rows][1][n] views): a small strided copy."""
    B = src.shape[0]
    R = src.shape[1] // ld_src
    assert src.stride(1) == 1 and dst.stride(1) == 1 and dst.shape[0] == B and dst.shape[1] == R * ld_dst
    check(lib().babe_axpby4d(ptr(src), src.stride(0), ld_src, ptr(dst), dst.stride(0), ld_dst, B, R, 1, n, 1.0, 0.0, stream()), "copy_cols")
    return dst


def rows_sum(rows, out, beta=0.0):
    """out[i] = beta*out[i] + sum_b rows[b, i] (b in increasing order: the fixed-order batch reduction of the parameter grads)."""
    B, n = rows.shape
    assert rows.stride(1) == 1 and out.is_contiguous() and out.numel() == n
    check(lib().babe_rows_sum(ptr(rows), rows.stride(0), B, n, ptr(out), beta, stream()), "rows_sum")
    return out


def gn_param_grad(z, da, scale, stats, gamma, film_aff, dgamma_rows, dfilm, cs=1.0, G=8):
    """GroupNorm * FiLM parameter gradients of a = gelu(z * scale) given da (babe_gn_param_grad): dgamma_rows[b, c] (summed over b
    later by rows_sum) and dfilm[b, c] (the gradient of the FiLM affine output); cs scales da.
    scale=None: a = z * scale without the GELU (babe_gn_param_grad_nogelu, which does not read scale)."""
    B, Cc, F, T = z.shape
    assert z.is_contiguous() and da.is_contiguous() and da.shape == z.shape
    assert film_aff.stride(1) == 1 and dgamma_rows.stride(1) == 1 and dfilm.stride(1) == 1
    assert dgamma_rows.shape == (B, Cc) and dfilm.shape == (B, Cc)
    tail = (ptr(stats), ptr(gamma), ptr(film_aff), film_aff.stride(0), cs, ptr(dgamma_rows), dgamma_rows.stride(0), ptr(dfilm),
            dfilm.stride(0), B, Cc, G, F * T, stream())
    if scale is None:
        check(lib().babe_gn_param_grad_nogelu(ptr(z), ptr(da), *tail), "gn_param_grad_nogelu")
    else:
        check(lib().babe_gn_param_grad(ptr(z), ptr(da), ptr(scale), *tail), "gn_param_grad")


def gn_param_grad_nogelu(z, da, stats, gamma, film_aff, dgamma_rows, dfilm, cs=1.0, G=8):
    """gn_param_grad for a = z * scale without the GELU (babe_gn_param_grad_nogelu: norm2 / affine2 of the attention branch)."""
    gn_param_grad(z, da, None, stats, gamma, film_aff, dgamma_rows, dfilm, cs, G)


def scale_channels(x, scale, out):
    """out = x * scale[b, c] (babe_scale_channels), dense [B,C,F,T]: scale_gelu without the GELU."""
    B, Cc, F, T = x.shape
    assert x.is_contiguous() and out.is_contiguous() and out.shape == x.shape and scale.is_contiguous() and scale.shape == (B, Cc)
    check(lib().babe_scale_channels(ptr(x), ptr(scale), ptr(out), B, Cc, F * T, stream()), "scale_channels")
    return out


def _attn_precision(who, precision):
    if precision not in ("f32", "bf16"):
        raise ValueError(f"{who}: precision must be 'f32' or 'bf16', got {precision!r}")
    return "_bf16" if precision == "bf16" else ""


def attn_qk_wgrad_workspace(B, HF, T, precision="f32"):
    """Floats of workspace attn_qk_wgrad needs at this shape (0: none; > 0: K is split into chunks); -1: unsupported shape."""
    return getattr(lib(), "babe_attn_qk_wgrad" + _attn_precision("attn_qk_wgrad_workspace", precision) + "_workspace")(B, HF, T)


def attn_qk_wgrad(dqk, a1, dW, alpha=1.0, beta=0.0, ws=None, precision="f32"):
    """dW [2HF, HF] = alpha * sum_b dqk[b] a1[b]^T + beta * dW (babe_attn_qk_wgrad): the qk Conv1d weight gradient, summed over
    the batch in a fixed order.  dqk [B,2HF,T], a1 [B,HF,T] dense.  precision: 'f32' (exact fp32 MFMA) or 'bf16'
    (babe_attn_qk_wgrad_bf16: both fp32 operands rounded once to bf16, fp32 accumulation)."""
    name = "attn_qk_wgrad" + _attn_precision("attn_qk_wgrad", precision)
    B, M, T = dqk.shape
    HF = a1.shape[1]
    for t in (dqk, a1, dW):
        assert t.is_contiguous() and t.dtype == torch.float32
    assert a1.shape == (B, HF, T) and M == 2 * HF and dW.numel() == M * HF
    n = getattr(lib(), f"babe_{name}_workspace")(B, HF, T)
    if n < 0:
        raise _lib.BabeHipError(f"{name}: unsupported shape B={B} HF={HF} T={T} (HF a multiple of 512, at most 3584)")
    if n and ws is None:
        ws = torch.empty(n, device=dW.device, dtype=torch.float32)
    assert not n or (ws.numel() >= n and ws.is_contiguous())
    check(getattr(lib(), "babe_" + name)(ptr(dqk), ptr(a1), ptr(dW), ptr(ws) if n else None, B, HF, T, alpha, beta, stream()), name)
    return dW


def attn_param_vjp(qk, a, out, lse, dout, dqk, scale, qk_bias=None, bucket=None, emb=None, demb_rows=None, dqkb_rows=None,
                   precision="f32"):
    """Table and bias gradients of attn_fwd per batch row (babe_attn_param_vjp), from the operands of attn_vjp and its dqk:
    demb_rows [B, nb*H] (with bucket / emb) and dqkb_rows [B, 2HF] (views with any row stride; None: not computed).
    precision: that of the attn_fwd / attn_vjp calls that wrote out, lse and dqk; 'bf16' is babe_attn_param_vjp_bf16, the table
    gradient of exactly the P the bf16 core's dQ pass used."""
    name = "attn_param_vjp" + _attn_precision("attn_param_vjp", precision)
    B, H, F, T = a.shape
    for t in (qk, a, out, lse, dout, dqk):
        assert t.is_contiguous() and t.dtype == torch.float32
    assert dout.shape == a.shape and dqk.numel() == qk.numel() == B * 2 * H * F * T
    nb = 0
    if bucket is not None:
        assert bucket.dtype == torch.int32 and bucket.numel() == 2 * T - 1 and emb.is_contiguous() and emb.shape[1] == H
        nb = emb.shape[0]
        assert demb_rows is not None and demb_rows.shape == (B, nb * H) and demb_rows.stride(1) == 1
    else:
        assert demb_rows is None
    if dqkb_rows is not None:
        assert dqkb_rows.shape == (B, 2 * H * F) and dqkb_rows.stride(1) == 1
    ws = torch.empty(max(1, getattr(lib(), f"babe_{name}_workspace")(B, H, T, nb)), device=a.device, dtype=torch.float32)
    check(getattr(lib(), "babe_" + name)(ptr(qk), ptr(qk_bias), ptr(a), ptr(bucket), ptr(emb), nb, ptr(out), ptr(lse), ptr(dout), ptr(dqk),
                                    ptr(ws), ptr(demb_rows), demb_rows.stride(0) if demb_rows is not None else 0, ptr(dqkb_rows),
                                    dqkb_rows.stride(0) if dqkb_rows is not None else 0, B, H, F, T, scale, stream()),
          name)


def linear_bwd(dy, x, W, dW, db, dx=None, y=None, beta=0.0, ws=None):
    """Backward of linear(x, W, bias, relu=y is not None) with output y: dW (+)= dp^T x, db (+)= sum_b dp, dx = dp W,
    dp = dy * (y > 0) (babe_linear_bwd; fixed-order sums)."""
    B, K = x.shape
    J = W.shape[0]
    assert dy.shape == (B, J) and all(t.is_contiguous() for t in (dy, x, W, dW)) and dW.shape == (J, K)
    assert db is None or (db.is_contiguous() and db.numel() == J)
    assert y is None or (y.is_contiguous() and y.shape == (B, J))
    if dx is not None:
        assert dx.is_contiguous() and dx.shape == (B, K)
        if ws is None:
            ws = torch.empty(lib().babe_linear_bwd_workspace(B, K, J), device=x.device, dtype=torch.float32)
    check(lib().babe_linear_bwd(ptr(dy), ptr(y), ptr(x), ptr(W), ptr(dW), ptr(db), ptr(dx), ptr(ws), B, K, J, beta, stream()),
          "linear_bwd")
    return dW
