"""Cases, data, float64 references and per-element bounds of the conv edge tests (tests/test_conv_cases_cpu.py pins this module
on the CPU, tests/test_gpu_conv_edges.py runs the kernels).  Importing it needs no GPU.

The op (include/babe_hip.h, babe_conv_args; csrc/conv_common.h, conv_w_tap and conv_epilogue_impl), stated once:
  forward    out[b,co,f,t] = alpha * oscale[b,co] * (fbias[co,f] + sum_{ci,kh,kw} w[co,ci,kh,kw] * x[b,ci,f+(kh-KH//2)*dil, t+kw-KW//2])
                             + rbeta * res[b,co,f,t]                      (x = 0 outside [0,F) x [0,T): "same" zero padding)
  input-VJP  gx[b,ci,f,t]  = alpha * sum_{co,kh,kw} w[co,ci,kh,kw] * in_scale[b,co] * gy[b,co,f-(kh-KH//2)*dil, t-(kw-KW//2)]
                             (+ rbeta * res): the same kernels on the flipped / transposed image, in_scale on the INPUT side.
ref_loops states it as nested loops; tests/test_conv_cases_cpu.py holds the float64 torch references to it on the tiniest case.

Data regimes (all seeded by the case's name):
  integers  x, res, fbias, w integers in [-4, 4]; alpha = 0.5, rbeta = 0.25; oscale and in_scale signed powers of two from
            {+-0.5, +-1, +-2}, another row per batch item.  Then every operand is exact in bf16 (|v| <= 8 integers and halves: at most
            5 significant bits; a bf16x3 low part is zero), every product x * in_scale * w is a multiple of 1/2 of magnitude <= 32,
            every partial sum of at most Cin*KH*KW <= 3840 of them (plus fbias) is a multiple of 1/2 below 2^17, and the epilogue
            (x 0.5, x 2^k, + 0.25 * integer) stays on the grid 2^-4 below 2^18: far inside the 2^24 of an fp32 significand, in any
            summation order, fused or not.  The fp32 MFMA kernels, the vector-ALU kernel and both bf16 precisions are therefore
            EXACT, and the expectation is torch.equal against float64.  exactness_precondition asserts the premises per case.
  impulse   x = 1.0 at the eight corners of the (channel, frequency, time) box and at one interior point, everything else as in
            `integers`: the output is the weights laid down around each point, so a wrong flip or offset fails by name.
  unit      randn x, res; randn / sqrt(Cin*KH*KW) weights; oscale, in_scale randn; alpha = 0.7, rbeta = 0.3.  For the Winograd
            families, which are not exact on integers (their weight transforms divide by 6, 24, 45, 90).

Per-element bound of the Winograd families:  |got - ref| <= c * 2^-24 * A,
  A = |alpha * oscale| * conv(|x * in_scale|, |w|) + |rbeta * res|   (the same conv on magnitudes),
  c = wino_c(family, n_acc) = growth * (n_acc + n_ops), derived below from the transform matrices of the kernels' headers - never
  from what a kernel returns.  See wino_c.
"""
import math
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
NAN = float("nan")
GUARD = 64                      # floats of canary on either side of every buffer (tests/fft_cases.py)
OUT_FILL, OUT_CANARY = 7.0, -3.0

# ----------------------------------------------------------------------------- kernels, counters, rules
# kernel -> launch-counter slot (babe_prof_slot_name, csrc/misc.hip).  Two pairs share a slot; which of the pair runs is the host
# rule restated in sub_kernel below (babe_conv11p_supported, babe_conv2d_wino4p_supported: no C linkage, so not callable).
KERNEL_SLOT = {"direct53": "conv53_direct", "direct11": "conv11", "conv11p": "conv11", "fewco": "conv53_fewco", "wino2": "conv53_wino2",
               "wino4": "conv53_wino4", "wino4p": "conv53_wino4", "wino45": "conv53_wino45", "wino85": "conv53_wino85",
               "bf16": "conv_bf16", "bf16p": "conv_bf16p"}
KERNEL_SOURCE = {"direct53": "conv.hip", "direct11": "conv.hip", "conv11p": "conv11p.hip", "fewco": "conv_fewco.hip",
                 "wino2": "conv_wino.hip", "wino4": "conv_wino4.hip", "wino4p": "conv_wino4p.hip", "wino45": "conv_wino45.hip",
                 "wino85": "conv_wino85.hip", "bf16": "conv_bf16.hip", "bf16p": "conv_bf16p.hip"}
SOURCES = sorted(set(KERNEL_SOURCE.values()))
CONV_SLOTS = sorted(set(KERNEL_SLOT.values()))
WINOGRAD = ("wino2", "wino4", "wino4p", "wino45", "wino85")
# the operands each kernel's *_supported rule has a view_aligned clause for (conv.hip and conv_bf16.hip take every view: the
# direct kernel only chooses its scalar staging), and the kernel a refused call ends on at these sizes: every Winograd rule has
# the same four clauses, so one misaligned operand takes all of them out
ALIGN_CLAUSE = {"direct53": (), "direct11": (), "bf16": (), "conv11p": ("in_", "in2"), "fewco": ("in_", "out", "res"),
                "wino2": ("in_", "in2", "out", "res"), "wino4": ("in_", "in2", "out", "res"), "wino4p": ("in_", "in2", "out", "res"),
                "wino45": ("in_", "in2", "out", "res"), "wino85": ("in_", "in2", "out", "res"), "bf16p": ("out", "res")}
FALLBACK = {"conv11p": "direct11", "fewco": "direct53", "wino2": "direct53", "wino4": "direct53", "wino4p": "direct53",
            "wino45": "direct53", "wino85": "direct53", "bf16p": "bf16"}

# images taken out of a PackedConv so that the dispatch ends on the family (assigning None removes the kernel: ops.PackedConv)
_W85 = ("fwd_wino85", "bwd_wino85")
_W45 = ("fwd_wino45", "bwd_wino45")
_W4 = ("fwd_wino4", "bwd_wino4")
_W2 = ("fwd_wino", "bwd_wino")
STRIP = {"direct": _W2 + _W4 + _W45 + _W85 + ("w_raw",), "conv11": (), "fewco": _W2 + _W4 + _W45 + _W85,
         "wino2": _W4 + _W45 + _W85 + ("w_raw",), "wino4": _W45 + _W85 + ("w_raw",), "wino45": (), "wino85": (), "bf16": ()}

Case = namedtuple("Case", "name family w B F T dil fwd vjp split vsplit fbias precision note")


def _c(name, family, w, B, Fq, T, dil, fwd, vjp, split=0, vsplit=0, fbias=False, precision="f32", note=""):
    return Case(name, family, w, B, Fq, T, dil, fwd, vjp, split, vsplit, fbias, precision, note)


# w = (Cout, Cin, KH, KW).  fwd / vjp: the kernel the call must take on aligned views.  split: channels of the FIRST of two forward
# sources (0 = one source); vsplit: the same for the transposed call (gy handed over as two tensors).
CASES = [
    # ---- direct (5,3), conv.hip: 32-channel row tiles, 8-channel slabs, 128 positions per workgroup
    _c("direct-5to20-T7", "direct", (20, 5, 5, 3), 2, 3, 7, 1, "direct53", "direct53", note="scalar staging (T % 4 != 0), padded channels on both sides"),
    _c("direct-8to32-dil2", "direct", (32, 8, 5, 3), 1, 2, 16, 2, "direct53", "direct53", note="vector staging; dil >= F: every off-centre frequency tap is outside"),
    _c("direct-12+9to40", "direct", (40, 21, 5, 3), 1, 5, 20, 1, "direct53", "direct53", split=12, vsplit=17, note="source split inside an 8-channel slab, two row tiles (one padded)"),
    _c("direct-T1", "direct", (33, 9, 5, 3), 2, 4, 1, 1, "direct53", "direct53", note="T = 1: both time halos outside at every position"),
    _c("direct-F1", "direct", (16, 8, 5, 3), 1, 1, 24, 1, "direct53", "direct53", note="F = 1: only the centre row exists"),
    _c("direct-two-tiles", "direct", (8, 8, 5, 3), 1, 3, 48, 1, "direct53", "direct53", note="64-step tiles over T = 48 (ragged), 2 rows per tile over F = 3: two workgroups"),
    _c("direct-8to96", "direct", (96, 8, 5, 3), 1, 2, 16, 1, "direct53", "direct53", note="three row tiles per workgroup"),
    _c("direct-8to128", "direct", (128, 8, 5, 3), 1, 2, 16, 1, "direct53", "direct53", note="four row tiles per workgroup"),
    _c("direct-3to132", "direct", (132, 3, 5, 3), 1, 2, 8, 1, "direct53", "direct53", note="five row tiles, one per workgroup, the last with 4 channels"),
    # ---- (1,1) fp32: conv.hip below 4096 positions and 256 input channels, conv11p.hip (16-channel slabs, 128 / 256 positions) above
    _c("c11-2to64-T5", "conv11", (64, 2, 1, 1), 2, 3, 5, 1, "direct11", "direct11"),
    _c("c11-2to64-T12-fb", "conv11", (64, 2, 1, 1), 2, 3, 12, 1, "direct11", "direct11", fbias=True),
    _c("c11-72to40-T5-fb", "conv11", (40, 72, 1, 1), 2, 3, 5, 1, "direct11", "direct11", fbias=True),
    _c("c11-72to40-T12", "conv11", (40, 72, 1, 1), 2, 3, 12, 1, "direct11", "direct11"),
    _c("c11-16+16to24-T5", "conv11", (24, 32, 1, 1), 2, 3, 5, 1, "direct11", "direct11", split=16),
    _c("c11-16+16to24-T12-fb", "conv11", (24, 32, 1, 1), 2, 3, 12, 1, "direct11", "direct11", split=16, fbias=True),
    _c("c11-64to2-T5-fb", "conv11", (2, 64, 1, 1), 2, 3, 5, 1, "direct11", "direct11", fbias=True),
    _c("c11-64to2-T12", "conv11", (2, 64, 1, 1), 2, 3, 12, 1, "direct11", "direct11"),
    _c("c11-64to64-T12", "conv11", (64, 64, 1, 1), 2, 3, 12, 1, "direct11", "direct11", note="tile counts even in both directions: packed for two row tiles"),
    _c("c11p-8to40", "conv11", (40, 8, 1, 1), 2, 16, 256, 1, "conv11p", "conv11p", note="4096 positions: the pipelined kernel, half a 16-channel slab, padded row tile"),
    _c("c11p-8to40-fb", "conv11", (40, 8, 1, 1), 1, 16, 256, 1, "conv11p", "conv11p", fbias=True, note="the bias variant of the pipelined kernel"),
    _c("c11p-256+16to40", "conv11", (40, 272, 1, 1), 2, 3, 12, 1, "conv11p", "direct11", split=256, note="Cin >= 256 on 36 positions: one ragged tile, 17 slabs over two sources"),
    _c("c11p-8+16to8", "conv11", (8, 24, 1, 1), 1, 16, 256, 1, "direct11", "conv11p", split=8, note="cin_split % 16 != 0: the pipelined rule refuses the forward"),
    # ---- few output channels, conv_fewco.hip: the VJP of [N, c, 5, 3]; 256 / 32 position quads per workgroup (8 channel slices from 64 channels)
    *[_c(f"fewco-8x{c}", "fewco", (8, c, 5, 3), 2, 3, 8, 1, "direct53", "fewco", note="one slice, 6 quads") for c in (1, 2, 3, 4)],
    *[_c(f"fewco-64x{c}-dil4", "fewco", (64, c, 5, 3), 1, 2, 16, 4, "direct53", "fewco", note="8 channel slices; dil >= F") for c in (1, 2, 3, 4)],
    _c("fewco-fwd-8to2", "fewco", (2, 8, 5, 3), 2, 3, 8, 1, "fewco", "direct53", note="the forward of a conv with two output channels, full epilogue"),
    _c("fewco-fwd-64to3-dil4", "fewco", (3, 64, 5, 3), 1, 2, 16, 4, "fewco", "direct53", note="three of the four-channel form's outputs, 8 channel slices"),
    # ---- F(2,3), conv_wino.hip: 32- / 64- / 96- / 128-channel tiles x 256 / 128 positions, rows of at least 16 steps
    _c("wino2-5to20", "wino2", (20, 5, 5, 3), 2, 3, 16, 1, "wino2", "wino2", note="one padded row tile, one padded slab"),
    _c("wino2-20+12to64", "wino2", (64, 32, 5, 3), 1, 5, 20, 2, "wino2", "wino2", split=20, note="two row tiles; source split inside a slab; ragged 32-step rows"),
    _c("wino2-8to96", "wino2", (96, 8, 5, 3), 1, 3, 16, 1, "wino2", "wino2", note="three row tiles: the phase-pair kernel"),
    _c("wino2-8to128", "wino2", (128, 8, 5, 3), 1, 2, 20, 1, "wino2", "wino2", note="128 co x 128 positions"),
    # ---- F(4,3): conv_wino4p.hip wherever conv_wino4.hip's rule holds, except two sources split inside a slab
    _c("wino4p-40to40", "wino4", (40, 40, 5, 3), 2, 3, 16, 1, "wino4p", "wino4p", note="two row tiles, one padded: 64 co x 512 positions"),
    _c("wino4p-40to96", "wino4", (96, 40, 5, 3), 1, 2, 20, 2, "wino4p", "wino4p", note="96 co: phase-planar activations; ragged rows; dil >= F"),
    _c("wino4p-8to128", "wino4", (128, 8, 5, 3), 1, 2, 36, 1, "wino4p", "wino2", note="128 co x 256 positions; T = 36 in 64-step tiles"),
    _c("wino4p-16to64-two-tiles", "wino4", (64, 16, 5, 3), 1, 9, 64, 2, "wino4p", "wino2", note="576 positions: a second, ragged 512-position tile"),
    _c("wino4-20+20to44", "wino4", (44, 40, 5, 3), 2, 3, 16, 1, "wino4", "wino4", split=20, vsplit=20, note="cin_split % 8 != 0: the round-1 kernel, 64 co"),
    _c("wino4-12+12to96", "wino4", (96, 24, 5, 3), 1, 3, 20, 1, "wino4", "wino2", split=12, note="round-1 kernel, 96 co"),
    _c("wino4-4+20to128", "wino4", (128, 24, 5, 3), 1, 2, 16, 1, "wino4", "wino2", split=4, note="round-1 kernel, 128 co, 8 waves"),
    # ---- F(2,5) x F(4,3), conv_wino45.hip: 64 co x (4 row pairs x 64 steps); Cin % 16 == 0, Cout > 32, T >= 64
    _c("wino45-16to40", "wino45", (40, 16, 5, 3), 2, 3, 64, 1, "wino45", "wino2", note="padded channel tile (PADC), odd row of a class"),
    _c("wino45-32to64-dil2", "wino45", (64, 32, 5, 3), 1, 9, 68, 2, "wino45", "wino2", note="ragged rows in both classes and one ragged time tile"),
    _c("wino45-48to48-dil4", "wino45", (48, 48, 5, 3), 1, 2, 64, 4, "wino45", "wino45", note="dil >= F: every class holds one row; both directions"),
    _c("wino45-16to96", "wino45", (96, 16, 5, 3), 1, 4, 64, 1, "wino45", "wino2", note="the 96-channel tile form where it is as full"),
    # ---- F(4,5) x F(4,3), conv_wino85.hip: 128 / 96 / 64 co x (one row quad x 64 steps)
    _c("wino85-16to64", "wino85", (64, 16, 5, 3), 2, 5, 64, 1, "wino85", "wino2", note="64-channel tiles; second quad holds one row"),
    _c("wino85-16to96-dil4", "wino85", (96, 16, 5, 3), 1, 3, 68, 4, "wino85", "wino2", note="96-channel tiles; dil >= F; ragged time tile"),
    _c("wino85-32to128", "wino85", (128, 32, 5, 3), 1, 9, 64, 1, "wino85", "wino2", note="128-channel tile, under both wave forms"),
    _c("wino85-64to64", "wino85", (64, 64, 5, 3), 1, 2, 64, 1, "wino85", "wino85", note="both directions"),
]
# ---- bf16 / bf16x3: conv_bf16p.hip takes KW = 3 or (1,1), T % 4 == 0, Cin % 8 == 0, Cout > 32, cin_split % 32 == 0 under 'bf16';
# conv_bf16.hip everything else and all of 'bf16x3'
for _p in ("bf16", "bf16x3"):
    _k = (lambda k: k) if _p == "bf16" else (lambda k: "bf16")
    CASES += [
        _c(f"{_p}-32to64", "bf16", (64, 32, 5, 3), 2, 3, 16, 1, _k("bf16p"), "bf16", precision=_p, note="transposed: Cout = 32 stays on the staging kernel"),
        _c(f"{_p}-40to96-dil2", "bf16", (96, 40, 5, 3), 1, 5, 36, 2, _k("bf16p"), _k("bf16p"), precision=_p, note="Cin % 32 != 0: half a 16-channel group is padding"),
        _c(f"{_p}-32+32to64", "bf16", (64, 64, 5, 3), 1, 3, 16, 1, _k("bf16p"), _k("bf16p"), split=32, vsplit=32, precision=_p),
        _c(f"{_p}-64to64-1x1", "bf16", (64, 64, 1, 1), 2, 3, 20, 1, _k("bf16p"), _k("bf16p"), precision=_p),
        _c(f"{_p}-32to64-T7", "bf16", (64, 32, 5, 3), 1, 3, 7, 1, "bf16", "bf16", precision=_p, note="T % 4 != 0: the staging kernel"),
    ]
del _p, _k
CASE_IDS = [c.name for c in CASES]
TINY = _c("tiny", "direct", (2, 2, 5, 3), 2, 3, 3, 2, "direct53", "direct53")       # the nested-loop pin


def case_by_name(name):
    return next(c for c in CASES if c.name == name)


def macs(c):
    Cout, Cin, KH, KW = c.w
    return c.B * Cout * Cin * KH * KW * c.F * c.T


def regimes_of(c, kernel):
    """Winograd kernels: the bound on `unit`, and on `integers` as a tap-placement check; every other kernel: equality."""
    return ("unit", "integers") if kernel in WINOGRAD else ("integers", "impulse")


# ----------------------------------------------------------------------------- layouts
def gap_floats(c):
    """Floats between two planes of a gapped view: every halo row of both neighbours (2 dil rows below one plane, 2 dil above the
    next) lies inside it, so a kernel that loads a halo row instead of taking zero reads NaN, never another plane's data."""
    return -(-(2 * c.dil * c.T + 2) // 4) * 4


def layout_of(c, name):
    """(off, extra) in floats: the view starts `off` floats into the buffer, plane stride F*T + extra."""
    g = gap_floats(c)
    odd = g + (1 - (c.F * c.T + g)) % 4                       # plane stride = 1 mod 4
    return {"dense": (0, 0), "gapped": (g, g), "odd": (1, g), "odd-stride": (0, odd)}[name]


def aligned(c, name):
    off, extra = layout_of(c, name)
    return off % 4 == 0 and (c.F * c.T + extra) % 4 == 0      # (batch stride = C * plane stride)


# every operand's layout; res: the layout of a residual of its own (each forward also runs with the residual aliasing out)
LAYOUTS = {
    "dense": dict(in_="dense", in2="dense", out="dense", res="dense"),
    "gapped": dict(in_="gapped", in2="gapped", out="gapped", res="gapped"),
    "in-gapped": dict(in_="gapped", in2="dense", out="dense", res="gapped"),
    "out-gapped": dict(in_="dense", in2="gapped", out="gapped", res="dense"),
    "odd": dict(in_="odd", in2="odd", out="odd", res="odd"),
    "odd-in": dict(in_="odd", in2="gapped", out="dense", res="gapped"),
    "odd-in2": dict(in_="gapped", in2="odd", out="gapped", res="dense"),
    "odd-out": dict(in_="gapped", in2="dense", out="odd", res="gapped"),
    "odd-res": dict(in_="dense", in2="gapped", out="gapped", res="odd"),
    "odd-stride": dict(in_="odd-stride", in2="odd-stride", out="odd-stride", res="odd-stride"),
}


def expected_kernel(c, direction, layout, res):
    """The kernel a call must take.  direction 'fwd' / 'vjp'; res: None, 'alias' (the residual is the output view) or 'own'."""
    k = c.fwd if direction == "fwd" else c.vjp
    lay = LAYOUTS[layout]
    two = (c.split if direction == "fwd" else c.vsplit) > 0
    present = {"in_": lay["in_"], "out": lay["out"]}
    if two:
        present["in2"] = lay["in2"]
    if res is not None:
        present["res"] = lay["out"] if res == "alias" else lay["res"]
    # (F(2,3) asks 8 bytes of out / res where the others ask 16; a float offset of 1 and an odd plane stride miss both)
    bad = {op for op, name in present.items() if not aligned(c, name)}
    return FALLBACK[k] if bad & set(ALIGN_CLAUSE[k]) else k


def exec_io(c, direction):
    """(Cin, Cout) of the op as executed."""
    Cout, Cin = c.w[:2]
    return (Cin, Cout) if direction == "fwd" else (Cout, Cin)


def sub_kernel(c, direction, two):
    """Which kernel of a shared counter slot runs on aligned views: the host rules restated (babe_conv11p_supported,
    csrc/conv11p.hip; babe_conv2d_wino4p_supported, csrc/conv_wino4p.hip) for the clauses these sizes can reach."""
    ci, co = exec_io(c, direction)
    split = (c.split if direction == "fwd" else c.vsplit) if two else 0
    if c.w[2:] == (1, 1) and c.precision == "f32":
        ok = c.T % 4 == 0 and not (two and split % 16) and not (c.F * c.T < 4096 and ci < 256)
        return "conv11p" if ok else "direct11"
    n32 = -(-co // 32)
    ok = (n32 % 4 == 0 or n32 in (2, 3)) and not (two and split % 8)
    return "wino4p" if ok else "wino4"


# ----------------------------------------------------------------------------- data
def _gen(c, *key):
    return torch.Generator().manual_seed(zlib.crc32(repr((c.name,) + key).encode()))


def _ints(g, shape, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _pow2(g, shape):
    mag = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, shape, generator=g)]
    return mag * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


def impulse_points(C, Fq, T):
    """The corners of the (channel, frequency, time) box and one interior point (fewer where an axis has one or two entries)."""
    pts = {(ch, f, t) for ch in (0, C - 1) for f in (0, Fq - 1) for t in (0, T - 1)}
    pts.add((C // 2, Fq // 2, T // 2))
    return sorted(pts)


def data(c, regime, direction):
    """dict of float32 CPU tensors of one (case, regime, direction): x [B, Cin_exec, F, T] (the forward input, or gy), w, res
    [B, Cout_exec, F, T], oscale / in_scale (or None), fbias (or None), alpha, rbeta.  The forward runs the full epilogue; the
    transposed call runs in_scale and alpha (the few-output-channel kernel, which takes no in_scale, accumulates into a residual)."""
    g, gw = _gen(c, regime, direction), _gen(c, regime != "unit", "w")      # (one set of weights for both directions and exact regimes)
    ci, co = exec_io(c, direction)
    Cout, Cin, KH, KW = c.w
    B, Fq, T = c.B, c.F, c.T
    exact = regime != "unit"
    if exact:
        w = _ints(gw, c.w)
        x = _ints(g, (B, ci, Fq, T))
        res = _ints(g, (B, co, Fq, T))
        osc, isc = _pow2(g, (B, co)), _pow2(g, (B, ci))
        fb = _ints(g, (co, Fq))
        alpha, rbeta = 0.5, 0.25
        if regime == "impulse":
            x = torch.zeros(B, ci, Fq, T)
            for ch, f, t in impulse_points(ci, Fq, T):
                x[:, ch, f, t] = 1.0
    else:
        w = torch.randn(c.w, generator=gw) / math.sqrt(Cin * KH * KW)
        x = torch.randn(B, ci, Fq, T, generator=g)
        res = torch.randn(B, co, Fq, T, generator=g)
        osc, isc = torch.randn(B, co, generator=g), torch.randn(B, ci, generator=g)
        fb = torch.randn(co, Fq, generator=g)
        alpha, rbeta = 0.7, 0.3
    d = dict(x=x, w=w, alpha=alpha, rbeta=rbeta, res=res, oscale=None, in_scale=None, fbias=None)
    if direction == "fwd":
        d["oscale"] = osc
        d["fbias"] = fb if c.fbias else None
    elif c.vjp == "fewco":
        pass                                            # alpha, and the residual accumulated in place
    else:
        d["in_scale"] = isc
        d["res"], d["rbeta"] = None, 0.0
    return d


def exactness_precondition(c, d):
    """The premises of the `integers` derivation (module docstring) on the data of one call; raises AssertionError."""
    Cout, Cin, KH, KW = c.w
    assert Cin * KH * KW <= 3840 and Cout * KH * KW <= 3840
    for k in ("x", "w", "res", "fbias"):
        if d[k] is not None:
            assert bool((d[k] == d[k].round()).all()) and float(d[k].abs().max()) <= 4, k
            assert torch.equal(d[k].bfloat16().float(), d[k]), k                   # exact in bf16
    for k in ("oscale", "in_scale"):
        if d[k] is not None:
            assert set(d[k].abs().flatten().tolist()) <= {0.5, 1.0, 2.0}, k
    assert d["alpha"] == 0.5 and d["rbeta"] in (0.0, 0.25)
    if d["in_scale"] is not None:
        xs = d["x"] * d["in_scale"][:, :, None, None]
        assert torch.equal(xs.bfloat16().float(), xs) and float(xs.abs().max()) <= 8


# ----------------------------------------------------------------------------- references (float64)
def _conv64(x, w, dil):
    KH, KW = w.shape[2:]
    return F.conv2d(x, w, padding=(dil * (KH // 2), KW // 2), dilation=(dil, 1))


def _epilogue64(y, d):
    if d["fbias"] is not None:
        y = y + d["fbias"].double()[None, :, :, None]
    y = d["alpha"] * y
    if d["oscale"] is not None:
        y = y * d["oscale"].double()[:, :, None, None]
    if d["res"] is not None:
        y = y + d["rbeta"] * d["res"].double()
    return y


def _core64(c, d, direction, magnitudes=False):
    """The conv (fwd) or its input-VJP from float64 autograd (vjp) of x (* in_scale), before the epilogue."""
    mag = (lambda t: t.abs()) if magnitudes else (lambda t: t)
    x, w = d["x"].double(), mag(d["w"].double())
    if d["in_scale"] is not None:
        x = x * d["in_scale"].double()[:, :, None, None]
    x = mag(x)
    if direction == "fwd":
        return _conv64(x, w, c.dil)
    Cout, Cin = c.w[:2]
    z = torch.zeros(c.B, Cin, c.F, c.T, dtype=torch.float64, requires_grad=True)
    gx, = torch.autograd.grad((_conv64(z, w, c.dil) * x).sum(), z)
    return gx


def reference(c, d, direction):
    return _epilogue64(_core64(c, d, direction), d)


def magnitude(c, d, direction):
    """A of the Winograd bound: the same op on |x * in_scale| and |w|, times |alpha * oscale|, plus |rbeta * res| (no bias: the
    Winograd rules refuse one)."""
    dm = dict(d, fbias=None, alpha=abs(d["alpha"]), rbeta=abs(d["rbeta"]), oscale=None if d["oscale"] is None else d["oscale"].abs(),
              res=None if d["res"] is None else d["res"].abs())
    return _epilogue64(_core64(c, d, direction, magnitudes=True), dm)


def ref_loops(c, d, direction):
    """The op as plain nested loops in float64 (module docstring): the one statement of the tap flip, of in_scale on the input
    side and of fbias inside alpha * oscale.  For the tiniest case only."""
    Cout, Cin, KH, KW = c.w
    B, Fq, T, dil = c.B, c.F, c.T, c.dil
    w, x = d["w"].double(), d["x"].double()
    ci_n, co_n = exec_io(c, direction)
    out = torch.zeros(B, co_n, Fq, T, dtype=torch.float64)
    for b in range(B):
        for co in range(Cout):
            for ci in range(Cin):
                for kh in range(KH):
                    for kw in range(KW):
                        df, dt = (kh - KH // 2) * dil, kw - KW // 2
                        for f in range(Fq):
                            for t in range(T):
                                if not (0 <= f + df < Fq and 0 <= t + dt < T):
                                    continue
                                if direction == "fwd":      # out[co, f, t] += w * x[ci, f + df, t + dt]
                                    out[b, co, f, t] += w[co, ci, kh, kw] * x[b, ci, f + df, t + dt]
                                else:                       # gx[ci, f + df, t + dt] += w * (in_scale[co] * gy[co, f, t])
                                    s = 1.0 if d["in_scale"] is None else float(d["in_scale"][b, co])
                                    out[b, ci, f + df, t + dt] += w[co, ci, kh, kw] * s * x[b, co, f, t]
    for b in range(B):
        for co in range(co_n):
            for f in range(Fq):
                for t in range(T):
                    v = out[b, co, f, t]
                    if d["fbias"] is not None:
                        v = v + float(d["fbias"][co, f])
                    v = d["alpha"] * v * (1.0 if d["oscale"] is None else float(d["oscale"][b, co]))
                    if d["res"] is not None:
                        v = v + d["rbeta"] * float(d["res"][b, co, f, t])
                    out[b, co, f, t] = v
    return out


# ----------------------------------------------------------------------------- Winograd transforms and the bound
# y[m outputs] = A^T [(G w) (.) (B^T d)], d = the m + r - 1 inputs from r // 2 before the first output: the matrices as the kernels'
# headers write them (csrc/conv_wino.hip; conv_wino4.hip; conv_wino45.hip with pack_wino45_kernel's G5; conv_wino85.hip with
# pack_wino85_kernel's G8).  winograd_identity_gap checks each transcription against the plain correlation.
_T = lambda rows: torch.tensor(rows, dtype=torch.float64)                                           # noqa: E731
BT4 = _T([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]])
F23 = dict(m=2, r=3, BT=_T([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]),
           G=_T([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]), AT=_T([[1, 1, 1, 0], [0, 1, -1, -1]]))
F43 = dict(m=4, r=3, BT=BT4, G=_T([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]),
           AT=_T([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]))
F25 = dict(m=2, r=5, BT=BT4,
           G=_T([[1 / 4, 0, 0, 0, 0], [-1 / 6] * 5, [-1 / 6, 1 / 6, -1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6, 1 / 3, 2 / 3],
                 [1 / 24, -1 / 12, 1 / 6, -1 / 3, 2 / 3], [0, 0, 0, 0, 1]]),
           AT=_T([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 1]]))
F45 = dict(m=4, r=5,
           BT=_T([[-1, 0, 21 / 4, 0, -21 / 4, 0, 1, 0],
                  [0, 1, 1, -17 / 4, -17 / 4, 1, 1, 0], [0, -1, 1, 17 / 4, -17 / 4, -1, 1, 0],
                  [0, 1 / 2, 1 / 4, -5 / 2, -5 / 4, 2, 1, 0], [0, -1 / 2, 1 / 4, 5 / 2, -5 / 4, -2, 1, 0],
                  [0, 2, 4, -5 / 2, -5, 1 / 2, 1, 0], [0, -2, 4, 5 / 2, -5, -1 / 2, 1, 0],
                  [0, -1, 0, 21 / 4, 0, -21 / 4, 0, 1]]),
           G=_T([[-1, 0, 0, 0, 0], [-2 / 9] * 5, [-2 / 9, 2 / 9, -2 / 9, 2 / 9, -2 / 9], [1 / 90, 1 / 45, 2 / 45, 4 / 45, 8 / 45],
                 [1 / 90, -1 / 45, 2 / 45, -4 / 45, 8 / 45], [32 / 45, 16 / 45, 8 / 45, 4 / 45, 2 / 45],
                 [32 / 45, -16 / 45, 8 / 45, -4 / 45, 2 / 45], [0, 0, 0, 0, 1]]),
           AT=_T([[1, 1, 1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 1 / 2, -1 / 2, 0], [0, 1, 1, 4, 4, 1 / 4, 1 / 4, 0],
                  [0, 1, -1, 8, -8, 1 / 8, -1 / 8, 1]]))
# family -> (frequency transform or None = the 5 taps stay a direct sum, time transform, weight transform in float64 at pack time)
FAMILY = {"wino2": (None, F23, False), "wino4": (None, F43, True), "wino4p": (None, F43, True), "wino45": (F25, F43, True),
          "wino85": (F45, F43, True)}


def winograd_identity_gap(tr, seed=0):
    """max |A^T[(G w)(.)(B^T d)] - correlation| over a seeded float64 draw: ~1e-15 when the three matrices belong together."""
    g = torch.Generator().manual_seed(seed)
    m, r = tr["m"], tr["r"]
    d, w = torch.randn(m + r - 1, generator=g, dtype=torch.float64), torch.randn(r, generator=g, dtype=torch.float64)
    y = tr["AT"] @ ((tr["G"] @ w) * (tr["BT"] @ d))
    ref = torch.stack([(w * d[o:o + r]).sum() for o in range(m)])
    return float((y - ref).abs().max())


def growth(tr):
    """How much larger the sum of magnitudes a transform forms is than the plain correlation's.  With every |w| and |d| equal to
    one, output o of the correlation sums r unit terms; the transform sums  sum_p |A^T[o,p]| (sum_k |G[p,k]|) (sum_i |B^T[p,i]|)
    (every cross term is present in magnitude and only cancels in exact arithmetic).  The ratio, at its worst output."""
    per_phase = tr["G"].abs().sum(1) * tr["BT"].abs().sum(1)
    return float((tr["AT"].abs() @ per_phase).max()) / tr["r"]


def _nnz(M):
    return int((M != 0).sum(1).max())


def wino_c(kernel, n_in):
    """c of the bound |got - ref| <= c 2^-24 A for a conv of n_in executed input channels.

    Standard forward error analysis with unit roundoff u = 2^-24: a value formed by n rounded operations from operands whose
    magnitudes sum to S carries an error of at most n u S (first order).  One output of a Winograd kernel is A^T applied to phase
    sums M_p = sum_k V_p[k] U_p[k] over n_acc = n_in * (5 frequency taps, where they stay a direct sum) channel-taps, and each
    operand is itself a short sum: U = B^T d in fp32 (nnz(B^T) operations per axis), V = G w rounded once from float64 (F(2,3):
    three fp32 operations), the output transform nnz(A^T) operations per axis, the nested kernels' carry of finished passes four,
    and in_scale, alpha, oscale and the residual add one each.  So n = n_acc + n_ops rounded operations act on a sum of magnitudes
    that is growth(frequency) * growth(time) times the A of the plain conv (growth, above; the two axes multiply because the nested
    transform is their Kronecker product).  A as the module defines it takes the magnitudes of the data as uniform over a
    transform's patch - true of the `unit` and `integers` regimes, not of `impulse`, which the Winograd families do not run.

    How wide this is: it multiplies two worst cases - every magnitude of every transform adding up, and every rounding error of
    n_acc + n_ops operations pointing the same way - where real errors largely cancel.  c is about 1e2 .. 1.3e3 for F(2,3),
    6e2 .. 8e3 for F(4,3), 6e3 .. 2.3e4 for F(2,5) x F(4,3) and 1e4 .. 3.5e4 for F(4,5) x F(4,3) over 5 .. 96 input channels,
    i.e. up to 1 - 2 % of the output's RMS per element for the nested kernels.  A correct fp32 implementation uses 0.1 - 2 % of
    it (the emulation here; the kernels' shares in tests/test_gpu_conv_edges.py's docstring).  A share of 0.3 is therefore NOT
    healthy: compare with the recorded shares.  What the bound catches for certain is a misplaced or dropped tap and a transform
    constant off by a quarter (tests/test_conv_cases_cpu.py); the exact `integers` / `impulse` runs of every other kernel and the
    NaN gaps do not depend on it."""
    ft, tt, w64 = FAMILY[kernel]
    g = growth(tt) * (growth(ft) if ft else 1.0)
    n_acc = n_in * (1 if ft else 5)
    n_ops = _nnz(tt["BT"]) + _nnz(tt["AT"]) + (1 if w64 else 3) + 4
    if ft:
        n_ops += _nnz(ft["BT"]) + _nnz(ft["AT"]) + 4
    return g * (n_acc + n_ops)


def direct_c(c, direction):
    """c of the same bound for the direct fp32 kernel, which a Winograd case ends on under a misaligned layout and then runs on
    `unit` data as well: one fp32 sum of Cin*KH*KW products (growth 1) and the four operations of in_scale and the epilogue."""
    return exec_io(c, direction)[0] * c.w[2] * c.w[3] + 4


def wino_bound(c, kernel, d, direction):
    cst = wino_c(kernel, exec_io(c, direction)[0]) if kernel in FAMILY else direct_c(c, direction)
    return cst * U32 * magnitude(c, d, direction)


def _tiles(x, dim, tr, n):
    """x zero-padded along dim for n tiles of tr and unfolded: the tile index replaces dim, the patch is appended last."""
    m, r = tr["m"], tr["r"]
    pad = [0, 0] * x.dim()
    lo, hi = r // 2, n * m + (r - 1 - r // 2) - x.shape[dim]
    pad[2 * (x.dim() - 1 - dim)], pad[2 * (x.dim() - 1 - dim) + 1] = lo, hi
    return F.pad(x, pad).unfold(dim, m + r - 1, m)


def wino_emulate(kernel, c, d, direction, mutate=None):
    """The family's algorithm in float32 on the CPU, from the matrices above: input transform, weight transform (float64 then
    rounded, as the pack kernels; F(2,3) in float32), fp32 accumulation over channels, output transform, epilogue.  Not the
    kernels' order of summation: any fp32 order obeys the bound.  mutate = (axis 'f' / 't', matrix 'G' / 'BT' / 'AT', row, column,
    factor): one constant of one transform scaled, for the test that the bound is not vacuous."""
    ft, tt, w64 = FAMILY[kernel]
    ft, tt = (dict(ft) if ft else None), dict(tt)
    if mutate:
        ax, name, i, j, fac = mutate
        tr = ft if ax == "f" else tt
        tr[name] = tr[name].clone()
        tr[name][i, j] *= fac
    f32 = lambda t: t.to(torch.float32)                                                              # noqa: E731
    x, w = d["x"], d["w"]
    if d["in_scale"] is not None:
        x = x * d["in_scale"][:, :, None, None]
    if direction == "vjp":                              # the transposed image: channels swapped, taps flipped on both axes
        w = w.transpose(0, 1).flip(2, 3)
    w = w.contiguous()
    B, Ci, Fq, T = x.shape
    Co, dil = w.shape[0], c.dil
    mt = tt["m"]
    nt = -(-T // mt)
    out = torch.zeros(B, Co, Fq, T)
    if ft is None:
        V = torch.einsum("pk,ochk->ochp", tt["G"] if w64 else f32(tt["G"]), w.double() if w64 else w)
        V = f32(V)
        U = torch.einsum("pi,bcfni->bcfnp", f32(tt["BT"]), _tiles(F.pad(x, (0, 0, 2 * dil, 2 * dil)), 3, tt, nt))
        M = torch.zeros(B, Co, Fq, nt, V.shape[-1])
        for kh in range(5):
            M = M + torch.einsum("ocp,bcfnp->bofnp", V[:, :, kh], U[:, :, kh * dil:kh * dil + Fq])
        out = torch.einsum("sp,bofnp->bofns", f32(tt["AT"]), M).reshape(B, Co, Fq, nt * mt)[..., :T]
    else:
        V = f32(torch.einsum("pk,ockl,ql->ocpq", ft["G"], w.double(), tt["G"]))
        mf = ft["m"]
        for r in range(min(dil, Fq)):                    # the rows of one residue class are an undilated problem
            rows = x[:, :, r::dil]
            nf = -(-rows.shape[2] // mf)
            D = _tiles(_tiles(rows, 2, ft, nf), 3, tt, nt)                      # [B, Ci, nf, nt, patch_f, patch_t]
            U = torch.einsum("pi,bcfnij,qj->bcfnpq", f32(ft["BT"]), D, f32(tt["BT"]))
            M = torch.einsum("ocpq,bcfnpq->bofnpq", V, U)
            Y = torch.einsum("rp,bofnpq,sq->bofrns", f32(ft["AT"]), M, f32(tt["AT"]))
            out[:, :, r::dil] = Y.reshape(B, Co, nf * mf, nt * mt)[:, :, :rows.shape[2], :T]
    y = out * torch.tensor(d["alpha"], dtype=torch.float32)
    if d["oscale"] is not None:
        y = y * d["oscale"][:, :, None, None]
    if d["res"] is not None:
        y = y + torch.tensor(d["rbeta"], dtype=torch.float32) * d["res"]
    return y


# ----------------------------------------------------------------------------- comparisons
def worst(err):
    """(value, (b, co, f, t)) of the largest entry of a 4-d tensor, NaN counting as the largest."""
    e = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    i = int(e.argmax())
    return float(e.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))


def check_exact(got, ref):
    """'' if got (float32) equals the float64 reference element for element, else a message naming the worst element."""
    if torch.equal(got.double(), ref):
        return ""
    v, idx = worst((got.double() - ref).abs())
    return f"{int((got.double() != ref).sum())} of {ref.numel()} elements differ; worst |got - ref| = {v:.3e} at (b, co, f, t) = {idx}: got {float(got[idx])}, want {float(ref[idx])}"


def bound_share(got, ref, bound):
    """(max |got - ref| / bound, its (b, co, f, t)); an element off its reference where the bound is zero, or a NaN, counts inf."""
    diff = (got.double() - ref).abs()
    share = torch.where(bound > 0, diff / bound.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))
    return worst(share)


def check_bound(got, ref, bound):
    v, idx = bound_share(got, ref, bound)
    msg = "" if v <= 1.0 else f"share {v:.3g} of the bound at (b, co, f, t) = {idx}: got {float(got[idx])}, want {float(ref[idx])}, bound {float(bound[idx]):.3e}"
    return msg, v


# ----------------------------------------------------------------------------- views in guarded buffers
class Placed:
    """A tensor [B, C, F, T] laid out in a buffer of its own at float offset `off` with plane stride F*T + extra, between two
    canaries of GUARD floats.  Everything that is not the view - the leading `off` floats, the gaps, the canaries - holds `fill` /
    `canary` (inputs: NaN, so a read outside the view poisons the result; outputs: 7.0 / -3.0, so a stray store of anything, NaN
    included, shows) and must come back bit for bit (intact).  Works on the CPU (tests of this module) and on the GPU."""

    def __init__(self, t, layout, fill=NAN, canary=NAN, device="cpu"):
        B, C, Fq, T = t.shape
        off, extra = layout
        self.cs = Fq * T + extra
        self.n = off + B * C * self.cs
        buf = torch.full((self.n + 2 * GUARD,), fill, dtype=torch.float32)
        buf[:GUARD] = canary
        buf[GUARD + self.n:] = canary
        self.buf = buf.to(device)
        self.view = self.buf.as_strided((B, C, Fq, T), (C * self.cs, self.cs, T, 1), GUARD + off)
        self.view.copy_(t)
        self.before = self.buf.clone()
        mask = torch.zeros(self.n + 2 * GUARD, dtype=torch.bool)
        mask.as_strided((B, C, Fq, T), (C * self.cs, self.cs, T, 1), GUARD + off).fill_(True)
        self.mask = mask

    def outside_intact(self):
        """Everything but the view is bit for bit what it was."""
        now, was = self.buf.cpu().view(torch.int32), self.before.cpu().view(torch.int32)
        return bool(torch.equal(now[~self.mask], was[~self.mask]))

    def unchanged(self):
        """The whole buffer, view included (an input)."""
        return bool(torch.equal(self.buf.cpu().view(torch.int32), self.before.cpu().view(torch.int32)))


def conv_with_memory_halo(c, d, placed):
    """The forward conv of the case's x as a kernel WITHOUT its frequency mask would compute it: halo rows taken from the memory
    around each plane of `placed` (a CPU Placed of x) instead of zero.  For the test that a NaN gap fails the comparison."""
    x = d["x"]
    B, C, Fq, T = x.shape
    pad = 2 * c.dil
    base = GUARD + (placed.buf.numel() - 2 * GUARD - B * C * placed.cs)
    xp = torch.zeros(B, C, Fq + 2 * pad, T, dtype=torch.float64)
    for b in range(B):
        for ch in range(C):
            s = base + (b * C + ch) * placed.cs - pad * T
            xp[b, ch] = placed.buf[s:s + (Fq + 2 * pad) * T].double().reshape(Fq + 2 * pad, T)
    return _epilogue64(F.conv2d(xp, d["w"].double(), padding=(0, c.w[3] // 2), dilation=(c.dil, 1)), d)


# ----------------------------------------------------------------------------- the library's own verdict (host rules, no GPU)
def library_slot(c, direction, layout, res):
    """The counter slot the library's exported host rules send this call to: babe_packed_conv_plan for the images, STRIP, then the
    order of ops.conv2d and babe_conv2d_auto (csrc/conv_auto.hip) over babe_conv2d_*_supported / *_preferred, asked with made-up
    addresses that have the layout's alignment.  A cross-check of the table on the CPU, not a second owner of the dispatch: it
    restates that order (the F(4,3) and F(2,3) steps ask for the forward image in both directions, as babe_conv2d_auto does) and
    has to follow a change of it; the GPU test asserts the launch counters whatever this says.  None for the bf16 precisions:
    their one rule, babe_conv2d_bf16p_supported, has no C linkage, so for those cases the table is checked on the GPU only."""
    import ctypes as C
    from babe_amd._cabi import IMAGE_SLOTS, ConvArgs, PackedConvLayout
    from babe_amd._lib import lib
    if c.precision != "f32":
        return None
    L = lib()
    Cout, Cin, KH, KW = c.w
    plan = PackedConvLayout()
    assert L.babe_packed_conv_plan(Cout, Cin, KH, KW, 0, 0, 2, 31, C.byref(plan)) == 0
    have = {n for n, b in zip(IMAGE_SLOTS, plan.bytes) if b} | ({"w_raw"} if plan.raw else set())
    have -= set(STRIP[c.family])
    lay = LAYOUTS[layout]
    ci, co = exec_io(c, direction)
    split = c.split if direction == "fwd" else c.vsplit
    a = ConvArgs()

    def put(prefix, name, chans, base):
        off, extra = layout_of(c, name)
        cs = c.F * c.T + extra
        setattr(a, prefix, base + 4 * off)
        setattr(a, prefix + ("bs" if prefix.endswith("_") else "_bs"), chans * cs)
        setattr(a, prefix + ("cs" if prefix.endswith("_") else "_cs"), cs)
    put("in_", lay["in_"], split or ci, 0x10000000)
    if split:
        put("in2", lay["in2"], ci - split, 0x20000000)
    a.cin_split = split or ci
    put("out", lay["out"], co, 0x30000000)
    if res == "alias":
        put("res", lay["out"], co, 0x30000000)
    elif res == "own":
        put("res", lay["res"], co, 0x40000000)
    a.w_packed = 0x50000000
    a.B, a.Cin, a.Cout, a.F, a.T, a.KH, a.KW, a.dil = c.B, ci, co, c.F, c.T, KH, KW, c.dil
    if direction == "vjp" and c.vjp != "fewco":
        a.in_scale = 0x60000000
    if direction == "fwd":
        a.oscale = 0x70000000
        if c.fbias:
            a.fbias = 0x80000000
    p = C.byref(a)
    d = "bwd" if direction == "vjp" else "fwd"
    if "w_raw" in have and co <= 4 and L.babe_conv2d_fewco_supported(p):
        return "conv53_fewco"
    nested, f45 = c.family == "wino45", c.family == "wino85"
    w85 = d + "_wino85" in have and not split and not nested
    if nested and d + "_wino45" in have and L.babe_conv2d_wino45_supported(p):
        return "conv53_wino45"
    if f45 and w85 and L.babe_conv2d_wino85_supported(p):
        return "conv53_wino85"
    if w85 and L.babe_conv2d_wino85_preferred(p):
        return "conv53_wino85"
    if d + "_wino45" in have and L.babe_conv2d_wino45_preferred(p):
        return "conv53_wino45"
    if "fwd_wino4" in have and L.babe_conv2d_wino4_supported(p):
        return "conv53_wino4"
    if "fwd_wino" in have and L.babe_conv2d_wino_supported(p):
        return "conv53_wino2"
    return "conv53_direct" if KH > 1 else "conv11"


# ----------------------------------------------------------------------------- the call (GPU)
def build_packed(c, w):
    """The case's PackedConv with the family's images only (STRIP), at the case's precision.  The bf16 cases are to be built with
    FORMS.bf16_hbm_f32 off (the caller selects the form, tests/test_gpu_conv_edges.py), so that the named precision is what runs
    for the narrow and the (1,1) shapes too; the assertion below holds the caller to it."""
    from babe_amd import ops
    pc = ops.PackedConv(w.cuda(), c.precision)
    assert pc.splits == {"f32": 0, "bf16": 1, "bf16x3": 2}[c.precision], (c.name, pc.splits)
    for name in STRIP[c.family]:
        setattr(pc, name, None)
    return pc


class GpuError(RuntimeError):
    """The device reported an error after a launch (a fault): the caller must start nothing more on the GPU."""


def run(c, pc, d, direction, layout, res_mode):
    """One call through ops.conv2d (babe_conv2d_auto, or the forced nested entry points) on Placed views.
    res_mode: None, 'alias' or 'own'.  Returns dict(got [B, C, F, T] on the CPU, counts {slot: launches}, out / ins Placed)."""
    from babe_amd import ops
    from babe_amd._lib import dispatch_counts
    lay = LAYOUTS[layout]
    L = lambda op: layout_of(c, lay[op])                                                             # noqa: E731
    x = d["x"]
    split = c.split if direction == "fwd" else c.vsplit
    ins = [Placed(x[:, :split] if split else x, L("in_"), device="cuda")]
    if split:
        ins.append(Placed(x[:, split:], L("in2"), device="cuda"))
    co = exec_io(c, direction)[1]
    has_res = d["res"] is not None and res_mode is not None
    init = d["res"] if has_res and res_mode == "alias" else torch.full((c.B, co, c.F, c.T), NAN)
    out = Placed(init, L("out"), fill=OUT_FILL, canary=OUT_CANARY, device="cuda")
    res = None
    if has_res:
        if res_mode == "own":
            ins.append(Placed(d["res"], L("res"), device="cuda"))
            res = ins[-1].view
        else:
            res = out.view
    small = {k: Placed(d[k].reshape(1, 1, 1, -1), (0, 0), device="cuda") for k in ("oscale", "in_scale", "fbias") if d[k] is not None}
    sv = lambda k: small[k].view.reshape(d[k].shape) if k in small else None                        # noqa: E731
    torch.cuda.synchronize()
    dispatch_counts(reset=True)
    ops.conv2d(ins[0].view, pc, out.view, dil=c.dil, transpose=direction == "vjp", x2=ins[1].view if split else None, res=res,
               in_scale=sv("in_scale"), oscale=sv("oscale"), alpha=d["alpha"], rbeta=d["rbeta"] if has_res else 0.0,
               force_nested=c.family == "wino45", force_f45=c.family == "wino85", fbias=sv("fbias"))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        raise GpuError(f"GPU error after {c.name} {layout} {direction} res={res_mode}: {e}") from e
    counts = {k: n for k, n in dispatch_counts().items() if n}
    return dict(got=out.view.cpu().clone(), counts=counts, out=out, ins=ins + list(small.values()))
