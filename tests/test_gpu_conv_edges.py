"""Every conv kernel family element by element on guarded, strided views: conv.hip, conv11p.hip, conv_fewco.hip, conv_wino.hip,
conv_wino4.hip, conv_wino4p.hip, conv_wino45.hip, conv_wino85.hip, conv_bf16.hip and conv_bf16p.hip, each forward with the full
epilogue and as input-VJP, at the smallest shapes that can still go wrong.  Cases, data, float64 references and the derived
bounds: tests/conv_cases.py, pinned on the CPU by tests/test_conv_cases_cpu.py.  Needs a MI355X.

Every call goes through ops.conv2d (babe_conv2d_auto, or the forced nested entry points) on `Placed` views: inputs lie in buffers
of their own between NaN canaries with NaN in every gap between planes, wide enough to hold all halo rows, so a kernel that LOADS a
row outside its view and cancels it with a packed zero or a masked multiply returns NaN; outputs are written over NaN inside the
view and 7.0 outside it, and everything outside the view - leading floats, gaps, both canaries - must come back bit for bit.  The
launch counters must show exactly the kernel the case was built for (no skip, no silent fall-back); on the misaligned layouts
the families with an alignment clause must show no launch and the direct / staging kernel one.  Non-Winograd kernels, both bf16
precisions included, are held to torch.equal against float64 on data that is exact in every format involved; the Winograd
families to the per-element bound c 2^-24 A of tests/conv_cases.py::wino_c.

Largest share of its bound that each kernel used on a MI355X, over every case, layout, regime and direction of this file (612
tests, 7.6 s; every call prints its own as `CONV_EDGE <kernel> share <x>`, the last test the worst per kernel as `CONV_EDGE worst`):
  kernel     source             worst share   where
  wino2      conv_wino.hip      0.0184        wino2-5to20, forward, unit
  wino4      conv_wino4.hip     0.0064        wino4-12+12to96, forward, unit
  wino4p     conv_wino4p.hip    0.0166        wino4p-8to128, forward, unit
  wino45     conv_wino45.hip    0.0034        wino45-16to40, forward, integers
  wino85     conv_wino85.hip    0.0053        wino85-16to96-dil4, forward, unit
  direct53   conv.hip           0.0307        wino2-5to20 on a misaligned layout (unit data on the direct kernel), forward
The bound is a product of two worst cases (tests/conv_cases.py::wino_c) and correct code uses a few hundredths of it at the most:
these figures, not 1, are what a later run is to be compared with - a share of 0.3 would be a regression by a factor of ten or
more.  Every other kernel (conv.hip on exact data, conv11p.hip, conv_fewco.hip, conv_bf16.hip, conv_bf16p.hip) is held to
equality.  The launch counters showed all ten sources in both directions; no case produced a NaN, a store outside its view or
a wrong element, so nothing in csrc changed.
"""
import pytest
import torch

from tests import conv_cases as cc

pytestmark = pytest.mark.gpu

_REF, _PC, _RAN, _SHARE = {}, {}, {}, {}


def _shared(c, regime, direction):
    """Data, float64 reference and bound of one (case, regime, direction): computed once, shared, never modified."""
    key = (c.name, regime, direction)
    if key not in _REF:
        d = cc.data(c, regime, direction)
        if regime != "unit":
            cc.exactness_precondition(c, d)
        _REF[key] = (d, cc.reference(c, d, direction))
    return _REF[key]


def _packed(c, regime, w):
    key = (c.name, regime != "unit")                   # (the exact regimes share their integer weights)
    if key not in _PC:
        from babe_amd.forms import FORMS
        with pytest.MonkeyPatch.context() as mp:       # the named precision is what runs, also for the narrow and the (1,1) shapes
            if c.precision != "f32":
                mp.setattr(FORMS, "bf16_hbm_f32", False)
            _PC[key] = cc.build_packed(c, w)
    return _PC[key]


def _one(c, layout, direction, regime, res_mode):
    """One call and every check on it; returns the output [B, C, F, T] (CPU) and the kernel that ran."""
    d, ref = _shared(c, regime, direction)
    pc = _packed(c, regime, d["w"])
    kernel = cc.expected_kernel(c, direction, layout, res_mode)
    what = f"{c.name} {layout} {direction} {regime} res={res_mode}"
    try:
        r = cc.run(c, pc, d, direction, layout, res_mode)
    except cc.GpuError as e:                            # a fault: nothing more is launched in this session
        pytest.exit(str(e), returncode=3)
    # the intended kernel ran, and no other conv kernel
    want = {cc.KERNEL_SLOT[kernel]: 1}
    assert {k: n for k, n in r["counts"].items() if k in cc.CONV_SLOTS} == want, (what, kernel, r["counts"])
    _RAN.setdefault(cc.KERNEL_SOURCE[kernel], set()).add(direction)
    # outputs: nothing outside the view touched, nothing inside left unwritten; inputs unchanged
    assert r["out"].outside_intact(), f"{what}: a store outside the output view (gap, leading floats or canary)"
    for pl in r["ins"]:
        assert pl.unchanged(), f"{what}: an input buffer was written"
    got = r["got"]
    nan = torch.isnan(got)
    assert not bool(nan.any()), f"{what}: {int(nan.sum())} NaN in the output, first at (b, co, f, t) = {tuple(int(v) for v in nan.nonzero()[0])}"
    # values
    if kernel in cc.WINOGRAD or regime == "unit":       # (unit data on the direct kernel: a Winograd case on a misaligned layout)
        assert kernel in cc.WINOGRAD or kernel == "direct53", what
        msg, share = cc.check_bound(got, ref, cc.wino_bound(c, kernel, d, direction))
        print(f"CONV_EDGE {kernel} share {share:.4f} ({what})")
        if share >= _SHARE.get(kernel, (-1.0, ""))[0]:
            _SHARE[kernel] = (share, what)
        assert msg == "", f"{what} on {kernel}: {msg}"         # (share <= 1: asserted here, where it is measured)
    else:
        msg = cc.check_exact(got, ref)
        assert msg == "", f"{what} on {kernel}: {msg}"
    return got, kernel


@pytest.mark.parametrize("layout", list(cc.LAYOUTS))
@pytest.mark.parametrize("c", cc.CASES, ids=cc.CASE_IDS)
def test_conv_case(c, layout):
    for direction in ("fwd", "vjp"):
        kernel0 = c.fwd if direction == "fwd" else c.vjp
        for regime in cc.regimes_of(c, kernel0):
            if direction == "fwd":
                a, ka = _one(c, layout, direction, regime, "alias")
                o, ko = _one(c, layout, direction, regime, "own")
                if ka == ko:                 # a residual that aliases the output and one of its own: the same bits
                    assert torch.equal(a.view(torch.int32), o.view(torch.int32)), (c.name, layout, regime, ka)
            else:
                _one(c, layout, direction, regime, "alias" if c.vjp == "fewco" else None)


def test_f45_wave_forms_agree_bit_for_bit():
    """The 128-channel tile of conv_wino85.hip under its 8- and its 12-wave form, on guarded gapped views."""
    from babe_amd._lib import lib
    c = cc.case_by_name("wino85-32to128")
    got = {}
    try:
        for waves in (8, 12):
            assert lib().babe_conv2d_wino85_set_waves(waves) == 0
            got[waves] = _one(c, "gapped", "fwd", "unit", "own")[0]
            _one(c, "dense", "fwd", "integers", "alias")
    finally:
        assert lib().babe_conv2d_wino85_set_waves(12) == 0
    assert torch.equal(got[8].view(torch.int32), got[12].view(torch.int32))


def test_every_source_ran_in_both_directions():
    """Each of the ten kernel sources takes at least one forward and one transposed call, by the launch counters that _one
    asserts.  Needs no other test of this file: a (source, direction) that no earlier test of the session has run is run here, on
    the first case of the table that reaches it.  Then the summary: the worst share of every kernel that was held to the bound
    in this session (each already asserted where it was measured)."""
    for c in cc.CASES:
        for direction, k in (("fwd", c.fwd), ("vjp", c.vjp)):
            if direction not in _RAN.get(cc.KERNEL_SOURCE[k], set()):
                _one(c, "dense", direction, cc.regimes_of(c, k)[0], "alias" if (direction == "fwd" or k == "fewco") else None)
    assert {s: sorted(v) for s, v in _RAN.items() if s in cc.SOURCES} == {s: ["fwd", "vjp"] for s in cc.SOURCES}
    for kernel, (share, what) in sorted(_SHARE.items()):
        print(f"CONV_EDGE worst {kernel} share {share:.4f} ({what})")
