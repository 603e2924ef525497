"""tests/conv_cases.py is right without a GPU: the float64 references equal the op stated as nested loops, the `integers` regime
really is exact in fp32 and bf16, the Winograd bound holds a float32 emulation of each algorithm and rejects one with a wrong
transform constant, the expected kernels are what the library's host rules answer, and the comparison helpers fail on the faults
they are there to find."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as cc

WINO_CASES = [(c, d) for c in cc.CASES for d in ("fwd", "vjp") if (c.fwd if d == "fwd" else c.vjp) in cc.WINOGRAD]
_WID = [f"{c.name}-{d}" for c, d in WINO_CASES]


# ----------------------------------------------------------------------------- the table itself
def test_table_reaches_every_source_in_both_directions():
    for src in cc.SOURCES:
        for attr in ("fwd", "vjp"):
            assert any(cc.KERNEL_SOURCE[getattr(c, attr)] == src for c in cc.CASES), (src, attr)
    assert len(set(cc.CASE_IDS)) == len(cc.CASES)
    for c in cc.CASES:
        assert 1000 <= cc.macs(c) <= 40e6, (c.name, cc.macs(c))          # small: a thousandth of the workload's layers at the most
        # the shared-slot pairs: the stated kernel is what the restated sub-rule answers
        for d, k, sp in (("fwd", c.fwd, c.split), ("vjp", c.vjp, c.vsplit)):
            if k in ("direct11", "conv11p", "wino4", "wino4p"):
                assert cc.sub_kernel(c, d, sp > 0) == k, (c.name, d)


def test_gaps_hold_every_halo_row():
    for c in cc.CASES:
        g = cc.gap_floats(c)
        assert g % 4 == 0 and g >= 2 * c.dil * c.T
        assert cc.layout_of(c, "odd")[0] == 1 and not cc.aligned(c, "odd") and not cc.aligned(c, "odd-stride")
        assert cc.aligned(c, "gapped") == cc.aligned(c, "dense") == ((c.F * c.T) % 4 == 0)


@pytest.mark.parametrize("c", cc.CASES, ids=cc.CASE_IDS)
def test_expected_kernels_are_the_host_rules_verdict(c):
    """Pure host arithmetic of the built library (as tests/test_conv_rules_cpu.py): every (layout, direction, residual) of the case
    goes where the table says, and a family with an alignment clause is refused on every layout that breaks it.  The bf16 cases
    have no verdict here (conv_cases.library_slot returns None for them: their rule is not callable from outside the library), so
    for them only the second half, the table's own consistency, is checked; which bf16 kernel runs is asserted on the GPU."""
    import os
    from babe_amd import _lib
    if not os.path.exists(_lib._LIB_PATH):
        pytest.fail(f"{_lib._LIB_PATH} is not built")
    for layout in cc.LAYOUTS:
        for d, modes in (("fwd", ("alias", "own")), ("vjp", ("alias",) if c.vjp == "fewco" else (None,))):
            for res in modes:
                want = cc.KERNEL_SLOT[cc.expected_kernel(c, d, layout, res)]
                got = cc.library_slot(c, d, layout, res)
                assert got is None or got == want, (c.name, layout, d, res, got, want)
    for d, k in (("fwd", c.fwd), ("vjp", c.vjp)):
        if cc.ALIGN_CLAUSE[k]:
            assert cc.expected_kernel(c, d, "odd", "alias" if d == "fwd" else None) == cc.FALLBACK[k]
            assert cc.expected_kernel(c, d, "odd-stride", "alias" if d == "fwd" else None) == cc.FALLBACK[k]


# ----------------------------------------------------------------------------- references
@pytest.mark.parametrize("direction", ["fwd", "vjp"])
@pytest.mark.parametrize("fbias", [False, True])
def test_references_equal_the_nested_loops(direction, fbias):
    c = cc.TINY._replace(fbias=fbias)
    for regime in ("integers", "unit"):
        d = cc.data(c, regime, direction)
        ref, loops = cc.reference(c, d, direction), cc.ref_loops(c, d, direction)
        if regime == "integers":
            assert torch.equal(ref, loops)
        else:
            assert float((ref - loops).abs().max()) < 1e-13
    # the convention is not symmetric: a flipped tap order or in_scale on the output side is another function
    d = cc.data(c, "unit", "vjp")
    flipped = dict(d, w=d["w"].flip(3))
    assert float((cc.reference(c, flipped, "vjp") - cc.ref_loops(c, d, "vjp")).abs().max()) > 1e-3


@pytest.mark.parametrize("c", cc.CASES, ids=cc.CASE_IDS)
def test_integers_are_exact_in_fp32(c):
    """The precondition holds and a float32 torch conv on the CPU equals the float64 reference bit for bit, both directions and both
    exact regimes: the data is exact in fp32, not merely close."""
    for direction in ("fwd", "vjp"):
        for regime in ("integers", "impulse"):
            d = cc.data(c, regime, direction)
            cc.exactness_precondition(c, d)
            ref = cc.reference(c, d, direction)
            x, w = d["x"], d["w"]
            if d["in_scale"] is not None:
                x = x * d["in_scale"][:, :, None, None]
            if direction == "vjp":
                w = w.transpose(0, 1).flip(2, 3).contiguous()
            y = F.conv2d(x, w, padding=(c.dil * (c.w[2] // 2), c.w[3] // 2), dilation=(c.dil, 1))
            if d["fbias"] is not None:
                y = y + d["fbias"][None, :, :, None]
            y = y * torch.tensor(d["alpha"])
            if d["oscale"] is not None:
                y = y * d["oscale"][:, :, None, None]
            if d["res"] is not None:
                y = y + torch.tensor(d["rbeta"]) * d["res"]
            assert y.dtype == torch.float32
            assert cc.check_exact(y, ref) == "", (direction, regime)
            if regime == "impulse":                        # the output is the weights laid down around each point: not all zero
                assert int((cc._core64(c, d, direction) != 0).sum()) > 0


# ----------------------------------------------------------------------------- Winograd bound
def test_transform_matrices_are_winograd_identities():
    for tr in (cc.F23, cc.F43, cc.F25, cc.F45):
        assert cc.winograd_identity_gap(tr) < 1e-12
    # growth: F(2,3) 8/3 (outputs sum 2 + 3 + 3 magnitudes where the correlation sums 3), larger for the larger tiles
    assert abs(cc.growth(cc.F23) - 8 / 3) < 1e-12
    assert cc.growth(cc.F23) < cc.growth(cc.F43) and cc.growth(cc.F25) < cc.growth(cc.F45)


@pytest.mark.parametrize("c,direction", WINO_CASES, ids=_WID)
def test_winograd_emulation_stays_inside_the_bound(c, direction):
    """A float32 emulation of the family's algorithm, built from the header's matrices, stays within c 2^-24 A on `unit` and
    `integers`; with one transform constant replaced by a neighbour (1/6 -> 1/8 and the like: x 3/4) it does not.  So the bound
    is met by a correct implementation and not vacuous, without having been measured on the code under test."""
    kernel = c.fwd if direction == "fwd" else c.vjp
    nested = cc.FAMILY[kernel][0] is not None
    for regime in ("unit", "integers"):
        d = cc.data(c, regime, direction)
        ref, bound = cc.reference(c, d, direction), cc.wino_bound(c, kernel, d, direction)
        msg, share = cc.check_bound(cc.wino_emulate(kernel, c, d, direction), ref, bound)
        print(f"CONV_EMU {kernel} {c.name} {direction} {regime} share {share:.3f}")
        assert msg == "", msg
    d = cc.data(c, "unit", direction)
    ref, bound = cc.reference(c, d, direction), cc.wino_bound(c, kernel, d, direction)
    mutations = [("t", "G", 1, 0, 0.75), ("t", "AT", 1, 2, 0.75), ("t", "BT", 1, 2, 0.75)]
    if nested:
        mutations += [("f", "G", 1, 0, 0.75), ("f", "AT", 0, 2, 0.75), ("f", "BT", 1, 2, 0.75)]      # (row 0: a class may hold one row)
    for mut in mutations:
        msg, share = cc.check_bound(cc.wino_emulate(kernel, c, d, direction, mutate=mut), ref, bound)
        assert msg != "" and share > 1.0, (mut, share)


# ----------------------------------------------------------------------------- the comparisons find the faults
def _exact_case():
    c = cc.case_by_name("direct-8to32-dil2")
    d = cc.data(c, "integers", "fwd")
    return c, d, cc.reference(c, d, "fwd")


def test_a_moved_tap_fails_both_comparisons():
    c, d, ref = _exact_case()
    w = d["w"].clone()
    w[3, 5, 2, 0], w[3, 5, 2, 1] = d["w"][3, 5, 2, 1], d["w"][3, 5, 2, 0] + 1       # one tap of one channel pair, one step along time
    bad = cc.reference(c, dict(d, w=w), "fwd").float()
    msg = cc.check_exact(bad, ref)
    assert msg and "(b, co, f, t) = (0, 3," in msg
    assert cc.check_exact(ref.float(), ref) == ""
    for c, direction in WINO_CASES:
        kernel = c.fwd if direction == "fwd" else c.vjp
        d = cc.data(c, "unit", direction)
        ref, bound = cc.reference(c, d, direction), cc.wino_bound(c, kernel, d, direction)
        assert cc.check_bound(ref.float(), ref, bound)[0] == ""
        w = d["w"].clone()            # the channel pair whose first two time taps of the centre row (inside at every dil) differ most
        kh = 2
        co, ci = (int(v) for v in torch.unravel_index((w[:, :, kh, 0] - w[:, :, kh, 1]).abs().argmax(), w.shape[:2]))
        w[co, ci, kh, 0], w[co, ci, kh, 1] = d["w"][co, ci, kh, 1], d["w"][co, ci, kh, 0]
        msg, share = cc.check_bound(cc.reference(c, dict(d, w=w), direction).float(), ref, bound)
        assert msg and share > 1.0, (c.name, direction, share)


def test_a_halo_row_from_memory_fails():
    c, d, ref = _exact_case()
    pl = cc.Placed(d["x"], cc.layout_of(c, "gapped"))
    got = cc.conv_with_memory_halo(c, d, pl)
    assert bool(torch.isnan(got).any()) and cc.check_exact(got.float(), ref) != ""
    # the same read goes unnoticed where the neighbourhood holds zeros: what the NaN gaps are for
    pl0 = cc.Placed(d["x"], cc.layout_of(c, "gapped"), fill=0.0, canary=0.0)
    assert cc.check_exact(cc.conv_with_memory_halo(c, d, pl0).float(), ref) == ""
    # a single halo row: the row just above plane (0, 1) taken from memory
    x = d["x"].double()
    xp = F.pad(x, (0, 0, 2 * c.dil, 2 * c.dil))
    xp[0, 1, 2 * c.dil - c.dil] = float("nan")
    one = cc._epilogue64(F.conv2d(xp, d["w"].double(), padding=(0, 1), dilation=(c.dil, 1)), d)
    msg = cc.check_exact(one.float(), ref)
    assert msg and "inf" in msg
    bound = torch.ones_like(ref)
    assert cc.check_bound(one.float(), ref, bound)[0] != ""


def test_an_unwritten_element_and_a_stray_store_fail():
    c, d, ref = _exact_case()
    got = ref.float()
    got[0, 31, 1, 15] = float("nan")
    msg = cc.check_exact(got, ref)
    assert msg and "(0, 31, 1, 15)" in msg
    m, share = cc.check_bound(got, ref, torch.ones_like(ref))
    assert m and share == float("inf")
    for layout in ("gapped", "odd", "odd-stride", "dense"):
        out = cc.Placed(torch.full(ref.shape, cc.NAN), cc.layout_of(c, layout), fill=cc.OUT_FILL, canary=cc.OUT_CANARY)
        out.view.copy_(ref.float())
        assert out.outside_intact() and not out.unchanged()
        outside = (~out.mask).nonzero().flatten()
        for pos in (outside[0], outside[len(outside) // 2], outside[-1]):       # a canary, a gap (or canary), the last canary
            for value in (0.0, float("nan")):
                keep = float(out.buf[pos])
                out.buf[pos] = value
                assert not out.outside_intact(), (layout, int(pos), value)
                out.buf[pos] = keep
        assert out.outside_intact()
    gapped = cc.Placed(torch.zeros(ref.shape), cc.layout_of(c, "gapped"))
    assert int((~gapped.mask).sum()) > 2 * cc.GUARD + cc.gap_floats(c)          # there are gap elements to overwrite
