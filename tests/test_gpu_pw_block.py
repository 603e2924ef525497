"""The fused forward passes of the k = (1,1) ResnetBlocks (csrc/pw_block.hip: the init blocks 2 -> N, the output heads N -> 2) against
a float64 torch composition of the formulas in the header of csrc/norm.hip plus 1x1 convs.

Tolerance: no fixed number.  The existing layer-by-layer HIP path (the calls UnetEngine.block_fwd makes) runs on the same inputs
against the same float64 result, and the fused pass may be at most twice as far away (relative L2; the margin covers the
re-associated channel sums), with a floor of 1e-6 where the layer-by-layer error is essentially zero.  stats and scale, which the
VJP reads, must be the bits babe_scale_gelu_fin writes.

Shapes: N in {64, 96, 128, 256} = two to eight 32-channel tiles, a width that is no power of two and a group size of 12, images
packed for 2 and for 3 row tiles; F = 3, T = 44 = 132 positions, one full 128-position tile and a ragged one; B = 2 with different
FiLM rows; the init block's output a frequency sub-range of a wider tensor."""
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

RS2 = 1.0 / math.sqrt(2.0)
F, T, B = 3, 44, 2
WIDTHS = [64, 96, 128, 256]


@pytest.fixture(autouse=True)
def _switch_on():
    """The library's switch on for every test here, whatever the process started with; restored afterwards."""
    from babe_amd import ops
    prev = ops.pw_block_enable(True)
    yield
    ops.pw_block_enable(prev)


def _block(N, head, gen):
    """A (1,1) ResnetBlock's weights: float64 masters (rounded to fp32 values) and the packed block the passes take."""
    from babe_amd import ops
    from babe_amd.networks.unet_c import c_block
    r = lambda *s: torch.randn(*s, generator=gen)
    w = {"H": r(N, N, 1, 1) / math.sqrt(N), "gamma": 1.0 + 0.2 * r(N)}
    if head:
        w["proj_out"], w["res_conv"] = r(2, N, 1, 1) / math.sqrt(N), r(2, N, 1, 1) / math.sqrt(N)
    else:
        w["proj_in"], w["res_conv"] = r(N, 2, 1, 1), r(N, 2, 1, 1)
    pc = {k: ops.PackedConv(v.cuda()) for k, v in w.items() if k != "gamma"}
    blk = types.SimpleNamespace(N=N, nd=1, k53=False, proj_in=pc.get("proj_in"), res_conv=pc["res_conv"], proj_out=pc.get("proj_out"),
                                H=[pc["H"]], gamma=[w["gamma"].cuda()], film_off=[(5, 5 + N)], fenc=None)
    blk.c = c_block(blk)
    return w, blk


def _inputs(N, head, gen):
    x = torch.randn(B, N if head else 2, F, T, generator=gen).cuda()
    film = (0.3 * torch.randn(B, 2 * N + 9, generator=gen)).cuda()            # rows differ; affine at 5, gate at 5 + N
    return x, film


def _reference(w, z, x, film, N, head, add=None):
    """float64: GroupNorm without mean removal (unbiased std over the group), FiLM, exact GELU, the (1,1) layer, the block's tail."""
    d = lambda t: t.double().cpu()
    z, film = d(z), d(film)
    aff, gate = film[:, 5:5 + N], film[:, 5 + N:5 + 2 * N]
    sd = z.reshape(B, 8, -1).std(dim=2, unbiased=True)
    scale = d(w["gamma"])[None] * (aff + 1) / (sd + 1e-7).repeat_interleave(N // 8, dim=1)
    u = z * scale[:, :, None, None]
    a = 0.5 * u * (1 + torch.erf(u * RS2))
    mm = lambda W, t: torch.einsum("oc,bcft->boft", d(W).reshape(W.shape[0], W.shape[1]), t)
    y = RS2 * gate[:, :, None, None] * mm(w["H"], a) + RS2 * z
    if head:
        out = RS2 * mm(w["res_conv"], z) + RS2 * mm(w["proj_out"], y)
        return out if add is None else RS2 * out + RS2 * d(add)
    return RS2 * mm(w["res_conv"], d(x)) + RS2 * y


def _layerwise(blk, z, x, film, N, head, out, add=None):
    """The launches of UnetEngine.block_fwd for this block (and the decoder's add for a head) -> stats, scale."""
    from babe_amd import ops
    gate = film[:, 5 + N:5 + 2 * N].contiguous()
    a = torch.empty_like(z)
    stats, scale = ops.gn_scale_gelu(z, blk.gamma[0], film[:, 5:5 + N], a)
    zn = ops.conv2d(a, blk.H[0], torch.empty_like(z), res=z, oscale=gate, alpha=RS2, rbeta=RS2)
    if head:
        zo = ops.conv2d(zn, blk.proj_out, torch.empty(B, 2, F, T, device="cuda"))
        if add is None:
            ops.conv2d(z, blk.res_conv, out, res=zo, alpha=RS2, rbeta=RS2)
        else:
            o = ops.conv2d(z, blk.res_conv, torch.empty(B, 2, F, T, device="cuda"), res=zo, alpha=RS2, rbeta=RS2)
            out.copy_(add)
            ops.axpby(o, out, alpha=RS2, beta=RS2)
    else:
        ops.conv2d(x, blk.res_conv, out, res=zn, alpha=RS2, rbeta=RS2)
    return stats, scale


def _rel(a, ref):
    a = a.double().cpu()
    return float((a - ref).norm() / ref.norm())


def _check(tag, fused, layer, ref):
    ef, el = _rel(fused, ref), _rel(layer, ref)
    print(f"pw_block parity {tag}: fused {ef:.3e} layer-by-layer {el:.3e}")
    assert ef <= max(2 * el, 1e-6), (tag, ef, el)


@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("fold", [False, True])
def test_head_forward_against_float64(N, fold):
    from babe_amd import ops
    gen = torch.Generator().manual_seed(100 + N)
    w, blk = _block(N, True, gen)
    z, film = _inputs(N, True, gen)
    add = torch.randn(B, 2, F, T, generator=gen).cuda() if fold else None
    ref = _reference(w, z, None, film, N, True, add)
    out_l = torch.empty(B, 2, F, T, device="cuda")
    st_l, sc_l = _layerwise(blk, z, None, film, N, True, out_l, add)
    # the fused pass: into a fresh tensor, or in place into the running sum as the decoder does
    out_f = add.clone() if fold else torch.full((B, 2, F, T), float("nan"), device="cuda")
    ss = ops.pw_block_fwd(blk.c, z, film, film[:, 5 + N:5 + 2 * N].contiguous(), out_f, add=out_f if fold else None)
    assert ss is not None, "the rule refused a qualifying head"
    torch.cuda.synchronize()
    assert torch.equal(ss[0], st_l) and torch.equal(ss[1], sc_l)
    _check(f"head N={N} fold={int(fold)}", out_f, out_l, ref)


@pytest.mark.parametrize("N", WIDTHS)
def test_init_forward_against_float64(N):
    from babe_amd import ops
    gen = torch.Generator().manual_seed(200 + N)
    w, blk = _block(N, False, gen)
    x, film = _inputs(N, False, gen)
    z = ops.conv2d(x, blk.proj_in, torch.empty(B, N, F, T, device="cuda"))    # the caller's proj_in launch, shared by all three
    ref = _reference(w, z, x, film, N, False)
    # the output is a frequency sub-range of a wider tensor; what lies around it stays untouched
    wide_l = torch.full((B, N, F + 3, T), 7.0, device="cuda")
    wide_f = wide_l.clone()
    st_l, sc_l = _layerwise(blk, z, x, film, N, False, wide_l[:, :, 1:1 + F, :])
    ss = ops.pw_block_fwd(blk.c, z, film, film[:, 5 + N:5 + 2 * N].contiguous(), wide_f[:, :, 1:1 + F, :], x=x)
    assert ss is not None, "the rule refused a qualifying init block"
    torch.cuda.synchronize()
    assert torch.equal(ss[0], st_l) and torch.equal(ss[1], sc_l)
    assert bool((wide_f[:, :, :1] == 7.0).all()) and bool((wide_f[:, :, 1 + F:] == 7.0).all())
    _check(f"init N={N}", wide_f[:, :, 1:1 + F, :], wide_l[:, :, 1:1 + F, :], ref)


def test_rule_refuses_a_narrow_block_and_follows_the_switch():
    """N = 8 (the reduced networks' width) never qualifies; a qualifying block is refused, and nothing is launched, while the
    library's switch is off; training (parameter gradients wanted) and a block of a bf16 / bf16x3 network are refused too."""
    from babe_amd import ops
    from babe_amd._lib import dispatch_counts
    gen = torch.Generator().manual_seed(7)
    _, blk8 = _block(8, True, gen)
    z8, film8 = _inputs(8, True, gen)
    out = torch.empty(B, 2, F, T, device="cuda")
    assert ops.pw_block_fwd(blk8.c, z8, film8, film8[:, 13:21].contiguous(), out) is None
    _, blk = _block(64, True, gen)
    z, film = _inputs(64, True, gen)
    gate = film[:, 69:133].contiguous()
    assert ops.pw_block_fwd(blk.c, z, film, gate, out, train=True) is None
    assert ops.pw_block_fwd(blk.c, z, film, gate, out, precision="bf16x3") is None      # fp32 images inside a bf16x3 network
    prev = ops.pw_block_enable(False)
    try:
        dispatch_counts(reset=True)
        assert ops.pw_block_fwd(blk.c, z, film, gate, out) is None
        assert not any(dispatch_counts().values()), "a refused block launched"
        assert ops.pw_block_enable(True) is False
        assert ops.pw_block_fwd(blk.c, z, film, gate, out) is not None
    finally:
        ops.pw_block_enable(prev)
