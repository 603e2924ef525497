"""Time-attention networks on the library-side UNet sequencer (csrc/unet_engine.hip with a babe_unet_attn per attention block,
CUnet(eng, attention=True)) against the Python-sequenced engine (UnetEngine.attn_fwd / attn_vjp): the same kernels in the same
order, so forward and input-VJP are IDENTICAL bit for bit, on the fp32 and the bf16 attention core, in an fp32 and a bf16 network;
and the relative-position bucket table the sequencer builds on the device (csrc/attn_buckets.hip).  Pattern of
tests/test_gpu_unet_c.py.  Needs a MI355X."""
import ctypes as C
import functools

import pytest
import torch

from tests.attention_weights import LAST_TWO, SMALL_DILS, SMALL_NS, attention_dict, attention_sd

pytestmark = pytest.mark.gpu

# (attention_layers, attention_dict): the table without a bias on the last two octaves and the bottleneck; the bias without a
# table on every level
LAYOUTS = {"last_two": (LAST_TWO, attention_dict()), "all": ([1] * 8, attention_dict(use_rel_pos=False, bias_qkv=True))}
# (network precision, attention core)
ARITH = [("f32", "f32"), ("f32", "bf16"), ("bf16", "bf16")]


@functools.lru_cache(maxsize=None)
def _sd(layout, zero_gate2=False):
    layers, adict = LAYOUTS[layout]
    sd = attention_sd(SMALL_NS, SMALL_DILS, layers, adict)
    if zero_gate2:
        sd = {k: (torch.zeros_like(v) if ".gate2." in k else v) for k, v in sd.items()}
    return {k: v.cuda() for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _engine(layout, precision, core, zero_gate2=False):
    """One engine per configuration for the whole file (never modified): the Python sequencer and the library plan share its
    packed weights."""
    from babe_amd.networks.unet_engine import UnetEngine
    layers, adict = LAYOUTS[layout]
    return UnetEngine(_sd(layout, zero_gate2), SMALL_NS, SMALL_DILS, precision=precision, attention_layers=layers, attention_dict=adict,
                      attention_precision=core)


def _case(B, T0, seed=5):
    """C_list[j] = [B, 2, 64, T0 * 2^j], a cotangent of the same shapes, noise levels.  T0 = 20 puts the three deep attention
    levels at T = 80, 40, 20 (F = 320, 384, 448): no multiple of the 16-row fp32 or the 32-row bf16 tiles."""
    gen = torch.Generator().manual_seed(seed + B)
    C_list = [torch.randn(B, 2, 64, T0 * 2 ** j, generator=gen).cuda() for j in range(7)]
    gouts = [torch.randn(c.shape, generator=gen).cuda() for c in C_list]
    cn = torch.linspace(-1.2, -0.3, B).reshape(B, 1).cuda()
    return C_list, gouts, cn


def _python(eng, C_list, film, gouts):
    outs = eng.forward(C_list, film)
    assert not eng._state.c_fwd                                  # the Python sequencer ran
    gC = eng.vjp(gouts)
    torch.cuda.synchronize()
    return outs + gC


def _library(cu, C_list, film, gouts):
    res = cu.fwd(C_list, film) + cu.vjp(gouts)
    torch.cuda.synchronize()
    return res


def _assert_equal(want, got):
    assert len(want) == len(got) == 14
    for a, b in zip(want, got):
        assert a.shape == b.shape and torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b), float((a - b).abs().max())


@pytest.mark.parametrize("precision,core", ARITH)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("B,T0", [(2, 20), (1, 16)])
def test_library_sequencer_equals_python_sequencer(monkeypatch, B, T0, layout, precision, core):
    from babe_amd.forms import FORMS
    from babe_amd.networks.unet_c import CUnet
    monkeypatch.setattr(FORMS, "unet_c", False)
    eng = _engine(layout, precision, core)
    assert eng.has_attention and eng.attn_core == core and eng._c_engine() is None
    C_list, gouts, cn = _case(B, T0)
    film = eng.embed(cn)
    want = _python(eng, C_list, film, gouts)
    cu = CUnet(eng, attention=True)
    _assert_equal(want, _library(cu, C_list, film, gouts))


def test_without_the_argument_an_attention_engine_is_refused_as_before():
    from babe_amd.networks.unet_c import CUnet
    from babe_amd.networks.unet_engine import UnetEngine
    layers, adict = LAYOUTS["last_two"]
    eng = UnetEngine(_sd("last_two"), SMALL_NS, SMALL_DILS, attention_layers=layers, attention_dict=adict)
    for make in (lambda: CUnet(eng), lambda: eng.c_plan()):
        with pytest.raises(NotImplementedError, match="does not support time-attention layers"):
            make()
    assert eng.c_plan(attention=True)


def test_second_evaluation_and_two_states_on_two_streams(monkeypatch):
    """A second evaluation through the same state and workspace (other inputs), then two states over one plan on two streams."""
    from babe_amd.forms import FORMS
    from babe_amd.networks.unet_c import CUnet
    monkeypatch.setattr(FORMS, "unet_c", False)
    eng = _engine("last_two", "f32", "f32")
    C_list, gouts, cn = _case(2, 20)
    C2 = [c * 0.5 + 0.1 for c in C_list]
    film = eng.embed(cn)
    want1, want2 = _python(eng, C_list, film, gouts), _python(eng, C2, film, gouts)
    cu = CUnet(eng, attention=True)
    _assert_equal(want1, _library(cu, C_list, film, gouts))
    _assert_equal(want2, _library(cu, C2, film, gouts))
    lane = CUnet(eng, attention=True)
    assert lane.plan == cu.plan and lane.state != cu.state
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        oa = cu.fwd(C_list, film)
    with torch.cuda.stream(s2):
        ob = lane.fwd(C2, film)
    with torch.cuda.stream(s1):
        ga = cu.vjp(gouts)
    with torch.cuda.stream(s2):
        gb = lane.vjp(gouts)
    torch.cuda.synchronize()
    _assert_equal(want1, oa + ga)
    _assert_equal(want2, ob + gb)


def test_the_attention_branch_is_in_the_library_outputs():
    """With every gate2 tensor zero the branch contributes nothing: the library's outputs differ from those with the fixture's O(1)
    gates, so the equality above is not one of two networks that both skip the branch."""
    from babe_amd.networks.unet_c import CUnet
    C_list, gouts, cn = _case(2, 20)
    res = []
    for zero in (False, True):
        eng = _engine("last_two", "f32", "f32", zero)
        res.append(_library(CUnet(eng, attention=True), C_list, eng.embed(cn), gouts))
    for name, a, b in zip(["out"] * 7 + ["vjp"] * 7, *res):
        rel = float((a - b).abs().max() / a.abs().max())
        print(f"gate2 zeroed, {name} {tuple(a.shape)}: relative difference {rel:.3e}")
        assert not torch.equal(a, b)


def test_workspace_bytes_suffices_and_one_granule_less_does_not():
    from babe_amd._lib import lib
    from babe_amd.networks.unet_c import CUnet
    L = lib()
    eng = _engine("last_two", "f32", "f32")
    cu = CUnet(eng, attention=True)
    C_list, gouts, cn = _case(2, 20)
    film = eng.embed(cn)
    want = _library(cu, C_list, film, gouts)
    P = C.c_void_p
    T_oct = (C.c_int * 7)(*[c.shape[-1] for c in C_list])
    n = L.babe_unet_workspace_bytes(cu.plan, 2, T_oct)
    assert n > 0 and n % 256 == 0

    def run(nbytes):
        ws = torch.empty(n, device="cuda", dtype=torch.uint8)                    # (the full size is there: only `nbytes` is offered)
        outs, gC = [torch.empty_like(c) for c in C_list], [torch.empty_like(c) for c in C_list]
        ptrs = lambda ts: (P * 7)(*[t.data_ptr() for t in ts])
        rc = L.babe_unet_fwd(cu.plan, cu.state, ptrs(C_list), film.data_ptr(), film.stride(0), 2, T_oct, ws.data_ptr(), nbytes, ptrs(outs), None)
        if rc == 0:
            rc = L.babe_unet_vjp(cu.plan, cu.state, ptrs(gouts), ptrs(gC), None)
        msg = L.babe_last_error()
        torch.cuda.synchronize()
        return rc, msg, outs + gC

    rc, msg, got = run(n)
    assert rc == 0, msg
    _assert_equal(want, got)
    rc, msg, _ = run(n - 256)
    assert rc != 0 and b"workspace too small" in msg, (rc, msg)


def test_plan_create_refuses_the_attention_descriptor_without_a_core(monkeypatch):
    """The engine's own descriptor with attn_core = 0: refused before any launch, the message names the field."""
    from babe_amd.networks import unet_c
    eng = _engine("last_two", "f32", "f32")
    monkeypatch.setattr(unet_c, "ATTN_CORES", {"f32": 0, "bf16": 0})
    with pytest.raises(RuntimeError, match="attn_core = 0"):
        unet_c.CPlan().get(eng, attention=True)


@pytest.mark.parametrize("nb,maxd", [(32, 64), (8, 16)])
def test_device_bucket_table_equals_the_host_table(nb, maxd):
    """babe_attn_bucket_table (the kernel the sequencer launches once per distinct time length) = ops.attn_buckets entry for
    entry; the entries around the table stay untouched."""
    from babe_amd import ops
    from babe_amd._cabi import AttnBucketThr
    from babe_amd._lib import check, lib, stream
    thr = AttnBucketThr()
    check(lib().babe_attn_bucket_thresholds(C.byref(thr), nb, maxd), "attn_bucket_thresholds")
    for T in (1, 2, 9, 20, 63, 64, 65, 300):
        n = 2 * T - 1
        buf = torch.full((n + 64,), -7, device="cuda", dtype=torch.int32)
        check(lib().babe_attn_bucket_table(C.byref(thr), T, buf.data_ptr() + 32 * 4, stream()), "attn_bucket_table")
        torch.cuda.synchronize()
        got = buf.cpu()
        assert torch.equal(got[32:32 + n], ops.attn_buckets(T, nb, maxd)), T
        assert (got[:32] == -7).all() and (got[32 + n:] == -7).all(), T
