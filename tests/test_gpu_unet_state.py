"""Plan and state of the Python-sequenced UNet engine (babe_amd/networks/unet_engine.py): UnetEngine.clone_state gives a second
handle with a _State of its own over the very same weight objects, so two evaluations interleaved on two handles equal, bit for
bit, the same evaluations run one after the other on a fresh engine - forward, input-VJP, parameter gradients, with and without
time attention.  And the launch tables of tests/golden/unet_launch_counts.json (make_unet_launch_counts_golden.py), recorded before
the state was split from the weights.  Needs a MI355X."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
B, T0 = 2, 16


def _recorder():
    spec = importlib.util.spec_from_file_location("make_unet_launch_counts_golden", os.path.join(G, "make_unet_launch_counts_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(autouse=True)
def python_sequencer(monkeypatch):
    """The forms the table was recorded with, whatever the environment selects: the Python sequencer, two launches per GroupNorm
    statistic."""
    from babe_amd.forms import FORMS
    monkeypatch.setattr(FORMS, "unet_c", False)
    monkeypatch.setattr(FORMS, "gn_fused", False)


def network(attention):
    """(device state dict, UnetEngine keyword arguments) of the reduced network, plain or with attention_layers [0,0,0,0,1,1,1,1]."""
    if not attention:
        return {k: v.cuda().float() for k, v in REC.small_sd().items()}, {}
    from tests.attention_weights import LAST_TWO, attention_dict, attention_sd
    ad = attention_dict()
    sd = attention_sd(REC.NS, REC.DILS, LAST_TWO, ad)
    return {k: v.cuda().float() for k, v in sd.items()}, dict(attention_layers=list(LAST_TWO), attention_dict=ad)


def engine(sd, kw):
    from babe_amd.networks.unet_engine import UnetEngine
    return UnetEngine(sd, REC.NS, REC.DILS, **kw)


def inputs(seed):
    """Two different evaluations (A, B): octave inputs, output gradients; the noise levels of all 2 B rows."""
    gen = torch.Generator().manual_seed(seed)
    shapes = [(B, 2, 64, T0 * 2 ** j) for j in range(7)]
    draw = lambda: [torch.randn(s, generator=gen).cuda() for s in shapes]
    return (draw(), draw()), (draw(), draw()), torch.linspace(-1.2, -0.3, 2 * B).reshape(2 * B, 1).cuda()


def evaluate(sd, kw, train, interleaved, seed=7):
    """The evaluations A and B, each forward then VJP: interleaved on a handle and its clone_state(), or one after the other on one
    fresh engine.  Returns every output, input gradient and (train) parameter gradient, and the handles."""
    from babe_amd.networks.unet_engine import ParamGrads
    (CA, CB), (gA, gB), cn = inputs(seed)
    e0 = engine(sd, kw)
    e1 = e0.clone_state() if interleaved else e0
    keep = [] if train else None
    film = e0.embed(cn, keep=keep)
    fA, fB = film[:B], film[B:]
    if interleaved:
        oA = e0.forward(CA, fA, train=train)
        oB = e1.forward(CB, fB, train=train)
        pg = ParamGrads.new(e0, 2 * B) if train else None
        dA = e0.vjp(gA, pg=pg.lane(0, B) if train else None)
        dB = e1.vjp(gB, pg=pg.lane(B, 2 * B) if train else None)
    else:
        oA = e0.forward(CA, fA, train=train)
        pg = ParamGrads.new(e0, 2 * B) if train else None
        dA = e0.vjp(gA, pg=pg.lane(0, B) if train else None)
        oB = e0.forward(CB, fB, train=train)
        dB = e0.vjp(gB, pg=pg.lane(B, 2 * B) if train else None)
    res = {f"{n}.{j}": t for n, ts in (("oA", oA), ("oB", oB), ("dA", dA), ("dB", dB)) for j, t in enumerate(ts)}
    if train:
        res.update({"grad." + k: v for k, v in e0.param_grads(pg, keep).items()})
    torch.cuda.synchronize()
    return res, e0, e1


@pytest.mark.parametrize("attention,train", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["plain", "train", "attention", "attention_train"])
def test_interleaved_handles_equal_sequential_evaluations(attention, train):
    sd, kw = network(attention)
    got, e0, e1 = evaluate(sd, kw, train, interleaved=True)
    want, _, _ = evaluate(sd, kw, train, interleaved=False)
    assert set(got) == set(want) and (not train or any(k.startswith("grad.") for k in got))
    assert not any(torch.equal(got[f"oA.{j}"], got[f"oB.{j}"]) for j in range(7))          # A and B differ
    for k in want:
        assert torch.isfinite(want[k]).all(), k
        assert torch.equal(got[k], want[k]), k
    # one set of weight objects, two states
    assert e1 is not e0 and e1._state is not e0._state
    for b0, b1 in zip(e0.blocks(), e1.blocks()):
        assert b0 is b1
    assert e1.main_blk[3].H[0] is e0.main_blk[3].H[0] and e1.film_idx is e0.film_idx and e1.packs is e0.packs
    assert all(pc0 is pc1 for pc0, pc1 in zip(e0.pyr_conv, e1.pyr_conv))
    if attention:
        assert e0.attn_blocks and e1.mid_blk.attn.qk is e0.mid_blk.attn.qk
    # the VJP consumed what the forward saved, in both states
    for e in (e0, e1):
        st = e._state
        assert st.hs is None and not any(r is not None for r in st.saved + st.attn + st.inp + st.zpo)


def test_refresh_through_one_handle_is_seen_by_the_other():
    sd, kw = network(False)
    e0 = engine(sd, kw)
    e1 = e0.clone_state()
    (CA, _), (gA, _), cn = inputs(9)
    before = e1.forward(CA, e1.embed(cn[:B]))
    e1.vjp(gA)
    conv_keys = {k for k, _ in e0.packs}
    sd2 = {k: (v * 1.25 if k in conv_keys else v + 0.1 if ".affine." in k and k.endswith(".bias") else v) for k, v in sd.items()}
    e0.refresh(sd2)
    fresh = engine(sd2, kw)
    film, film_fresh = e1.embed(cn[:B]), fresh.embed(cn[:B])
    assert torch.equal(film, film_fresh)
    got, want = e1.forward(CA, film) + e1.vjp(gA), fresh.forward(CA, film_fresh) + fresh.vjp(gA)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not any(torch.equal(a, b) for a, b in zip(before, got[:7]))                         # the new weights are in use


@pytest.fixture(scope="module")
def launch_table():
    with open(os.path.join(G, "unet_launch_counts.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("case", sorted(REC.CASES))
def test_launch_counts_equal_the_recorded_table(launch_table, case):
    """Every slot of _lib.dispatch_counts() after one forward plus VJP: one lane, two lanes, a training step, attention."""
    got = REC.CASES[case]()
    want = launch_table[case]
    assert sum(want.values()) > 500
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
