"""Training a CQTDiff+ UNet whose time-attention core runs on bf16 MFMA (attention_precision='bf16') under
set_trainable(True, attention='bf16'): the opt-in's contract, every parameter gradient against the same network on the fp32 core
(which tests/test_gpu_unet_attention_train.py pins to the reference), the training step's forward and input gradient against the
sampler's path, lane independence, the qk weight gradient under wgrad='bf16', and one optimizer step of each kind.  Fixtures
"a" and "b" of tests/attention_weights.py, inputs of tests/golden/attention_train.npz; bars and measurements:
tests/attention_bf16_train_cases.py.  Needs a MI355X."""
import functools

import pytest
import torch

from tests import attention_bf16_train_cases as C
from tests.test_gpu_unet_attention_bf16 import make_net
from tests.test_gpu_unet_attention_train import golden, golden_inputs
from tests.test_gpu_unet_train_bf16 import WG_TOL

pytestmark = pytest.mark.gpu
QK = "attn_block.qk.weight"


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def fixture_of(name):
    return str(golden()[name + ".fixture"])


def grads(net, name, **trainable):
    """(y, gx, {key: gradient}) of one training step's forward / backward on the golden inputs of `name`."""
    x, cn, w = golden_inputs(name)
    net.set_trainable(True, **trainable)
    for p in net.parameters():
        p.grad = None
    xi = x.cuda().requires_grad_(True)
    y = net(xi, cn.cuda())
    (y * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), xi.grad.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.requires_grad}


@functools.lru_cache(maxsize=None)
def fp32_core_grads(name):
    """The parameter gradients of the f32 network on the fp32 core: computed once per fixture and left unchanged."""
    return grads(make_net(fixture_of(name))[0], name, attention=True)[2]


def test_opt_in_contract():
    from babe_amd._lib import dispatch_counts
    from tests import test_gpu_unet_train as plain
    net, _ = make_net("a", "f32", "bf16")
    with pytest.raises(NotImplementedError, match="attention_precision"):      # True keeps promising the 2e-4 gradients
        net.set_trainable(True, attention=True)
    with pytest.raises(NotImplementedError):                                     # 'bf16' is for a bf16 core
        make_net("a")[0].set_trainable(True, attention="bf16")
    with pytest.raises(NotImplementedError):
        make_net("a", "bf16", "f32")[0].set_trainable(True, attention="bf16", wgrad="bf16")
    for bad in ("f32", "fp16", 1, None):
        with pytest.raises(ValueError):
            net.set_trainable(True, attention=bad)
    # attention-free network: 'bf16' does nothing, like True
    xs, cs, ws = plain.inputs(2, plain.L_SMALL, seed=6)
    res = []
    for att in (False, "bf16"):
        p = plain.make_net()
        p.set_trainable(True, attention=att)
        y = p(xs.cuda(), cs.cuda())
        (y * ws.cuda()).sum().backward()
        res.append({k: q.grad.clone() for k, q in p.named_parameters() if q.requires_grad})
    assert set(res[0]) == set(res[1]) and all(torch.equal(res[0][k], res[1][k]) for k in res[0])
    # after set_trainable(False): the bits and the dispatch counts of a network that never trained
    x, cn, w = golden_inputs("a")
    fresh, _ = make_net("a", "f32", "bf16")
    grads(net, "a", attention="bf16")
    net.set_trainable(False)
    out = []
    for n in (fresh, net):
        dispatch_counts(reset=True)
        xi = x.cuda().requires_grad_(True)
        y = n(xi, cn.cuda())
        gx, = torch.autograd.grad((y * w.cuda()).sum(), xi)
        torch.cuda.synchronize()
        out.append((dispatch_counts(reset=True), y.detach(), gx))
    assert out[0][0] == out[1][0] and sum(out[0][0].values()) > 0
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])


@pytest.mark.parametrize("name", ["a", "b"])
def test_param_grads_on_the_bf16_core_vs_the_fp32_core(name):
    """f32 network, bf16 core, attention='bf16': every gradient finite and within the measured bars of the fp32 core's; the
    training step's forward and input gradient are the sampler's fwd_nograd / vjp bit for bit."""
    want = fp32_core_grads(name)
    net, _ = make_net(fixture_of(name), "f32", "bf16")
    y, gx, got = grads(net, name, attention="bf16")
    assert set(got) == set(want) and any(k.endswith(QK) for k in got)
    assert all(torch.isfinite(g).all() for g in got.values())
    keys = sorted(want)
    errs = {k: rel(got[k], want[k]) for k in keys}
    for k in keys:
        print(f"{name} {k}: bf16 core vs fp32 core {errs[k]:.3e}")
    for k in keys:                                                # the two halves of the qk rows: queries, then keys, per head
        if ".attn_block.qk." in k:
            g, r = (t.double().reshape(8, 2, -1) for t in (got[k], want[k]))
            n = float(r.norm())
            print(f"{name} {k}: Q rows {float((g[:, 0] - r[:, 0]).norm()) / n:.3e}, K rows {float((g[:, 1] - r[:, 1]).norm()) / n:.3e} "
                  f"of |g|; |K rows| / |g|: fp32 core {float(r[:, 1].norm()) / n:.3e}, bf16 core {float(g[:, 1].norm()) / n:.3e}")
    cat = lambda d: torch.cat([d[k].double().reshape(-1) for k in keys])
    whole = rel(cat(got), cat(want))
    worst = max(errs, key=errs.get)
    print(f"fixture {name}: worst key {worst} {errs[worst]:.3e}, whole gradient {whole:.3e}")
    over = {k: e for k, e in errs.items() if e > C.NET_FINDING}
    assert all(k.endswith(C.NET_FINDING_KEYS) for k in over), over          # the explained finding: gradients of the qk Conv1d
    assert errs[worst] <= C.NET_BAR_KEY and whole <= C.NET_BAR_WHOLE
    for k in keys:                                                # the key half of the qk bias gradient is zero mathematically
        if k.endswith("attn_block.qk.bias"):
            r = want[k].double().reshape(8, 2, -1)
            assert float(r[:, 1].norm()) < 1e-4 * float(r.norm()), k
    x, cn, w = golden_inputs(name)
    net.set_trainable(False)
    y0 = net.fwd_nograd(x.cuda(), cn.cuda())
    gx0 = net.vjp(w.cuda())
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and torch.equal(gx, gx0)


def test_one_lane_and_two_lanes_give_bit_identical_grads(monkeypatch):
    monkeypatch.setenv("BABE_BF16_LANES", "1")                     # a bf16 core keeps one stream unless the host opts in
    net2, _ = make_net("a", "f32", "bf16")
    net2.MAX_LANES = 2
    assert net2._get_lanes(2) is not None and len(net2._get_lanes(2)) == 2
    y2, gx2, g2 = grads(net2, "a", attention="bf16")
    net1, _ = make_net("a", "f32", "bf16")
    net1.MAX_LANES = 1
    assert net1._get_lanes(2) is None
    y1, gx1, g1 = grads(net1, "a", attention="bf16")
    assert torch.equal(y1, y2) and torch.equal(gx1, gx2) and set(g1) == set(g2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    _, _, g2b = grads(net2, "a", attention="bf16")                # run to run
    for k in g2:
        assert torch.equal(g2b[k], g2[k]), k


def test_qk_weight_gradient_follows_wgrad_on_the_bf16_core_only():
    """precision='bf16' network: under attention='bf16' the qk weight gradients move from babe_attn_qk_wgrad to
    babe_attn_qk_wgrad_bf16 with wgrad; on the fp32 core of the same network wgrad leaves them where they were."""
    net, _ = make_net("a", "bf16", "bf16")
    _, _, g32 = grads(net, "a", attention="bf16", wgrad="f32")
    _, _, g16 = grads(net, "a", attention="bf16", wgrad="bf16")
    _, _, g16x = grads(net, "a", attention="bf16", wgrad="f32")    # back again: the knob is per step
    nqk = 0
    for k in g32:
        assert torch.equal(g32[k], g16x[k]), k
        if k.endswith(QK):
            nqk += 1
            d = rel(g16[k], g32[k])
            print(f"{k}: qk weight gradient, wgrad bf16 vs f32 {d:.3e}")
            assert 1e-5 < d < WG_TOL, (k, d)
    assert nqk == 7                                               # LAST_TWO: three octaves down, the bottleneck, three up
    # the conv weight gradients follow wgrad as they always did; with those held at fp32 the two steps differ in the qk weight
    # gradients alone: every other key is unchanged bit for bit
    eng = net.engine()
    orig = eng._wg
    eng._wg = lambda pg, *a, **kw: orig(pg, *a, **{**kw, "precision": "f32"})
    try:
        _, _, gq = grads(net, "a", attention="bf16", wgrad="bf16")
    finally:
        del eng._wg
    for k in g32:
        if k.endswith(QK):
            assert torch.equal(gq[k], g16[k]), k
        else:
            assert torch.equal(gq[k], g32[k]), k
    core32, _ = make_net("a", "bf16", "f32")
    _, _, h32 = grads(core32, "a", attention=True, wgrad="f32")
    _, _, h16 = grads(core32, "a", attention=True, wgrad="bf16")
    for k in h32:
        if k.endswith(QK):
            assert torch.equal(h32[k], h16[k]), k


@pytest.mark.parametrize("fused", [False, True])
def test_train_step_then_forward_matches_fresh_network(fused):
    from babe_amd import training
    from babe_amd.diff_params.edm import EDM
    from babe_amd.optim import FusedAdamEMA
    x, cn, _ = golden_inputs("a")
    net, args = make_net("a", "bf16", "bf16")
    net.set_trainable(True, attention="bf16", wgrad="bf16")
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    opt = (FusedAdamEMA if fused else torch.optim.Adam)(net.parameters(), lr=1e-4)
    torch.manual_seed(3)
    loss, err, sigma = training.train_step(net, opt, EDM(args), lambda: x.cuda(), 1, lr=1e-4)
    assert torch.isfinite(loss) and float(loss) > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters() if p.requires_grad)
    after = net.state_dict()
    moved = [k for k, p in net.named_parameters() if p.requires_grad and not torch.equal(before[k], after[k])]
    assert any(k.endswith(QK) for k in moved) and any("relative_attention_bias" in k for k in moved)
    with torch.no_grad():
        y = net(x.cuda(), cn.cuda())
    fresh, _ = make_net("a", "bf16", "bf16")
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in after.items()}, strict=True)
    with torch.no_grad():
        y_fresh = fresh(x.cuda(), cn.cuda())
    assert torch.isfinite(y).all() and torch.equal(y, y_fresh)
