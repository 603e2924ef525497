"""Training a CQTDiff+ UNet WITH time-attention layers on the HIP path: every parameter gradient against the reference network's
own autograd (tests/golden/attention_train.npz, make_attention_train_golden.py), lane independence, the training step's forward
and input gradient against the sampler's path, the opt-in contract of set_trainable(attention=True), the refresh after an optimizer
step and one training.train_step.  Needs a MI355X."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
TOL = 2e-4            # the parameter-gradient bar of tests/test_gpu_unet_train.py


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(G, "attention_train.npz"))


@functools.lru_cache(maxsize=None)
def weights(fixture):
    from tests.attention_weights import fixture_sd
    return fixture_sd(fixture)


def make_net(fixture, sd=None):
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    from tests.attention_weights import FIXTURES
    Ns, fs, L, layers, adict = FIXTURES[fixture]
    args = default_args(sample_rate=fs, audio_len=L, Ns=Ns)
    args.network.attention_layers = list(layers)
    args.network.attention_dict = dict(adict)
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(weights(fixture) if sd is None else sd, strict=True)      # (copies: the cached weights stay as they are)
    return net, args


def golden_inputs(name):
    f = golden()
    B, L = int(f[name + ".B"]), int(f[name + ".L"])
    gen = torch.Generator().manual_seed(int(f[name + ".grad_seed"]))
    x = 0.1 * torch.randn(B, L, generator=gen)
    cn = torch.from_numpy(f[name + ".cnoise"])
    w = torch.randn(B, L, generator=gen)
    return x, cn, w


def hip_grads(net, x, cn, w, attention=True):
    net.set_trainable(True, attention=attention)
    for p in net.parameters():
        p.grad = None
    y = net(x.cuda(), cn.cuda())
    (y * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("name", ["a", "b"])
def test_attention_param_grads_vs_reference_fixture(name):
    """Per trainable tensor the norm and 4 projections (Gaussian directions; rank-1 directions u v^T for the qk weights), projection
    error relative to |g| |d|.  The key set is the reference's requires_grad set."""
    f = golden()
    x, cn, w = golden_inputs(name)
    net, _ = make_net(str(f[name + ".fixture"]))
    _, got = hip_grads(net, x, cn, w)
    keys = f[name + ".trainable"].tolist()
    assert set(got) == set(keys), sorted(set(got) ^ set(keys))
    assert any(k.endswith("attn_block.qk.weight") for k in keys)
    gd = torch.Generator().manual_seed(int(f[name + ".dir_seed"]))
    worst, worst_attn = ("", 0.0), ("", 0.0)
    bad = []
    for k, n_ref, p_ref in zip(keys, f[name + ".grad_norm"], f[name + ".grad_proj"]):
        g = got[k].double().cpu()
        if k.endswith("attn_block.qk.weight"):
            u = torch.randn(4, g.shape[0], generator=gd).double()
            v = torch.randn(4, g.shape[1], generator=gd).double()
            proj = torch.einsum("ko,oi,ki->k", u, g.reshape(g.shape[0], g.shape[1]), v)
            dn = float((u.norm(dim=1) * v.norm(dim=1)).max())
        else:
            d = torch.randn(4, g.numel(), generator=gd).double()
            proj = d @ g.reshape(-1)
            dn = float(d.norm(dim=1).max())
        en = abs(float(g.norm()) - float(n_ref)) / float(n_ref)
        ep = float((proj - torch.from_numpy(p_ref)).abs().max()) / (float(n_ref) * dn)
        e = max(en, ep)
        if e > worst[1]:
            worst = (k, e)
        if any(t in k for t in ("attn_block", ".norm2.", ".affine2.", ".gate2.")) and e > worst_attn[1]:
            worst_attn = (k, e)
        if not (en < TOL and ep < TOL):
            bad.append((k, en, ep))
    print(f"config {name}: worst relative error {worst[1]:.2e} ({worst[0]}), worst attention-branch tensor {worst_attn[1]:.2e} ({worst_attn[0]})")
    assert not bad, bad[:8]


def test_one_lane_and_two_lanes_give_bit_identical_grads():
    x, cn, w = golden_inputs("a")
    net2, _ = make_net("a")
    net2.MAX_LANES = 2
    y2, g2 = hip_grads(net2, x, cn, w)
    net1, _ = make_net("a")
    net1.MAX_LANES = 1
    y1, g1 = hip_grads(net1, x, cn, w)
    assert torch.equal(y1, y2)
    assert set(g1) == set(g2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    _, g2b = hip_grads(net2, x, cn, w)                     # run to run
    for k in g2:
        assert torch.equal(g2b[k], g2[k]), k


def test_training_step_forward_and_input_gradient_equal_the_samplers_path():
    x, cn, w = golden_inputs("a")
    net, _ = make_net("a")
    net.set_trainable(True, attention=True)
    xi = x.cuda().requires_grad_(True)
    y = net(xi, cn.cuda())
    (y * w.cuda()).sum().backward()
    assert all(p.grad is not None for k, p in net.named_parameters() if k.endswith("attn_block.qk.weight"))
    net.set_trainable(False)
    y0 = net.fwd_nograd(x.cuda(), cn.cuda())
    gx0 = net.vjp(w.cuda())
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), y0) and torch.equal(xi.grad, gx0)


def test_opt_in_contract():
    from babe_amd._lib import dispatch_counts
    from tests import test_gpu_unet_train as plain
    x, cn, w = golden_inputs("a")
    # attention network without the opt-in: the refusal stays
    net, _ = make_net("a")
    net.set_trainable(True)
    with pytest.raises(NotImplementedError):
        net(x[:1].cuda(), cn[:1].cuda())
    # nothing requires grad: a forward + VJP launches what a network that never trained launches, and gives the same bits
    fresh, _ = make_net("a")
    hip_grads(net, x, cn, w)
    net.set_trainable(False)
    res = []
    for n in (fresh, net):
        dispatch_counts(reset=True)
        xi = x.cuda().requires_grad_(True)
        y = n(xi, cn.cuda())
        gx, = torch.autograd.grad((y * w.cuda()).sum(), xi)
        torch.cuda.synchronize()
        res.append((dispatch_counts(reset=True), y.detach(), gx))
    assert res[0][0] == res[1][0] and sum(res[0][0].values()) > 0
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    # attention-free network: attention=True is a no-op
    xs, cs, ws = plain.inputs(2, plain.L_SMALL, seed=6)
    _, g0 = hip_grads(plain.make_net(), xs, cs, ws, attention=False)
    _, g1 = hip_grads(plain.make_net(), xs, cs, ws, attention=True)
    assert set(g0) == set(g1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_adam_step_then_forward_matches_fresh_network():
    """The refresh after an optimizer step reaches the attention branch's packed convs and its plain tensors (norm2.gamma, the
    relative-position table, affine2 / gate2 in the FiLM matrix): the next forward is that of a network built from the updated
    state_dict, and not the one before the step."""
    x, cn, w = golden_inputs("a")
    net, _ = make_net("a")
    net.set_trainable(True, attention=True)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    y_before, _ = hip_grads(net, x, cn, w)
    opt.step()
    with torch.no_grad():
        y = net(x.cuda(), cn.cuda())
    fresh, _ = make_net("a", sd={k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    with torch.no_grad():
        y_fresh = fresh(x.cuda(), cn.cuda())
    assert torch.equal(y, y_fresh)
    assert not torch.equal(y, y_before)


def test_train_step_with_edm_runs_on_an_attention_network():
    from babe_amd import training
    from babe_amd.diff_params.edm import EDM
    x, _, _ = golden_inputs("a")
    net, args = make_net("a")
    net.set_trainable(True, attention=True)
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    torch.manual_seed(3)
    loss, err, sigma = training.train_step(net, opt, EDM(args), lambda: x.cuda(), 1, lr=1e-4)
    assert torch.isfinite(loss) and float(loss) > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters() if p.requires_grad)
