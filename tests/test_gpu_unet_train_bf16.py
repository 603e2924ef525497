"""Mixed-precision training of the HIP CQTDiff+ UNet: set_trainable(True, wgrad='bf16') puts the UNet body's conv weight
gradients on the bf16-operand kernel (babe_conv_wgrad_bf16_rows) and leaves everything else where it was; with wgrad given a
precision='bf16' network trains as well.  Bars: tests/wgrad_bf16_cases.py's rounding model (2.4e-3 per weight gradient, 1e-2 =
4 x that), the fp32 training bar 2e-4 (tests/test_gpu_unet_train.py) and the bf16 input-VJP bar 6e-2 (RP_TOL of
tests/test_gpu_unet_full.py).  Needs a MI355X."""
import functools

import pytest
import torch

from tests.test_gpu_unet_train import L_SMALL, TOL, inputs, make_net, oracle_grads, rel, small_sd

pytestmark = pytest.mark.gpu
WG_TOL = 1e-2         # 4 x the rounding model of one weight gradient
RP_TOL = 6e-2         # tests/test_gpu_unet_full.py: the bf16 network's input-VJP bar


def hip_grads(net, x, cn, w, **trainable):
    net.set_trainable(True, **trainable)
    for p in net.parameters():
        p.grad = None
    xi = x.cuda().requires_grad_(True)
    y = net(xi, cn.cuda())
    (y * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), xi.grad.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.requires_grad}


@functools.lru_cache(maxsize=None)
def oracle_small():
    """float64 autograd gradients of the reduced-width network for inputs(2, L_SMALL): computed once, read only."""
    x, cn, w = inputs(2, L_SMALL)
    return oracle_grads(small_sd(), x, cn, w, L_SMALL, 22050)


def is_conv_weight(k, v):
    return v.dim() == 4 and k.endswith(".weight")


def test_f32_network_wgrad_bf16_vs_f32_and_oracle():
    net = make_net()
    x, cn, w = inputs(2, L_SMALL)
    y32, gx32, g32 = hip_grads(net, x, cn, w, wgrad="f32")
    y16, gx16, g16 = hip_grads(net, x, cn, w, wgrad="bf16")
    assert torch.equal(y32, y16) and torch.equal(gx32, gx16)       # forward and input-VJP are untouched
    assert set(g32) == set(g16)
    want = oracle_small()
    assert set(want) == set(g16)
    nconv = 0
    for k in sorted(g16):
        d, e = rel(g16[k], g32[k]), rel(g16[k], want[k])
        print(f"{k}: bf16 vs f32 weight gradients {d:.3e}, vs float64 {e:.3e}")
    for k in g16:
        d = rel(g16[k], g32[k])
        if k.endswith(".gamma"):
            assert torch.equal(g16[k], g32[k]), k
        elif is_conv_weight(k, g16[k]):
            nconv += 1
            assert 1e-5 < d < WG_TOL, (k, d)
        else:
            assert d < WG_TOL, (k, d)
        assert rel(g16[k], want[k]) < WG_TOL + TOL, k
    assert nconv > 50


def test_wgrad_none_is_f32_and_bad_value_raises():
    net = make_net()
    x, cn, w = inputs(2, L_SMALL, seed=2)
    _, gx0, g0 = hip_grads(net, x, cn, w)
    _, gx1, g1 = hip_grads(net, x, cn, w, wgrad="f32")
    assert torch.equal(gx0, gx1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    with pytest.raises(ValueError):
        net.set_trainable(True, wgrad="fp16")


def test_lanes_and_run_to_run_bit_identical_under_bf16():
    x, cn, w = inputs(2, L_SMALL, seed=1)
    net = make_net()
    net.MAX_LANES = 2
    y2, gx2, g2 = hip_grads(net, x, cn, w, wgrad="bf16")
    net1 = make_net()
    net1.MAX_LANES = 1
    y1, gx1, g1 = hip_grads(net1, x, cn, w, wgrad="bf16")
    assert torch.equal(y1, y2) and torch.equal(gx1, gx2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    _, _, g2b = hip_grads(net, x, cn, w, wgrad="bf16")                # run to run
    for k in g2:
        assert torch.equal(g2b[k], g2[k]), k


def test_bf16_network_trains_once_wgrad_is_given():
    """precision='bf16': forward and input-VJP on the bf16 conv kernels, weight gradients from the fp32 activations the forward
    saved.  Measured per tensor on the MI355X: see DESIGN.md, "Mixed-precision training"."""
    x, cn, w = inputs(2, L_SMALL)
    net = make_net(precision="bf16")
    net.set_trainable(True)
    with pytest.raises(NotImplementedError):
        net(x.cuda(), cn.cuda())
    want = oracle_small()
    _, _, g32 = hip_grads(net, x, cn, w, wgrad="f32")
    _, _, g16 = hip_grads(net, x, cn, w, wgrad="bf16")
    assert set(g32) == set(want) == set(g16)
    keys = sorted(want)
    cat = lambda d: torch.cat([d[k].detach().double().cpu().reshape(-1) for k in keys])
    e32 = {k: rel(g32[k], want[k]) for k in keys}
    e16 = {k: rel(g16[k], want[k]) for k in keys}
    for k in keys:
        print(f"{k}: bf16 network vs float64, wgrad f32 {e32[k]:.3e}, wgrad bf16 {e16[k]:.3e}")
    whole32, whole16 = rel(cat(g32), cat(want)), rel(cat(g16), cat(want))
    print(f"whole gradient vector: wgrad f32 {whole32:.3e}, wgrad bf16 {whole16:.3e}")
    assert whole32 < RP_TOL
    for k in keys:
        assert e16[k] <= e32[k] + WG_TOL, (k, e16[k], e32[k])


def test_sgd_step_lowers_loss_first_order_bf16():
    from babe_amd.config import default_args
    from babe_amd.diff_params.edm import EDM
    args = default_args(sample_rate=22050, audio_len=L_SMALL, Ns=[8, 8, 8, 8, 16, 16, 16])
    edm = EDM(args)
    net = make_net()
    net.set_trainable(True, wgrad="bf16")
    x, _, _ = inputs(2, L_SMALL, seed=5)
    x = x.cuda()

    def loss():
        torch.manual_seed(7)
        return edm.loss_fn(net, x)[0].mean()

    l0 = loss()
    l0.backward()
    gn2 = sum(float((p.grad.double() ** 2).sum()) for p in net.parameters() if p.grad is not None)
    lr = 1e-3 / gn2 ** 0.5 * float(l0.detach())
    with torch.no_grad():
        for p in net.parameters():
            if p.grad is not None:
                p -= lr * p.grad
        l1 = loss()
    want = lr * gn2
    print(f"loss {float(l0):.6g} -> {float(l1):.6g}: decrease {float(l0 - l1):.4g}, predicted {want:.4g}")
    assert float(l0 - l1) > 0 and abs(float(l0 - l1) - want) < 0.2 * want


def test_full_width_L46046_wgrad_bf16_vs_f32():
    """The 256-channel tiles and dilation 64."""
    from tests.golden_weights import FULL_NS, full_width_sd
    L = 46046
    net = make_net(full_width_sd(0), Ns=FULL_NS, L=L, fs=44100)
    x, cn, w = inputs(1, L, seed=3)
    _, _, g32 = hip_grads(net, x, cn, w, wgrad="f32")
    _, _, g16 = hip_grads(net, x, cn, w, wgrad="bf16")
    errs = {k: rel(g16[k], g32[k]) for k in g32 if is_conv_weight(k, g32[k])}
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    print("worst conv weight gradients, bf16 vs f32:", worst)
    assert len(errs) > 50 and all(1e-5 < e < WG_TOL for e in errs.values()), worst
