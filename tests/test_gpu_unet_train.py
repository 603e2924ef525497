"""Training path of the HIP CQTDiff+ UNet: every parameter gradient of <net(x, cnoise), w> against float64 autograd through the
oracle (oracle/unet.py), lane / sequencer independence, the opt-in contract (nothing changes while no parameter requires grad),
the repack after an optimizer step, a first-order loss check and the refusals.  Needs a MI355X."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
CFG = dict(num_octs=7, bins_per_oct=64, num_dils=[2, 3, 4, 5, 6, 7, 7])
L_SMALL = 92092
TOL = 2e-4            # the input-VJP bar (tests/test_gpu_sampler.py)


def small_sd():
    u = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(G, "unet_small.npz")).items()}
    return {k[3:]: v for k, v in u.items() if k.startswith("sd.")}


def make_net(sd=None, Ns=(8, 8, 8, 8, 16, 16, 16), L=L_SMALL, fs=22050, **kw):
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    args = default_args(sample_rate=fs, audio_len=L, Ns=list(Ns))
    for k, v in kw.items():
        args.network[k] = v
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(small_sd() if sd is None else sd, strict=True)
    return net


def inputs(B, L, seed=0):
    gen = torch.Generator().manual_seed(seed)
    x = 0.1 * torch.randn(B, L, generator=gen)
    cn = torch.linspace(-0.4, 0.3, B).reshape(B, 1)
    w = torch.randn(B, L, generator=gen)
    return x, cn, w


def hip_grads(net, x, cn, w):
    net.set_trainable(True)
    for p in net.parameters():
        p.grad = None
    y = net(x.cuda(), cn.cuda())
    (y * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.requires_grad}


def oracle_grads(sd, x, cn, w, L, fs):
    """float64 autograd through oracle.unet's body (the CQT itself in fp32, it has no parameters)."""
    from oracle import unet as UN
    from oracle.nsgt import CQT_nsgt
    sd64 = {k: v.detach().double().requires_grad_(not k.endswith(".kernel") and k != "embedding.RFF_freq") for k, v in sd.items()}
    cqt = CQT_nsgt(7, 64, "oct", ("kaiser", 1), fs, L)
    with torch.no_grad():
        C = [torch.view_as_real(c.squeeze(1)).permute(0, 3, 1, 2).contiguous().double() for c in cqt.fwd(x.unsqueeze(1))]
    outs = UN.unet_body(sd64, CFG, C, UN.embedding(sd64, cn.double()))
    O = [torch.view_as_complex(o.float().permute(0, 2, 3, 1).contiguous()).unsqueeze(1) for o in outs]
    y = cqt.bwd(O).squeeze(1)[:, :L]
    keys = [k for k, v in sd64.items() if v.requires_grad]
    gr = torch.autograd.grad((y.double() * w.double()).sum(), [sd64[k] for k in keys])
    return dict(zip(keys, gr))


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def check_all(got, want, tol):
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    errs = {k: rel(got[k], want[k]) for k in want}
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    print("worst per-tensor relative errors:", worst)
    assert all(e < tol for e in errs.values()), worst


def test_reduced_width_param_grads_vs_oracle_float64():
    sd = small_sd()
    net = make_net(sd)
    x, cn, w = inputs(2, L_SMALL)
    _, got = hip_grads(net, x, cn, w)
    want = oracle_grads(sd, x, cn, w, L_SMALL, 22050)
    check_all(got, want, TOL)


def test_reduced_width_param_grads_vs_reference_fixture():
    """The reference network's own gradients (tests/golden/train.npz, make_train_golden.py): per-tensor norm and the projections
    onto 4 seeded Gaussian directions, at the 2e-4 bar (projection error relative to |g| |d|)."""
    f = np.load(os.path.join(G, "train.npz"))
    gen = torch.Generator().manual_seed(int(f["grad_seed"]))
    x = 0.1 * torch.randn(2, L_SMALL, generator=gen)
    cn = torch.from_numpy(f["grad_cnoise"])
    w = torch.randn(2, L_SMALL, generator=gen)
    _, got = hip_grads(make_net(), x, cn, w)
    keys = f["trainable"].tolist()
    assert set(got) == set(keys)
    gd = torch.Generator().manual_seed(int(f["dir_seed"]))
    worst = 0.0
    for k, n_ref, p_ref in zip(keys, f["grad_norm"], f["grad_proj"]):
        g = got[k].double().cpu().reshape(-1)
        d = torch.randn(4, g.numel(), generator=gd).double()
        en = abs(float(g.norm()) - float(n_ref)) / float(n_ref)
        ep = float(((d @ g) - torch.from_numpy(p_ref)).abs().max()) / (float(n_ref) * float(d.norm(dim=1).max()))
        worst = max(worst, en, ep)
        assert en < TOL and ep < TOL, (k, en, ep)
    print(f"worst relative error vs the reference fixture: {worst:.2e}")


def test_full_width_L46046_param_grads_vs_oracle_with_f45_dispatch():
    from babe_amd._lib import dispatch_counts
    from tests.golden_weights import FULL_NS, full_width_sd
    sd = full_width_sd(0)
    L = 46046
    net = make_net(sd, Ns=FULL_NS, L=L, fs=44100)
    x, cn, w = inputs(1, L, seed=3)
    dispatch_counts(reset=True)
    _, got = hip_grads(net, x, cn, w)
    c = dispatch_counts(reset=True)
    want = oracle_grads(sd, x, cn, w, L, 44100)
    check_all(got, want, TOL)
    assert c["conv53_wino85"] > 0 and c["conv_bf16"] == 0, c


def test_two_lanes_and_c_sequencer_give_bit_identical_grads(monkeypatch):
    x, cn, w = inputs(2, L_SMALL, seed=1)
    net = make_net()
    net.MAX_LANES = 2
    y2, g2 = hip_grads(net, x, cn, w)
    net1 = make_net()
    net1.MAX_LANES = 1
    y1, g1 = hip_grads(net1, x, cn, w)
    assert torch.equal(y1, y2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    from babe_amd.forms import FORMS
    monkeypatch.setattr(FORMS, "unet_c", True)
    netc = make_net()
    yc, gc = hip_grads(netc, x, cn, w)
    for k in g1:
        assert torch.equal(g1[k], gc[k]), k
    _, g2b = hip_grads(net, x, cn, w)                     # run to run
    for k in g1:
        assert torch.equal(g2b[k], g2[k]), k


def test_no_param_grad_changes_nothing():
    x, cn, w = inputs(2, L_SMALL, seed=2)
    ref = make_net()
    trained = make_net()
    trained.set_trainable(True)
    hip_grads(trained, x, cn, w)                          # a training step's forward/backward, no update
    trained.set_trainable(False)
    for net in (ref, trained):
        xi = x.cuda().requires_grad_(True)
        y = net(xi, cn.cuda())
        gx, = torch.autograd.grad((y * w.cuda()).sum(), xi)
        net._res = (y.detach(), gx)
        assert all(p.grad is None or net is trained for p in net.parameters())
    assert all(p.grad is None for p in ref.parameters())
    assert torch.equal(ref._res[0], trained._res[0]) and torch.equal(ref._res[1], trained._res[1])


def test_adam_step_then_forward_matches_fresh_network():
    x, cn, w = inputs(2, L_SMALL, seed=4)
    net = make_net()
    net.set_trainable(True)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    hip_grads(net, x, cn, w)
    opt.step()
    with torch.no_grad():
        y = net(x.cuda(), cn.cuda())
    fresh = make_net({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    with torch.no_grad():
        y_fresh = fresh(x.cuda(), cn.cuda())
    assert torch.equal(y, y_fresh)
    # the input-VJP and the parameter gradients (transposed images, Wcat) after the step as well
    _, g_net = hip_grads(net, x, cn, w)
    _, g_fresh = hip_grads(fresh, x, cn, w)
    for k in g_fresh:
        assert torch.equal(g_net[k], g_fresh[k]), k


IMAGES = ("fwd", "bwd", "fwd_wino", "bwd_wino", "fwd_wino4", "bwd_wino4", "fwd_wino45", "bwd_wino45", "fwd_wino85", "bwd_wino85",
          "w_raw")


@pytest.mark.parametrize("shape", [(256, 256, 5, 3), (128, 96, 5, 3), (96, 96, 5, 3), (64, 64, 5, 3), (64, 2, 5, 3), (2, 64, 1, 1),
                                   (96, 192, 1, 1), (128, 64, 1, 1)])
def test_repack_in_place_equals_fresh_pack_full_width_shapes(shape):
    """PackedConv.repack writes, into the SAME buffers, every image (forward and transposed, direct and Winograd) a freshly built
    PackedConv holds for the new weights: the full-width shapes, where the F(2,5)/F(4,5) images exist."""
    from babe_amd import ops
    gen = torch.Generator().manual_seed(sum(shape))
    w0 = torch.randn(shape, generator=gen).cuda()
    w1 = torch.randn(shape, generator=gen).cuda()
    pc = ops.PackedConv(w0.clone())
    ptrs = {n: getattr(pc, n).data_ptr() for n in IMAGES if getattr(pc, n) is not None}
    pc.repack(w1)
    fresh = ops.PackedConv(w1.clone())
    for n in IMAGES:
        a, b = getattr(pc, n), getattr(fresh, n)
        assert (a is None) == (b is None), n
        if a is not None:
            assert a.data_ptr() == ptrs[n], n
            assert torch.equal(a, b), n
    assert shape[:2] not in ((256, 256),) or pc.fwd_wino85 is not None


def test_sgd_step_lowers_loss_first_order():
    from babe_amd.config import default_args
    from babe_amd.diff_params.edm import EDM
    args = default_args(sample_rate=22050, audio_len=L_SMALL, Ns=[8, 8, 8, 8, 16, 16, 16])
    edm = EDM(args)
    net = make_net()
    net.set_trainable(True)
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


def test_param_grads_refused_for_attention_and_bf16():
    from babe_amd.networks.cqtdiff_plus import init_state_dict
    att = [0, 0, 0, 0, 0, 1, 1, 1]
    Ns = [8, 8, 8, 8, 16, 16, 16]
    net = make_net(init_state_dict(Ns, CFG["num_dils"], attention_layers=att, attention_dict=dict(num_heads=2)), Ns=Ns,
                   attention_layers=att, attention_dict=dict(num_heads=2))
    net.set_trainable(True)
    x, cn, _ = inputs(1, L_SMALL)
    with pytest.raises(NotImplementedError):
        net(x.cuda(), cn.cuda())
    nb = make_net(precision="bf16")
    nb.set_trainable(True)
    with pytest.raises(NotImplementedError):
        nb(x.cuda(), cn.cuda())
    nr = make_net()
    nr.embedding.RFF_freq.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        nr(x.cuda(), cn.cuda())
