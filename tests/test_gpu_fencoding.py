"""Frequency encodings (use_fencoding) folded into a conv bias: the conv epilogue's fbias, the bias-table and weight-gradient
kernels of csrc/fenc.hip against float64 torch, the network against the imported reference's outputs
(tests/golden/make_fencoding_golden.py), the library-side sequencers, parameter gradients and the weight refresh.  Needs a MI355X."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
TOL_OP = 3e-6                              # the project's op bar (tests/test_gpu_ops.py)
TOL_FWD, TOL_VJP = 2e-5, 2e-4              # tests/test_gpu_unet_attention.py
TOL_GRAD = 2e-4                            # tests/test_gpu_unet_train.py
RS2 = 1.0 / math.sqrt(2.0)
L = 92092


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def load(name):
    return {k: (torch.from_numpy(np.asarray(v)) if np.asarray(v).dtype.kind in "fiu" else np.asarray(v))
            for k, v in np.load(os.path.join(G, name)).items()}


def make_net(name="a", sd=None):
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    from tests.fencoding_weights import FIXTURES, FS, fencoding_sd
    from tests.attention_weights import SMALL_NS
    layers, adict, _ = FIXTURES[name]
    args = default_args(sample_rate=FS, audio_len=L, Ns=list(SMALL_NS))
    args.network.use_fencoding = True
    if layers:
        args.network.attention_layers = list(layers)
        args.network.attention_dict = dict(adict)
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(fencoding_sd(name) if sd is None else sd, strict=True)
    return net


def golden_inputs(g, B):
    gen = torch.Generator().manual_seed(int(g["seed"]))
    x = 0.1 * torch.randn(B, L, generator=gen)
    w = torch.randn(B, L, generator=gen)
    return x.cuda(), g["cnoise"].cuda(), w.cuda()


def fwd_vjp(net, x, cn, w):
    y = net.fwd_nograd(x, cn)
    gx = net.vjp(w)
    torch.cuda.synchronize()
    return y, gx


# ---------------------------------------------------------------------------------------------------- kernels
def _conv_case(Cout, T, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 2, 64, T, generator=g)
    w66 = torch.randn(Cout, 66, generator=g) / math.sqrt(66)
    emb = torch.randn(64, 64, generator=g)
    x66 = torch.cat([x.double(), emb.double()[None, :, :, None].expand(2, 64, 64, T)], 1)
    ref = torch.einsum("oc,bcft->boft", w66.double(), x66)
    return x, w66, emb, ref


# T = 5 / 130 take the direct (1,1) kernel (T % 4 != 0), T = 64 / 132 the pipelined conv11p_fb_kernel: 64 at its threshold
# F * T = 4096 with whole time tiles, 132 with a partial time tile in the buffer-descriptor epilogue.
@pytest.mark.parametrize("T", [5, 64, 130, 132])
@pytest.mark.parametrize("Cout", [8, 96, 256])
def test_conv_fbias_vs_float64_conv_on_66_channels(Cout, T):
    from babe_amd import ops
    x, w66, emb, ref = _conv_case(Cout, T, 100 * Cout + T)
    pc = ops.PackedConv(w66[:, :2].reshape(Cout, 2, 1, 1).contiguous().cuda())
    fb = ops.fenc_bias(w66.cuda(), emb.cuda(), torch.empty(Cout, 64, device="cuda"))
    out = ops.conv2d(x.cuda(), pc, torch.empty(2, Cout, 64, T, device="cuda"), fbias=fb)
    e = rel(out, ref)
    print(f"fbias conv Cout={Cout} T={T}: rel {e:.2e}")
    assert e < TOL_OP
    plain = ops.conv2d(x.cuda(), pc, torch.empty(2, Cout, 64, T, device="cuda"))
    assert rel(plain, ref) > 0.5                        # without the table the result is a different tensor


@pytest.mark.parametrize("Cout,T", [(8, 130), (96, 64), (256, 5), (8, 132), (256, 132)])
def test_conv_fbias_into_strided_view_with_residual(Cout, T):
    """The form of the init block's res_conv call: out a frequency sub-view of a taller buffer, res, alpha = rbeta = 1/sqrt2."""
    from babe_amd import ops
    x, w66, emb, ref = _conv_case(Cout, T, 7 * Cout + T)
    g = torch.Generator().manual_seed(Cout)
    res = torch.randn(2, Cout, 64, T, generator=g)
    pc = ops.PackedConv(w66[:, :2].reshape(Cout, 2, 1, 1).contiguous().cuda())
    fb = ops.fenc_bias(w66.cuda(), emb.cuda(), torch.empty(Cout, 64, device="cuda"))
    big = torch.full((2, Cout, 192, T), 7.0, device="cuda")
    ops.conv2d(x.cuda(), pc, big[:, :, :64, :], res=res.cuda(), alpha=RS2, rbeta=RS2, fbias=fb)
    e = rel(big[:, :, :64, :], RS2 * ref + RS2 * res.double())
    print(f"fbias conv (strided, res) Cout={Cout} T={T}: rel {e:.2e}")
    assert e < TOL_OP
    assert float((big[:, :, 64:, :] - 7.0).abs().max()) == 0.0


def test_fbias_on_a_5x3_conv_is_refused_not_ignored():
    from babe_amd import _lib, ops
    g = torch.Generator().manual_seed(1)
    pc = ops.PackedConv(torch.randn(64, 16, 5, 3, generator=g).cuda())
    x = torch.randn(1, 16, 64, 64, generator=g).cuda()
    fb = torch.zeros(64, 64, device="cuda")
    with pytest.raises(_lib.BabeHipError, match="fbias"):
        ops.conv2d(x, pc, torch.empty(1, 64, 64, 64, device="cuda"), fbias=fb)
    pb = ops.PackedConv(torch.randn(64, 64, 1, 1, generator=g).cuda(), "bf16")
    assert pb.splits
    with pytest.raises(_lib.BabeHipError, match="fbias"):
        ops.conv2d(torch.randn(1, 64, 64, 64, generator=g).cuda(), pb, torch.empty(1, 64, 64, 64, device="cuda"), fbias=fb)


def test_fenc_wgrad_rows_refuses_another_bin_count():
    from babe_amd import _lib, ops
    g = torch.zeros(1, 8, 32, 8, device="cuda")
    with pytest.raises(_lib.BabeHipError, match="F = 32"):
        ops.fenc_wgrad_rows(g, torch.zeros(64, 64, device="cuda"), torch.zeros(1, 8 * 66, device="cuda"))


@pytest.mark.parametrize("Cout,T", [(8, 5), (8, 130), (96, 5), (96, 130)])
def test_fenc_bias_and_wgrad_rows_vs_float64(Cout, T):
    from babe_amd import ops
    g = torch.Generator().manual_seed(Cout + T)
    w66 = torch.randn(Cout, 66, generator=g)
    emb = torch.randn(64, 64, generator=g)
    fb = ops.fenc_bias(w66.cuda(), emb.cuda(), torch.empty(Cout, 64, device="cuda"))
    fb2 = ops.fenc_bias(w66.cuda(), emb.cuda(), torch.empty(Cout, 64, device="cuda"))
    assert rel(fb, w66[:, 2:].double() @ emb.double()) < TOL_OP and torch.equal(fb, fb2)
    big = torch.randn(3, Cout, 128, T, generator=g).cuda()
    gv = big[:, :, 64:, :]                                  # a strided frequency sub-view
    want = 0.7 * torch.einsum("jf,bcf->bcj", emb.double(), gv.double().cpu().sum(-1))
    outs = []
    for _ in range(2):
        rows = torch.full((3, Cout * 66 + 5), 3.0, device="cuda")[:, :Cout * 66]      # row stride != row length
        ops.fenc_wgrad_rows(gv, emb.cuda(), rows, alpha=0.7)
        outs.append(rows.clone())
    got = outs[0].view(3, Cout, 66)
    e = rel(got[:, :, 2:], want)
    print(f"fenc_wgrad_rows Cout={Cout} T={T}: rel {e:.2e}")
    assert e < TOL_OP and torch.equal(outs[0], outs[1])
    assert float((got[:, :, :2] - 3.0).abs().max()) == 0.0   # the signal columns are not this kernel's


# ---------------------------------------------------------------------------------------------------- network
@pytest.fixture(scope="module")
def net_a():
    return make_net("a")


@pytest.fixture(scope="module")
def gold_a():
    g = load("fencoding_a.npz")
    g["gx"] = load("fencoding_a_vjp.npz")["gx"]
    return g


def test_network_vs_reference_golden_and_tables_are_visible(net_a, gold_a):
    x, cn, w = golden_inputs(gold_a, 2)
    y, gx = fwd_vjp(net_a, x, cn, w)
    ey, eg = rel(y, gold_a["y"]), rel(gx, gold_a["gx"])
    print(f"fencoding fixture a: fwd rel {ey:.2e}, vjp rel {eg:.2e}")
    assert ey < TOL_FWD and eg < TOL_VJP
    net0 = make_net("a")
    for blk in net0.engine().init_blk:
        blk.fb_proj_in.zero_()
        blk.fb_res_conv.zero_()
    y0, gx0 = fwd_vjp(net0, x, cn, w)
    print(f"Fb = 0: fwd rel {rel(y0, gold_a['y']):.2e}, vjp rel {rel(gx0, gold_a['gx']):.2e}")
    assert rel(y0, gold_a["y"]) > 100 * TOL_FWD and rel(gx0, gold_a["gx"]) > 100 * TOL_VJP


def test_network_with_attention_and_encodings_vs_reference_golden():
    g = load("fencoding_b.npz")
    net = make_net("b")
    x, cn, w = golden_inputs(g, 1)
    y, gx = fwd_vjp(net, x, cn, w)
    ey, eg = rel(y, g["y"]), rel(gx, g["gx"])
    print(f"fencoding fixture b (attention): fwd rel {ey:.2e}, vjp rel {eg:.2e}")
    assert ey < TOL_FWD and eg < TOL_VJP


@pytest.mark.parametrize("B", [1, 2])
def test_library_side_unet_equals_python_sequencer(monkeypatch, gold_a, B):
    from babe_amd.forms import FORMS
    x, cn, w = golden_inputs(gold_a, 2)
    x, cn, w = x[:B].contiguous(), cn[:B].contiguous(), w[:B].contiguous()
    monkeypatch.setattr(FORMS, "unet_c", False)
    y0, g0 = fwd_vjp(make_net("a"), x, cn, w)
    monkeypatch.setattr(FORMS, "unet_c", True)
    netc = make_net("a")
    y1, g1 = fwd_vjp(netc, x, cn, w)
    assert netc.engine()._c_engine().ws is not None, "the library path did not run"       # its state already holds a workspace
    assert torch.equal(y0, y1) and torch.equal(g0, g1)


@pytest.mark.parametrize("B", [1, 2])
def test_library_side_score_eval_equals_python_sequencer(monkeypatch, B):
    import babe_amd.testing.blind_bwe_sampler as bs
    from babe_amd.config import default_args
    from babe_amd.diff_params.edm import EDM
    from tests.attention_weights import SMALL_NS
    from tests.fencoding_weights import FS
    monkeypatch.setenv("BABE_CQT_C", "1")
    net = make_net("a")
    args = default_args(sample_rate=FS, audio_len=L, Ns=list(SMALL_NS), T=3, start_sigma=0.05)
    smp = bs.BlindSampler(net, EDM(args), args, batch_semantics="per_clip")
    g = torch.Generator().manual_seed(5)
    y = (0.1 * torch.randn(B, L, generator=g)).cuda()
    x = (y.cpu() + 0.05 * torch.randn(B, L, generator=g)).cuda()
    specY = smp.stft_ops(L, y.device).stft(y)
    ic = smp.args.tester.blind_bwe.initial_conditions
    fp = torch.tensor([list(ic.fc), list(ic.A)], dtype=torch.float32).unsqueeze(0).repeat(B, 1, 1).cuda()
    outs = {}
    for mode in (False, True):
        monkeypatch.setattr(bs, "EVAL_C", mode)
        d, x_den, p = smp.evaluate(x, 0.05, y, specY, fp, True, lane=0)
        torch.cuda.synchronize()
        outs[mode] = (d.clone(), x_den.clone(), p.clone())
    assert smp._ceval, "the library path did not run"
    assert all(torch.equal(u, v) for u, v in zip(outs[False], outs[True]))


def hip_grads(net, x, cn, w):
    net.set_trainable(True)
    for p in net.parameters():
        p.grad = None
    y = net(x, cn)
    (y * w).sum().backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.requires_grad}


def test_param_grads_vs_reference_golden(net_a, gold_a):
    f = gold_a
    x, cn, w = golden_inputs(f, 2)
    got = hip_grads(net_a, x, cn, w)
    net_a.set_trainable(False)
    keys = f["trainable"].tolist()
    assert set(got) == set(keys)
    assert tuple(got["downs.0.0.proj_in.weight"].shape) == (8, 66, 1, 1)
    gd = torch.Generator().manual_seed(int(f["dir_seed"]))
    worst = ("", 0.0)
    for k, n_ref, p_ref in zip(keys, f["grad_norm"], f["grad_proj"]):
        g = got[k].double().cpu().reshape(-1)
        d = torch.randn(4, g.numel(), generator=gd).double()
        en = abs(float(g.norm()) - float(n_ref)) / float(n_ref)
        ep = float(((d @ g) - p_ref.double()).abs().max()) / (float(n_ref) * float(d.norm(dim=1).max()))
        if max(en, ep) > worst[1]:
            worst = (k, max(en, ep))
        assert en < TOL_GRAD and ep < TOL_GRAD, (k, en, ep)
    print(f"worst relative error vs the reference fixture: {worst[1]:.2e} ({worst[0]})")


_ONE_LANE = """
import sys, torch
sys.path.insert(0, {root!r})
from tests.test_gpu_fencoding import make_net, load, golden_inputs, hip_grads
net = make_net("a")
assert net.MAX_LANES == 1
x, cn, w = golden_inputs(load("fencoding_a.npz"), 2)
torch.save({{k: v.cpu() for k, v in hip_grads(net, x, cn, w).items()}}, {out!r})
"""


def test_two_lanes_equal_one_lane_row_for_row(net_a, gold_a, tmp_path):
    """BABE_UNET_STREAMS=1 is read at import, so the one-lane run is a fresh child process."""
    out = str(tmp_path / "one_lane.pt")
    env = dict(os.environ, BABE_UNET_STREAMS="1")
    subprocess.run([sys.executable, "-c", _ONE_LANE.format(root=ROOT, out=out)], check=True, env=env, cwd=ROOT, timeout=300)
    one = torch.load(out)
    assert net_a.MAX_LANES == 2
    x, cn, w = golden_inputs(gold_a, 2)
    two = hip_grads(net_a, x, cn, w)
    net_a.set_trainable(False)
    assert set(one) == set(two)
    for k in one:
        assert torch.equal(one[k], two[k].cpu()), k


def test_in_place_weight_change_rebuilds_the_bias_table(gold_a):
    x, cn, w = golden_inputs(gold_a, 2)
    net = make_net("a")
    y_before, _ = fwd_vjp(net, x, cn, w)
    fb_ptr = net.engine().init_blk[3].fb_proj_in.data_ptr()
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():
        wp = net.get_parameter("downs.3.0.proj_in.weight")
        wp.add_(0.05 * torch.randn(wp.shape, generator=gen).cuda())
    y, gx = fwd_vjp(net, x, cn, w)
    assert net.engine().init_blk[3].fb_proj_in.data_ptr() == fb_ptr          # rewritten in place
    fresh = make_net("a", sd={k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    yf, gf = fwd_vjp(fresh, x, cn, w)
    assert not torch.equal(y, y_before)
    assert torch.equal(y, yf) and torch.equal(gx, gf)
