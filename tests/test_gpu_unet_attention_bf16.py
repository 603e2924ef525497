"""CQTDiff+ UNet with time-attention layers in a bf16 / bf16x3 network, and the attention core on bf16 MFMA
(attention_precision, csrc/attention_bf16.hip): forward and input-VJP against the fp32 network on the same weights and inputs
(which tests/test_gpu_unet_attention.py pins to the reference), the option's contract, and the blind sampler.  Needs a MI355X."""
import functools

import pytest
import torch

from tests.test_gpu_unet_attention import ResidualNet, load, rel, rms_err
from tests.test_gpu_unet_full import RP_TOL

pytestmark = pytest.mark.gpu
CORE_FWD, CORE_VJP = 5e-3, 7e-3            # the kernel bars of tests/attention_bf16_cases.py (out; dqk)


def make_net(name, precision="f32", attention_precision=None, T=3, start_sigma=0.05, via_args=False):
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    from tests.attention_weights import FIXTURES, fixture_sd
    Ns, fs, L, layers, adict = FIXTURES[name]
    args = default_args(sample_rate=fs, audio_len=L, Ns=Ns, T=T, start_sigma=start_sigma)
    args.network.attention_layers = list(layers)
    args.network.attention_dict = dict(adict)
    if via_args:
        args.network.attention_precision = attention_precision
        net = Unet_CQT_oct_with_attention(args, "cuda", precision=precision)
    else:
        net = Unet_CQT_oct_with_attention(args, "cuda", precision=precision, attention_precision=attention_precision)
    net.load_state_dict(fixture_sd(name), strict=True)
    return net, args


def inputs(name):
    """x, cnoise and the VJP's cotangent of tests/test_gpu_unet_attention.py::fwd_vjp for this fixture."""
    from tests.attention_weights import FIXTURES
    g = load(f"attention_{name}.npz")
    L = FIXTURES[name][2]
    gen = torch.Generator().manual_seed(int(g["seed"]))
    x = (0.1 * torch.randn(1, L, generator=gen)).cuda()
    wv = torch.randn(1, L, generator=gen).cuda()
    return x, g["cnoise"].cuda(), wv


def fwd_vjp(net, name):
    x, cn, wv = inputs(name)
    y = net.fwd_nograd(x, cn)
    gx = net.vjp(wv)
    torch.cuda.synchronize()
    return y.cpu(), gx.cpu()


@functools.lru_cache(maxsize=None)
def fp32_result(name):
    """The fp32 network's (y, gx), computed once per fixture and left unchanged."""
    return fwd_vjp(make_net(name)[0], name)


def errors(name, precision, attention_precision):
    y32, g32 = fp32_result(name)
    y, gx = fwd_vjp(make_net(name, precision, attention_precision)[0], name)
    assert torch.isfinite(y).all() and torch.isfinite(gx).all()
    ey, eg = rel(y, y32), rel(gx, g32)
    print(f"fixture {name} precision={precision} attention_precision={attention_precision}: fwd rel {ey:.2e}, vjp rel {eg:.2e}")
    return ey, eg


@pytest.mark.parametrize("name", ["a", "b"])
def test_bf16_network_with_attention_vs_fp32_network(name):
    """precision='bf16' with the fp32 and with the bf16 attention core: both within the project's bf16 network bars
    (RP_TOL['bf16'] of tests/test_gpu_unet_full.py), and the bf16 core costs at most its own kernel bars on top."""
    ty, tg = RP_TOL["bf16"]
    ey_f, eg_f = errors(name, "bf16", "f32")
    ey_b, eg_b = errors(name, "bf16", "bf16")
    assert ey_f < ty and eg_f < tg
    assert ey_b < ty and eg_b < tg
    assert ey_b <= ey_f + CORE_FWD and eg_b <= eg_f + CORE_VJP


def test_bf16_full_width_network_with_bf16_attention_vs_fp32_network():
    """Fixture "c": full widths at L = 46046 (attention at F = 320, 384, 448), bf16 network, bf16 core."""
    ey, eg = errors("c", "bf16", "bf16")
    assert ey < RP_TOL["bf16"][0] and eg < RP_TOL["bf16"][1]


def test_bf16x3_network_keeps_the_fp32_core():
    ey, eg = errors("a", "bf16x3", "f32")
    assert ey < RP_TOL["bf16x3"][0] and eg < RP_TOL["bf16x3"][1]


def test_fp32_network_with_bf16_core_and_the_options_contract(monkeypatch):
    """precision='f32' with attention_precision='bf16' (the A/B of the core alone): forward within 5e-3 and VJP within 7e-3 of
    the fp32 network; autograd through net(x, cnoise) runs the same VJP; the lane rule, training and the library-side
    sequencers treat the network as the issue states."""
    from babe_amd.networks.unet_c import CUnet
    from babe_amd.testing import eval_c
    y32, g32 = fp32_result("a")
    net, _ = make_net("a", "f32", "bf16", via_args=True)            # the option given as args.network.attention_precision
    assert net.attention_precision == "bf16" and net.engine().attn_core == "bf16"
    y, gx = fwd_vjp(net, "a")
    ey, eg = rel(y, y32), rel(gx, g32)
    print(f"fixture a precision=f32 attention_precision=bf16: fwd rel {ey:.2e}, vjp rel {eg:.2e}")
    assert ey < CORE_FWD and eg < CORE_VJP
    assert ey > 1e-5                                                # the bf16 core really ran (fp32 repeats itself bit for bit)
    # autograd through the module = net.vjp
    x, cn, wv = inputs("a")
    xr = x.clone().requires_grad_(True)
    ga, = torch.autograd.grad((net(xr, cn) * wv).sum(), xr)
    assert torch.equal(ga.cpu(), gx)
    # lanes: like precision='bf16'
    monkeypatch.delenv("BABE_BF16_LANES", raising=False)
    assert not net.concurrent_lanes_ok and not net.lanes_ok_for("cpu")
    monkeypatch.setenv("BABE_BF16_LANES", "1")
    assert net.concurrent_lanes_ok and net.lanes_ok_for("cpu") and not net.lanes_ok_for("cuda")
    monkeypatch.delenv("BABE_BF16_LANES")
    # training stays fp32-only
    with pytest.raises(NotImplementedError, match="attention_precision"):
        net.set_trainable(True, attention=True)
    # the library-side sequencers still refuse the network
    assert net.has_attention and net.engine()._c_engine() is None
    with pytest.raises(NotImplementedError):
        CUnet(net.engine())

    class Smp:
        model = net
        norm, stft_dist, obs_snr, sigma_den, degradation, dc, _dc_cfg, data_consistency = 2, None, None, 0, None, None, False, False
    assert not eval_c.supported(Smp(), torch.zeros(1), True)


def test_attention_precision_values_and_defaults():
    for prec in ("bf16", "bf16x3"):
        with pytest.raises(NotImplementedError):                   # None: today's refusal
            make_net("a", prec)
    for bad in ("fp16", "bf16x3", 1):
        with pytest.raises(ValueError):
            make_net("a", "f32", bad)
        with pytest.raises(ValueError):
            make_net("a", "bf16", bad)
    # 'f32' inside a bf16 network: the existing fp32-only refusal of parameter gradients applies unchanged
    net, _ = make_net("a", "bf16", "f32")
    assert net.engine().attn_core == "f32" and not net.concurrent_lanes_ok
    net.set_trainable(True, attention=True)
    x, cn, _ = inputs("a")
    with pytest.raises(NotImplementedError, match="fp32 only"):
        net(x, cn)
    # on an attention-free network the option does nothing
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    from tests.attention_weights import SMALL_NS
    args = default_args(sample_rate=22050, audio_len=92092, Ns=SMALL_NS)
    plain = Unet_CQT_oct_with_attention(args, "cuda", attention_precision="bf16")
    assert not plain.has_attention and plain.concurrent_lanes_ok and plain.engine().attn_core is None
    plain.set_trainable(True, attention=True)                      # no attention layers: the flag does nothing


class _Residual(ResidualNet):
    """ResidualNet with the inner network's lane rule (the wrapper of the fp32 golden always allows two lanes)."""

    @property
    def concurrent_lanes_ok(self):
        return self.inner.concurrent_lanes_ok

    def lanes_ok_for(self, noise_device="cpu"):
        return self.inner.lanes_ok_for(noise_device)


def test_blind_sampler_bf16_network_bf16_attention_vs_fp32_run():
    """predict_blind_bwe at the T, seed and noise of test_blind_sampler_with_attention_vs_reference_golden: the bf16 network with
    the bf16 core against the fp32 network.  The project's bf16 sampler bar: RMS error below 5 % of the signal RMS."""
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    s = load("attention_d_sampler.npz")
    L = 92092
    res = {}
    for key, (prec, core) in {"f32": ("f32", None), "bf16": ("bf16", "bf16")}.items():
        net, args = make_net("a", prec, core, T=3, start_sigma=float(s["start_sigma"]))
        gen = torch.Generator().manual_seed(int(s["seed"]))
        _ = torch.randn(1, L, generator=gen)
        it = iter([torch.randn(1, L, generator=gen) for _ in range(4)])
        smp = BlindSampler(_Residual(net, float(s["res_a"]), 0.063), EDM(args), args)
        smp._randn = lambda shape, device: next(it).to(device)
        res[key] = smp.predict_blind_bwe(s["y"].cuda(), rid=True)[0].detach().cpu()
    x32, xb = res["f32"], res["bf16"]
    assert torch.isfinite(xb).all()
    sig = float(x32.double().pow(2).mean().sqrt())
    err = rms_err(xb, x32)
    print(f"sampler, bf16 network + bf16 attention vs fp32: RMS err {err:.2e}, signal RMS {sig:.2e}, ratio {err / sig:.2e}")
    assert err < 0.05 * sig
