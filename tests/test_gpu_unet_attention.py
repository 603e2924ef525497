"""CQTDiff+ UNet with time-attention layers: HIP forward and input-VJP against the imported reference's outputs
(tests/golden/make_attention_golden.py), lanes, the blind sampler, and the paths that refuse attention.  Needs a MI355X."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
TOL_FWD, TOL_VJP = 2e-5, 2e-4              # the bars of the attention-off UNet goldens (tests/test_gpu_sampler.py)


def load(name):
    return {k: (torch.from_numpy(np.asarray(v)) if np.asarray(v).dtype.kind in "fiu" else np.asarray(v))
            for k, v in np.load(os.path.join(G, name)).items()}


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rms_err(a, b):
    return float((a.detach().double().cpu() - b.double().cpu()).pow(2).mean().sqrt())


def make_net(name, T=3, start_sigma=0.05, precision="f32", sd=None):
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    from tests.attention_weights import FIXTURES, fixture_sd
    Ns, fs, L, layers, adict = FIXTURES[name]
    args = default_args(sample_rate=fs, audio_len=L, Ns=Ns, T=T, start_sigma=start_sigma)
    args.network.attention_layers = list(layers)
    args.network.attention_dict = dict(adict)
    net = Unet_CQT_oct_with_attention(args, "cuda", precision=precision)
    net.load_state_dict(fixture_sd(name) if sd is None else sd, strict=True)
    return net, args


def fwd_vjp(net, g, L, B=1):
    gen = torch.Generator().manual_seed(int(g["seed"]))
    x = (0.1 * torch.randn(1, L, generator=gen)).cuda()
    cn = g["cnoise"].cuda()
    y = net.fwd_nograd(x.expand(B, L).contiguous(), cn.expand(B, 1).contiguous())
    wv = torch.randn(1, L, generator=gen).cuda()
    gx = net.vjp(wv.expand(B, L).contiguous())
    torch.cuda.synchronize()
    return y, gx


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_unet_attention_vs_reference_golden(name):
    from tests.attention_weights import FIXTURES
    g = load(f"attention_{name}.npz")
    L = FIXTURES[name][2]
    net, _ = make_net(name)
    y, gx = fwd_vjp(net, g, L)
    ey, eg = rel(y, g["y"]), rel(gx, g["gx"])
    print(f"attention fixture {name}: fwd rel {ey:.2e}, vjp rel {eg:.2e}")
    assert ey < TOL_FWD and eg < TOL_VJP


def test_unet_attention_autograd_and_branch_is_visible():
    """Autograd through the HIP VJP matches the golden; with gate2 zeroed the attention branch vanishes and the output moves
    far outside the bar - the fixtures exercise the attention path."""
    from tests.attention_weights import fixture_sd
    g = load("attention_a.npz")
    net, _ = make_net("a")
    gen = torch.Generator().manual_seed(int(g["seed"]))
    x = (0.1 * torch.randn(1, 92092, generator=gen)).cuda().requires_grad_(True)
    y = net(x, g["cnoise"].cuda())
    wv = torch.randn(y.shape, generator=gen)
    gx, = torch.autograd.grad((y * wv.cuda()).sum(), x)
    assert rel(y, g["y"]) < TOL_FWD and rel(gx, g["gx"]) < TOL_VJP
    sd = fixture_sd("a")
    for k in sd:
        if ".gate2." in k:
            sd[k] = torch.zeros_like(sd[k])
    net0, _ = make_net("a", sd=sd)
    y0, gx0 = fwd_vjp(net0, g, 92092)
    print(f"gate2 = 0: fwd rel {rel(y0, g['y']):.2e}, vjp rel {rel(gx0, g['gx']):.2e}")
    assert rel(y0, g["y"]) > 100 * TOL_FWD and rel(gx0, g["gx"]) > 100 * TOL_VJP


def test_unet_attention_two_lanes_equal_one_bit_exact(monkeypatch):
    g = load("attention_a.npz")
    net, _ = make_net("a")
    y2, g2 = fwd_vjp(net, g, 92092, B=2)                    # two stream lanes (MAX_LANES = 2)
    monkeypatch.setattr(type(net), "MAX_LANES", 1)
    net._lanes = None
    y1, g1 = fwd_vjp(net, g, 92092, B=2)                    # one stream
    assert torch.equal(y1, y2) and torch.equal(g1, g2)
    assert torch.equal(y2[0], y2[1]) and torch.equal(g2[0], g2[1])
    assert rel(y1[:1], g["y"]) < TOL_FWD and rel(g1[:1], g["gx"]) < TOL_VJP


class ResidualNet:
    """a*net(x,c) + (sigma/sigma_data)*x, sigma = exp(4c) (the wrapper of make_attention_golden.d)."""

    def __init__(self, inner, a, sigma_data):
        self.inner, self.a, self.sd = inner, a, sigma_data
        self.CQTransform = inner.CQTransform

    supports_lanes = True
    concurrent_lanes_ok = True

    def lanes_ok_for(self, noise_device="cpu"):
        return True

    def fwd_nograd(self, x, cn, lane=None):
        self.k = float(torch.exp(4 * cn[0, 0])) / self.sd
        kw = {} if lane is None else {"lane": lane}
        return self.a * self.inner.fwd_nograd(x, cn, **kw) + self.k * x

    def vjp(self, g, lane=None):
        kw = {} if lane is None else {"lane": lane}
        return self.a * self.inner.vjp(g, **kw) + self.k * g


def test_blind_sampler_with_attention_vs_reference_golden():
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    s = load("attention_d_sampler.npz")
    net, args = make_net("a", T=3, start_sigma=float(s["start_sigma"]))
    L = 92092
    gen = torch.Generator().manual_seed(int(s["seed"]))
    _ = torch.randn(1, L, generator=gen)
    noises = [torch.randn(1, L, generator=gen) for _ in range(4)]
    smp = BlindSampler(ResidualNet(net, float(s["res_a"]), 0.063), EDM(args), args)
    it = iter(noises)
    smp._randn = lambda shape, device: next(it).to(device)
    x, fp, dden, t, dfil = smp.predict_blind_bwe(s["y"].cuda(), rid=True)
    assert torch.equal(t, s["t"])
    for i in range(3):
        assert rel(dden[i][:, ::16], s["data_denoised_sub16"][i]) < 1e-3, i
    print(f"sampler with attention: RMS err {rms_err(x, s['x']):.2e}, rel {rel(x, s['x']):.2e}, fp {fp.tolist()} vs {s['filter_params'].tolist()}")
    assert rms_err(x, s["x"]) < 1e-3 and rel(x, s["x"]) < 2e-3
    assert torch.allclose(fp[0].cpu(), s["filter_params"][0], rtol=1e-2) and torch.allclose(fp[1].cpu(), s["filter_params"][1], atol=1.0)


def test_attention_refused_by_bf16_and_library_sequencers():
    from babe_amd.networks.unet_c import CUnet
    from babe_amd.testing import eval_c
    for prec in ("bf16", "bf16x3"):
        with pytest.raises(NotImplementedError):
            make_net("a", precision=prec)
    net, args = make_net("a")
    assert net.has_attention
    eng = net.engine()
    assert eng._c_engine() is None
    with pytest.raises(NotImplementedError):
        CUnet(eng)

    class Smp:                                   # every other condition of the default evaluation holds
        model = net
        norm, stft_dist, obs_snr, sigma_den, degradation, dc, _dc_cfg, data_consistency = 2, None, None, 0, None, None, False, False
    assert not eval_c.supported(Smp(), torch.zeros(1), True)
