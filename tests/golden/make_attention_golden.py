"""Generate the time-attention golden vectors (tests/golden/attention_*.npz) by IMPORTING the reference.

Run in the build container only (needs the reference sources, see oracle/ref_shim.py):
    python tests/golden/make_attention_golden.py [a b c d]
Weights: babe_amd's init_state_dict(seed) with the attention keys (tests/attention_weights.py), loaded into the reference
network; only outputs are stored (the qk weights alone are 25.7 M parameters per attention block at the deepest level).
  a: reduced width, 22.05 kHz, L = 92092, attention_layers [0,0,0,0,1,1,1,1], relative position bias on - UNet output and
     input-VJP, plus the reference's state-dict key list with shapes;
  b: the same net with attention on all 8 levels, use_rel_pos=False, bias_qkv=True;
  c: full width, 44.1 kHz, L = 46046, [0,0,0,0,1,1,1,1];
  d: the reference's predict_blind_bwe at T = 3 with net (a) (recorded noises, as make_golden.g7_8).
"""
import contextlib
import importlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from oracle.nsgt import CQT_nsgt  # noqa: E402

ref_shim.install(CQT_nsgt)
torch.set_num_threads(8)

from tests.attention_weights import FIXTURES, fixture_sd  # noqa: E402

edm_mod = importlib.import_module("diff_params.edm")
bu = importlib.import_module("utils.blind_bwe_utils")
net_mod = importlib.import_module("networks.cqtdiff+")
samp_mod = importlib.import_module("testing.blind_bwe_sampler")


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def save(name, **kw):
    np.savez_compressed(os.path.join(HERE, name), **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in kw.items()})
    print("wrote", name, os.path.getsize(os.path.join(HERE, name)) // 1024, "KiB")


def ref_net(name, T=3):
    Ns, fs, L, layers, adict = FIXTURES[name]
    args = ref_shim.load_args(exp="maestro22k_8s" if fs == 22050 else "maestro44k_8s")
    args.exp.audio_len = L
    args.exp.sample_rate = fs
    args.network.Ns = list(Ns)
    args.network.attention_layers = list(layers)
    args.network.attention_dict = ref_shim.to_attr(dict(adict))
    args.tester.T = T
    with quiet():
        net = net_mod.Unet_CQT_oct_with_attention(args, "cpu")
    net.load_state_dict(fixture_sd(name), strict=True)
    return net, args


def unet_fixture(name, seed):
    net, args = ref_net(name)
    L = args.exp.audio_len
    g = torch.Generator().manual_seed(seed)
    x = (0.1 * torch.randn(1, L, generator=g)).requires_grad_(True)
    cn = torch.tensor([[-0.4]])
    y = net(x, cn)
    wv = torch.randn(y.shape, generator=g)
    gx, = torch.autograd.grad((y * wv).sum(), x)
    keys = np.array([f"{k}:{'x'.join(str(s) for s in v.shape)}" for k, v in net.state_dict().items()])
    save(f"attention_{name}.npz", seed=seed, cnoise=cn, y=y.detach(), gx=gx, keys=keys)


def a():
    unet_fixture("a", 5100)


def b():
    unet_fixture("b", 5200)


def c():
    unet_fixture("c", 5300)


class ResidualNetRef:
    """net'(x, c) = a*net(x, c) + (sigma/sigma_data)*x (make_golden.g7_8): keeps the per-step filter fit well posed."""

    def __init__(self, inner, a, sigma_data):
        self.inner, self.a, self.sd = inner, a, sigma_data
        self.CQTransform = inner.CQTransform

    def __call__(self, x, cnoise):
        return self.a * self.inner(x, cnoise) + (torch.exp(4 * cnoise) / self.sd) * x


def d():
    net, args = ref_net("a", T=3)
    L = args.exp.audio_len
    args.tester.posterior_sampling.start_sigma = 0.05
    with quiet():
        s = samp_mod.BlindSampler(ResidualNetRef(net, 0.3, args.tester.diff_params.sigma_data), edm_mod.EDM(args), args)
    g = torch.Generator().manual_seed(5400)
    t_ax = torch.arange(L) / args.exp.sample_rate
    clean = sum(0.05 / (k + 1) * torch.sin(2 * np.pi * 220.0 * (k + 1) * t_ax) * torch.exp(-t_ax * (1 + k)) for k in range(12))
    clean = clean[None] + 0.1 * torch.randn(1, L, generator=g)
    f = torch.fft.rfftfreq(4096, d=1 / args.exp.sample_rate)
    y = bu.apply_filter(clean, bu.design_filter(torch.tensor([2000.0]), torch.tensor([-40.0]), f), 4096)
    noises = [torch.randn(1, L, generator=g) for _ in range(1 + args.tester.T)]
    it = iter(noises)
    orig_randn = torch.randn
    torch.randn = lambda *a_, **k: next(it)
    try:
        with quiet(), contextlib.redirect_stderr(io.StringIO()):
            xres, fp, data_den, t, data_filt = s.predict_blind_bwe(y.clone(), rid=True)
    finally:
        torch.randn = orig_randn
    # per-step denoised estimates every 16th sample (as make_golden's sampler_obs_noise): keeps the fixture small
    save("attention_d_sampler.npz", seed=5400, res_a=0.3, start_sigma=0.05, y=y, x=xres, filter_params=fp, t=t,
         data_filters=data_filt, data_denoised_sub16=data_den[:, :, ::16])


if __name__ == "__main__":
    for w in sys.argv[1:] or ["a", "b", "c", "d"]:
        globals()[w]()
