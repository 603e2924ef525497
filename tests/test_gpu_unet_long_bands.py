"""A real design with 8192-point bands end to end: Unet_CQT_oct_with_attention at 48 kHz with the reference's 8 s context
(audio_len = 384000: T_oct = 128 .. 8192, the top octave's bands up to 4168 samples) - the CQT on band_fft13_kernel, and the
conv, GroupNorm, resample and element-wise kernels at T = 8192 - against the CPU oracle (oracle/unet.py + oracle/nsgt.py, float32
torch, autograd for the VJP), with the same check at the 22050 / 92092 design beside it as the control.  Then one babe_score_eval
call on that network against the Python sequencer, bit for bit (tests/test_gpu_eval_c.py does this at 92092).  Needs a MI355X.

Relative L2 against the oracle on a MI355X (bars: the project's attention-free bars, 2e-5 forward and 2e-4 VJP):
    48000 / 384000   forward 4.06e-7   VJP 4.08e-7
    22050 /  92092   forward 3.92e-7   VJP 3.93e-7"""
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_VJP = 2e-5, 2e-4
NS = [8, 8, 8, 8, 16, 16, 16]
LONG = (48000, 384000)
_NETS = {}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def net_of(fs, L):
    """One network per design for the module: (args, HIP network, its weights on the CPU)."""
    if (fs, L) not in _NETS:
        from babe_amd.config import default_args
        from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
        args = default_args(sample_rate=fs, audio_len=L, Ns=NS, T=3, start_sigma=0.05)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("BABE_CQT_C", "1")
            net = Unet_CQT_oct_with_attention(args, "cuda")
        sd = init_state_dict(NS, args.network.num_dils, seed=0, gate_scale=1.0)
        net.load_state_dict(sd)
        _NETS[(fs, L)] = (args, net, sd)
    return _NETS[(fs, L)]


def _against_oracle(fs, L):
    from oracle import unet as UN
    from oracle.nsgt import CQT_nsgt as OracleCQT
    args, net, sd = net_of(fs, L)
    cfg = dict(num_octs=7, bins_per_oct=64, num_dils=list(args.network.num_dils))
    gen = torch.Generator().manual_seed(21)
    x = 0.1 * torch.randn(1, L, generator=gen)
    wv = torch.randn(1, L, generator=gen)
    cn = torch.tensor([[-0.7]])
    y = net.fwd_nograd(x.cuda(), cn.cuda())
    gx = net.vjp(wv.cuda())
    torch.cuda.synchronize()
    eng = net.engine()
    assert eng._c_engine() is not None, "the library-side UNet sequencer did not run"
    assert bool(net.CQTransform._plan), "the library's CQT plan did not run"
    xo = x.clone().requires_grad_(True)
    yo = UN.unet_forward(sd, cfg, OracleCQT(7, 64, "oct", ("kaiser", 1), fs, L), xo, cn)
    go, = torch.autograd.grad((yo * wv).sum(), xo)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(gx).all())
    return rel(y, yo), rel(gx, go)


def test_unet_at_48k_8s_vs_oracle(monkeypatch):
    """Fails in the constructor without the 8192-point band transform (design_bands: "band longer than the LDS FFT supports").
    The UNet body runs on the library-side sequencer (BABE_UNET_C=1: babe_unet_fwd / babe_unet_vjp), the CQT on the library's plan."""
    from babe_amd.forms import FORMS
    monkeypatch.setattr(FORMS, "unet_c", True)
    _, net, _ = net_of(*LONG)
    assert net.CQTransform.T_oct == [128, 256, 512, 1024, 2048, 4096, 8192] and int(net.CQTransform.design["M"].max()) == 4168
    ef, ev = _against_oracle(*LONG)
    cf, cv = _against_oracle(22050, 92092)
    print(f"unet vs oracle: 48000/384000 forward {ef:.3e} vjp {ev:.3e}   control 22050/92092 forward {cf:.3e} vjp {cv:.3e}")
    assert cf < TOL_FWD and cv < TOL_VJP, ("control", cf, cv)
    assert ef < TOL_FWD and ev < TOL_VJP, (ef, ev)


def test_score_eval_on_the_long_design_equals_the_python_sequencer_bit_for_bit(monkeypatch):
    """One babe_score_eval call (UNet plan + CQT plan with long bands + STFT tables) against BlindSampler.evaluate sequencing the
    same kernels from Python."""
    import babe_amd.testing.blind_bwe_sampler as bs
    from babe_amd.diff_params.edm import EDM
    fs, L = LONG
    args, net, _ = net_of(fs, L)
    smp = bs.BlindSampler(net, EDM(args), args, batch_semantics="per_clip")
    g = torch.Generator().manual_seed(5)
    y = (0.1 * torch.randn(1, L, generator=g)).cuda()
    x = (y.cpu() + 0.05 * torch.randn(1, L, generator=g)).cuda()
    specY = smp.stft_ops(L, y.device).stft(y)
    ic = smp.args.tester.blind_bwe.initial_conditions
    fp = torch.tensor([list(ic.fc), list(ic.A)], dtype=torch.float32).unsqueeze(0).cuda()
    res = {}
    for mode in (False, True):
        monkeypatch.setattr(bs, "EVAL_C", mode)
        d, x_den, p = smp.evaluate(x, 0.05, y, specY, fp, True, lane=0)
        torch.cuda.synchronize()
        res[mode] = (d.clone(), x_den.clone(), p.clone())
    assert smp._ceval, "the library path did not run"
    assert bool(torch.isfinite(res[True][0]).all())
    for a, b, name in zip(res[False], res[True], ("score", "x_den", "filter parameters")):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
