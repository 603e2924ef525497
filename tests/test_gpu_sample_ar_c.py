"""The AR observation model of predict_bwe_AR in the library: babe_score_eval with desc.mask / desc.dc_mask (csrc/score_eval.hip
through testing/eval_c.py) and a whole predict_bwe_AR(..., 'fc_A') run as ONE babe_sample_bwe call (BlindSampler(loop="library"))
against the Python sequencer issuing the same kernels, bit for bit.  Fixture of tests/test_gpu_sample_c.py: the smallest with a
churned Heun step, a plain Heun step and a final Euler step.  Needs a MI355X."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

NS, L, FS, T = [8, 8, 8, 8, 16, 16, 16], 92092, 22050, 3
OVERLAP = 5512                                            # int(0.25 * FS): the known head of an AR segment


def _args(inpaint_dc=True):
    from babe_amd.config import default_args
    args = default_args(sample_rate=FS, audio_len=L, Ns=NS, T=T, start_sigma=0.05)
    args.tester.complete_recording.inpaint_DC = inpaint_dc
    return args


@pytest.fixture(scope="module")
def world():
    """One network, one observed segment, the tail of a previous result and T + 1 noise tensors (never modified)."""
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    mp = pytest.MonkeyPatch()
    mp.setenv("BABE_CQT_C", "1")                       # the Python sequencer on the library's CQT plan (same tables)
    args = _args()
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(init_state_dict(NS, args.network.num_dils, seed=0, gate_scale=1.0))
    g = torch.Generator().manual_seed(11)
    ylpf = (0.1 * torch.randn(1, L, generator=g)).cuda()
    y_masked = torch.zeros(1, L)
    y_masked[:, :OVERLAP] = 0.1 * torch.randn(1, OVERLAP, generator=g)
    mask = torch.zeros(1, L)
    mask[:, :OVERLAP] = 1
    noises = [torch.randn(1, L, generator=g) for _ in range(T + 1)]
    yield dict(net=net, ylpf=ylpf, y_masked=y_masked.cuda(), mask=mask.cuda(), noises=noises)
    mp.undo()


def _sampler(world, inpaint_dc=True, **kw):
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    args = _args(inpaint_dc)
    return BlindSampler(world["net"], EDM(args), args, **kw)


def _known_filter():
    return torch.tensor([[3000.0, 5000.0], [-20.0, -40.0]])


def _last_segment(world, n=60000):
    """The inputs of restore_file_AR's last, short segment: the signal zero-padded, mask and y_masked cleared past n."""
    ylpf, y_masked, mask = world["ylpf"].clone(), world["y_masked"].clone(), world["mask"].clone()
    ylpf[:, n:] = 0
    y_masked[:, n:] = 0
    mask[:, n:] = 0
    return ylpf, y_masked, mask


@pytest.mark.parametrize("case", ["dc", "nodc", "last"])
def test_one_masked_evaluation_equals_the_python_sequencer_bit_for_bit(monkeypatch, world, case):
    """CEval with a mask (and the inpaint_DC pair) = BlindSampler.evaluate sequencing the kernels itself (BABE_EVAL_C=0), in d
    and x_den."""
    import babe_amd.testing.blind_bwe_sampler as bs
    from babe_amd.degrade import MaskMixDegradation, make_degradation
    from babe_amd.stft import lincomb, mask_blend
    from babe_amd.testing import eval_c
    ylpf, y_masked, mask = _last_segment(world) if case == "last" else (world["ylpf"], world["y_masked"], world["mask"])
    smp = _sampler(world, inpaint_dc=case != "nodc")
    smp.stft_ops(L, ylpf.device)
    _, params = make_degradation(_known_filter(), "fc_A", ylpf.device)
    y = mask_blend(mask, y_masked, ylpf)
    dc = None
    if case != "nodc":
        sm = smp.prepare_smooth_mask(mask, 50)
        dc = (sm, mask_blend(sm, y_masked, None))
    t = 0.05
    x = lincomb(torch.empty_like(y), 1.0, y, t, world["noises"][0].cuda())
    res = []
    for mode in (True, False):
        monkeypatch.setattr(bs, "EVAL_C", mode)
        with smp._guiding(MaskMixDegradation(mask, None), dc):
            assert eval_c.supported(smp, y, False) and not eval_c.supported(smp, y, True)
            d, x_den, _ = smp.evaluate(x, t, y, None, params, False)
        torch.cuda.synchronize()
        res.append((d.clone(), x_den.clone()))
    assert len(smp._ceval) == 1, "the library evaluation did not run"
    (d0, xd0), (d1, xd1) = res
    assert torch.isfinite(d0).all() and torch.isfinite(xd0).all()
    assert torch.equal(xd0, xd1), float((xd0 - xd1).abs().max())
    assert torch.equal(d0, d1), float((d0 - d1).abs().max())
    if case != "nodc":
        # the replacement step did something: on the known head the Tweedie estimate x - t d is the known signal
        x0 = x - t * d0
        assert float((x0[:, :OVERLAP - 50] - y_masked[:, :OVERLAP - 50]).abs().max()) < 1e-4


def _feed(smp, noises):
    it = iter(noises)
    smp._randn = lambda shape, device: next(it)[:shape[0]].contiguous().to(device)


def _run_ar(smp, world, filt_type="fc_A", **kw):
    filt = _known_filter() if filt_type == "fc_A" else torch.hann_window(33, periodic=False) / 16.0
    out = smp.predict_bwe_AR(world["ylpf"], world["y_masked"], filt, filt_type, mask=world["mask"], **kw)
    torch.cuda.synchronize()
    assert out.shape == (1, L) and torch.isfinite(out).all()
    return out.clone()


@pytest.mark.parametrize("noise", ["fed", "philox"])
def test_predict_bwe_AR_on_the_library_equals_the_python_loop_bit_for_bit(world, noise):
    """predict_bwe_AR(..., 'fc_A') with loop="library" is ONE babe_sample_bwe call and equals loop="python": fed the same T + 1
    noise tensors, and seeded on the library's generator (noise_device="philox") under a clip number."""
    kw = dict(seed=9, noise_device="philox") if noise == "philox" else {}
    call = dict(clip0=4) if noise == "philox" else {}
    lib_smp = _sampler(world, loop="library", **kw)
    py = _sampler(world, loop="python", **kw)
    if noise == "fed":
        _feed(lib_smp, world["noises"])
        _feed(py, world["noises"])
    got = _run_ar(lib_smp, world, **call)
    assert lib_smp._csample is not None and lib_smp._csample.calls == 1, "the library run did not run"
    want = _run_ar(py, world, **call)
    assert py._csample is None
    assert torch.equal(got, want), float((got - want).abs().max())
    if noise == "philox":
        other = _run_ar(_sampler(world, loop="library", **kw), world, clip0=5)
        assert not torch.equal(other, got)


def test_firwin_AR_stays_on_the_python_loop(world):
    smp = _sampler(world, loop="library", seed=1, noise_device="philox")
    _run_ar(smp, world, "firwin")
    assert smp._csample is None


def test_masked_workspace_is_exact_and_the_unmasked_size_unchanged(world):
    """babe_eval_workspace_bytes of the masked descriptor is what babe_score_eval takes: one byte less is refused before a
    launch; the unmasked descriptor's size is what it is with mask = NULL."""
    from babe_amd._lib import lib, ptr, stream
    from babe_amd.degrade import make_degradation
    from babe_amd.stft import mask_blend
    from babe_amd.testing import eval_c
    smp = _sampler(world)
    y, mask, y_masked = world["ylpf"], world["mask"], world["y_masked"]
    smp.stft_ops(L, y.device)
    ce = eval_c.CEval(smp, None)
    d = ce.desc
    _, params = make_degradation(_known_filter(), "fc_A", y.device)
    d.K, d.blind = 2, 0
    d.mask = None
    plain = lib().babe_eval_workspace_bytes(ctypes.byref(d), 1)
    assert plain > 0
    sm = smp.prepare_smooth_mask(mask, 50)
    y_sm = mask_blend(sm, y_masked, None)
    d.mask, d.mask_bs, d.dc_mask, d.dc_y = ptr(mask), 0, ptr(sm), ptr(y_sm)
    need = lib().babe_eval_workspace_bytes(ctypes.byref(d), 1)
    assert need >= plain
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dd, x_den = torch.empty_like(y), torch.empty_like(y)
    call = lambda nbytes: lib().babe_score_eval(ctypes.byref(d), ptr(y), 0.05, 0.5, 0.03, 10.0, -0.75, ptr(y), None, ptr(params), ptr(dd),
                                               ptr(x_den), None, ptr(ws), nbytes, 1, stream())
    dd.fill_(float("nan"))
    assert call(need - 1) < 0 and b"workspace" in lib().babe_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(dd).all()                               # nothing was launched
    assert call(need) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dd).all() and torch.isfinite(x_den).all()
    d.mask, d.dc_mask, d.dc_y = None, None, None
    assert lib().babe_eval_workspace_bytes(ctypes.byref(d), 1) == plain
