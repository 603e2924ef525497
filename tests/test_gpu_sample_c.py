"""csrc/sample.hip: a whole sampling run as ONE C-ABI call (babe_sample_bwe; BlindSampler(loop="library") through
testing/sample_c.py) against the Python loop sequencing the same kernels, bit for bit; the seeded runs on the library's
generator (csrc/randn.hip).  Fixture shape of tests/test_gpu_eval_c.py: the smallest on which the loop has all three kinds of
step - churned Heun, Heun, final Euler.  Needs a MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, L, FS, T = [8, 8, 8, 8, 16, 16, 16], 92092, 22050, 3


def _args():
    from babe_amd.config import default_args
    return default_args(sample_rate=FS, audio_len=L, Ns=NS, T=T, start_sigma=0.05)


@pytest.fixture(scope="module")
def world():
    """One network, one pair of observations and one set of T + 1 noise tensors for the whole file (never modified)."""
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    mp = pytest.MonkeyPatch()
    mp.setenv("BABE_CQT_C", "1")                       # the Python sequencer on the library's CQT plan (same tables)
    args = _args()
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(init_state_dict(NS, args.network.num_dils, seed=0, gate_scale=1.0))
    g = torch.Generator().manual_seed(5)
    y = (0.1 * torch.randn(2, L, generator=g)).cuda()
    noises = [torch.randn(2, L, generator=g) for _ in range(T + 1)]
    yield dict(net=net, y=y, noises=noises)
    mp.undo()


def _sampler(world, semantics="per_clip", variant=None, **kw):
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    args = _args()
    smp = BlindSampler(world["net"], EDM(args), args, batch_semantics=semantics, **kw)
    if variant == "order1":
        smp.order = 1
    elif variant == "nochurn":
        smp.diff_params.Schurn = 0
    elif variant == "cold":
        smp.start_sigma = None
    return smp


def _feed(smp, noises, B):
    """The sampler draws these tensors, in order, instead of torch.randn (as test_whole_sampler_run_on_the_library_evaluation)."""
    it = iter(noises)
    smp._randn = lambda shape, device: next(it)[:B].contiguous().to(device)


def _known_filter():
    return torch.tensor([[3000.0, 5000.0], [-20.0, -40.0]])


def _run(smp, y, blind, **kw):
    res = smp.predict_blind_bwe(y, **kw) if blind else (smp.predict_bwe(y, _known_filter(), "fc_A", **kw),)
    torch.cuda.synchronize()
    return tuple(r.clone() if torch.is_tensor(r) else r for r in res)


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.shape == v.shape and torch.isfinite(u).all()
        assert torch.equal(u, v), float((u - v).abs().max())


@pytest.mark.parametrize("B,semantics,blind,variant", [
    (1, "per_clip", True, None), (2, "per_clip", True, None), (2, "reference", True, None), (1, "per_clip", False, None),
    (1, "per_clip", True, "order1"), (2, "per_clip", True, "nochurn"), (1, "per_clip", True, "cold"), (2, "reference", True, "cold"),
])
def test_library_run_equals_the_python_loop_bit_for_bit(monkeypatch, world, B, semantics, blind, variant):
    """babe_sample_bwe on a [T+1][B][L] noise buffer = the Python loop fed the same tensors through _randn, in x and
    filter_params, with the Python side on the library evaluation (BABE_EVAL_C=1) and on its own sequencing (=0)."""
    import babe_amd.testing.blind_bwe_sampler as bs
    y = world["y"][:B].contiguous()
    lib_smp = _sampler(world, semantics, variant, loop="library")
    _feed(lib_smp, world["noises"], B)
    got = _run(lib_smp, y, blind)
    assert lib_smp._csample is not None and lib_smp._csample.calls == 1, "the library run did not run"
    for mode in (True, False):
        monkeypatch.setattr(bs, "EVAL_C", mode)
        py = _sampler(world, semantics, variant)
        _feed(py, world["noises"], B)
        want = _run(py, y, blind)
        assert py._csample is None
        _same(got, want)


def test_records_equal_those_of_the_python_loop(world):
    """rec_x_den / rec_params = data_denoised / data_filters of predict_blind_bwe(rid=True), bit for bit (per clip and with the
    reference's shared filter, whose records drop the clip axis)."""
    for semantics in ("per_clip", "reference"):
        res = []
        for loop in ("library", "python"):
            smp = _sampler(world, semantics, loop=loop)
            _feed(smp, world["noises"], 2)
            res.append(_run(smp, world["y"], True, rid=True))
        (x0, p0, den0, t0, f0), (x1, p1, den1, t1, f1) = res
        assert den0.shape == (T, 2, L) and f0.shape == ((T, 2, 2, 5) if semantics == "per_clip" else (T, 2, 5))
        assert not den0.is_cuda and not f0.is_cuda and torch.equal(t0, t1)
        _same((x0, p0, den0, f0), (x1, p1, den1, f1))


def test_seeded_run_equals_the_buffer_run_and_the_python_loop_on_the_generator(world):
    """noise = NULL under (seed, clip0) = the buffer run fed babe_randn(seed, clip0 + b, k) = loop="python" with
    noise_device="philox" under the same seed, bit for bit."""
    from babe_amd._lib import check, lib, stream
    seed, clip0, B = (1 << 35) + 17, 3, 2
    y = world["y"]
    seeded = _sampler(world, loop="library", seed=seed)
    got = _run(seeded, y, True, clip0=clip0)
    assert seeded._csample.calls == 1
    buf = torch.empty(T + 1, B, L, device="cuda")
    for k in range(T + 1):
        check(lib().babe_randn(buf[k].data_ptr(), L, B, L, seed, clip0, k, stream()), "randn")
    fed = _sampler(world, loop="library")
    _feed(fed, [b for b in buf], B)
    _same(got, _run(fed, y, True))
    py = _sampler(world, loop="python", noise_device="philox", seed=seed)
    _same(got, _run(py, y, True, clip0=clip0))
    assert py._csample is None
    other = _run(_sampler(world, loop="library", seed=seed + 1), y, True, clip0=clip0)
    assert not torch.equal(other[0], got[0])


def test_a_seeded_clip_does_not_depend_on_its_batch(world):
    """Per-clip semantics, B = 2: row 1 = the B = 1 run of that clip with clip0 = 1; the same through sub-batches of one
    (max_segments_in_flight = 1)."""
    seed, y = 77, world["y"]
    both = _run(_sampler(world, loop="library", seed=seed), y, True)
    one = _run(_sampler(world, loop="library", seed=seed), y[1:2].contiguous(), True, clip0=1)
    assert torch.equal(both[0][1], one[0][0]) and torch.equal(both[1][1], one[1].reshape(both[1][1].shape))
    sub = _sampler(world, loop="library", seed=seed, max_segments_in_flight=1)
    res = _run(sub, y, True)
    assert sub._csample.calls == 2
    _same(both, res)


def test_two_runs_on_two_streams_over_one_plan(world):
    """Two babe_sample_bwe runs enqueued on two streams, each with its own UNet state and workspace over the one plan = the
    same two runs one after the other."""
    from babe_amd.testing import sample_c
    smp = _sampler(world, loop="library", seed=5)
    y = world["y"]
    smp.stft_ops(L, y.device)
    runs = [sample_c.CSample(smp, lane) for lane in (0, 1)]
    assert runs[0].ce.cu.plan == runs[1].ce.cu.plan and runs[0].ce.cu.state != runs[1].ce.cu.state
    rows, t0, _ = sample_c.steps_from(smp.diff_params, T, smp.order, smp.start_sigma, 1.0)
    fp = smp._init_params(1, y.device)
    ys = [y[k:k + 1].contiguous() for k in (0, 1)]
    call = lambda k: runs[k](smp, ys[k], fp, True, rows, t0, True, None, 5, k)
    serial = [call(0), call(1)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in (0, 1)]
    conc = []
    for k in (0, 1):
        streams[k].wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(streams[k]):
            conc.append(call(k))
    for s in streams:
        s.synchronize()
    for k in (0, 1):
        _same(serial[k], conc[k])
    assert not torch.equal(serial[0][0], serial[1][0])


def test_unsupported_configurations_take_the_python_loop(world):
    """sample_c.supported is False - and the Python loop runs, no babe_sample_bwe call is made - for an attention network, a
    bf16 network, observation noise (SNR_observations) and a 'firwin' degradation; the default configuration makes one call."""
    from babe_amd.diff_params.edm import EDM
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    from babe_amd.testing import sample_c
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    from tests.attention_weights import FIXTURES, fixture_sd
    y = world["y"][:1].contiguous()
    calls = []
    real = sample_c.CSample.__call__
    mp = pytest.MonkeyPatch()
    mp.setattr(sample_c.CSample, "__call__", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    try:
        ok = _sampler(world, loop="library", seed=1)
        assert sample_c.supported(ok, y, True, False) and sample_c.supported(ok, y, True, True) and sample_c.supported(ok, y, False, False)
        assert not sample_c.supported(ok, y, False, True)          # the known-filter loop keeps other records
        _run(ok, y, True)
        assert len(calls) == 1 and ok._csample.calls == 1

        def python_loop_runs(smp, run=lambda s: _run(s, y, True)):
            n = len(calls)
            res = run(smp)
            assert len(calls) == n and smp._csample is None and torch.isfinite(res[0]).all()

        # an attention network
        Ns, fs, La, layers, adict = FIXTURES["a"]
        args = _args()
        args.network.attention_layers, args.network.attention_dict = list(layers), dict(adict)
        net = Unet_CQT_oct_with_attention(args, "cuda")
        net.load_state_dict(fixture_sd("a"), strict=True)
        smp = BlindSampler(net, EDM(args), args, loop="library", seed=1)
        assert not sample_c.supported(smp, y, True, False)
        python_loop_runs(smp)
        # a bf16 network
        args = _args()
        net = Unet_CQT_oct_with_attention(args, "cuda", precision="bf16")
        net.load_state_dict(init_state_dict(NS, args.network.num_dils, seed=0, gate_scale=1.0))
        smp = BlindSampler(net, EDM(args), args, loop="library", seed=1)
        assert not sample_c.supported(smp, y, True, False)
        python_loop_runs(smp)
        # observation noise
        args = _args()
        args.tester.posterior_sampling.SNR_observations = 50
        smp = BlindSampler(world["net"], EDM(args), args, loop="library", seed=1, noise_device="philox")
        assert not sample_c.supported(smp, y, True, False)
        python_loop_runs(smp)
        # a FIR degradation: supported() is asked while the degradation is set
        seen = []
        sup = sample_c.supported
        mp.setattr(sample_c, "supported", lambda *a: (seen.append(sup(*a)), seen[-1])[1])
        smp = _sampler(world, loop="library", seed=1, noise_device="philox")
        taps = torch.hann_window(33, periodic=False)
        python_loop_runs(smp, lambda s: (s.predict_bwe(y, taps / taps.sum(), "firwin"),))
        assert seen == [False]
    finally:
        mp.undo()


def test_restore_cli_is_a_function_of_the_seed(tmp_path):
    """python -m babe_amd.restore --loop library --seed 3, twice, on a 2-segment synthetic wav: byte-equal outputs, and different
    from --seed 4.  (One child process makes the three command-line runs, on the reduced network: the path is what is
    exercised, and the process start and the weight packing are paid once.)"""
    from scipy.io import wavfile
    n = L + 30000                                                        # two segments of L samples
    t = np.arange(n) / FS
    x = (0.2 * np.sin(2 * np.pi * 440 * t) + 0.05 * np.sin(2 * np.pi * 3000 * t)).astype(np.float32)
    wav = str(tmp_path / "in.wav")
    wavfile.write(wav, FS, x)
    outs = [str(tmp_path / d) for d in ("a", "b", "c")]
    code = ("import sys; import babe_amd.config as c; _d = c.default_args; "
            "c.default_args = lambda **k: _d(**dict(k, Ns=[8, 8, 8, 8, 16, 16, 16])); "
            "from babe_amd import restore\n"
            "for out, seed in zip(%r, ('3', '3', '4')):\n"
            "    sys.argv = ['restore', %r, out, '--T', '3', '--sample-rate', '%d', '--audio-len', '%d', '--batch', '2', "
            "'--loop', 'library', '--seed', seed]\n"
            "    restore.main()\n") % (outs, wav, FS, L)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b, c = (open(os.path.join(o, "in.wav"), "rb").read() for o in outs)
    assert len(a) > 44 + 2 * n and a == b and a != c
    sr, yv = wavfile.read(os.path.join(outs[0], "in.wav"))
    assert sr == FS and yv.shape[0] == n and np.isfinite(yv).all() and yv.std() > 0
