"""Declipping, compressed sensing and phase retrieval of testing/edm_sampler.Sampler, host side: frame counts, argument
refusals and the fixture file (tests/golden/make_edm_tasks_golden.py).  No GPU needed."""
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")


class _NoNet:
    CQTransform = None


def _sampler(xi=0.25, data_consistency=False, audio_len=92092, phase_retrieval=None):
    from babe_amd.config import default_args, to_attr
    from babe_amd.diff_params.edm import EDM
    from babe_amd.testing.edm_sampler import Sampler
    args = default_args(sample_rate=22050, audio_len=audio_len, T=3, xi=xi)
    args.tester.posterior_sampling.data_consistency = data_consistency
    if phase_retrieval is not None:
        args.tester.phase_retrieval = to_attr(phase_retrieval)
    return Sampler(_NoNet(), EDM(args), args)


@pytest.mark.parametrize("L,win,hop", [(92092, 1024, 256), (1000, 256, 64), (100, 256, 64), (1024, 256, 256)])
def test_frame_count_and_out_shape_are_torch_stfts(L, win, hop):
    from babe_amd.degrade import STFTMagnitudeDegradation, stft_mag_frames
    x = torch.cat((torch.zeros(1, L), torch.zeros(1, win)), -1)
    want = torch.stft(x, win, hop_length=hop, window=torch.hamming_window(win), center=False, return_complex=True).shape[1:]
    deg = STFTMagnitudeDegradation(win, hop, L, "cpu")
    assert deg.out_shape() == tuple(want) == (win // 2 + 1, 1 + L // hop)
    assert stft_mag_frames(L, hop) == want[1]


def test_stft_magnitude_degradation_refuses_bad_sizes_and_cpu_tensors():
    from babe_amd.degrade import ClipDegradation, STFTMagnitudeDegradation, clip_residual
    for win in (128, 8192, 1000, 0, 384):
        with pytest.raises(ValueError, match="power of two"):
            STFTMagnitudeDegradation(win, 64, 1000, "cpu")
    for hop in (0, -1, 257):
        with pytest.raises(ValueError, match="hop"):
            STFTMagnitudeDegradation(256, hop, 1000, "cpu")
    assert STFTMagnitudeDegradation(256, 256, 1000, "cpu").out_shape() == (129, 4)
    assert STFTMagnitudeDegradation(4096, 1, 10, "cpu").out_shape() == (2049, 11)
    deg = STFTMagnitudeDegradation(256, 64, 1000, "cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        deg.fwd(torch.zeros(1, 1000))
    with pytest.raises(RuntimeError, match="GPU only"):
        deg.adj(torch.zeros(1, 129 * 16))
    with pytest.raises(NotImplementedError, match="data-consistency"):
        deg.fwd_dc(torch.zeros(1, 1000))
    with pytest.raises(ValueError, match=">= 0"):
        ClipDegradation(-0.1)
    with pytest.raises(RuntimeError, match="GPU only"):
        ClipDegradation(0.5).fwd(torch.zeros(1, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        ClipDegradation(0.5).residual(torch.zeros(1, 8), torch.zeros(1, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        clip_residual(torch.zeros(1, 8), torch.zeros(1, 8), 0.5)


@pytest.mark.parametrize("call", [lambda s: s.predict_declipping(torch.zeros(1, 92092), 0.1),
                                  lambda s: s.predict_compsens(torch.zeros(1, 92092), torch.ones(92092)),
                                  lambda s: s.predict_pr(torch.zeros(1, 513, 360))], ids=["declipping", "compsens", "pr"])
def test_tasks_refuse_a_run_without_guidance(call):
    with pytest.raises(ValueError, match="xi"):
        call(_sampler(xi=0))


def test_tasks_refuse_data_consistency():
    s = _sampler(data_consistency=True)
    with pytest.raises(ValueError, match="data_consistency"):
        s.predict_declipping(torch.zeros(1, 92092), 0.1)
    with pytest.raises(ValueError, match="data_consistency"):
        s.predict_compsens(torch.zeros(1, 92092), torch.ones(92092))
    with pytest.raises(NotImplementedError, match="data_consistency"):
        s.predict_pr(torch.zeros(1, 513, 360))
    assert s.degradation is None


def test_predict_pr_checks_the_observations_shape_and_reads_its_defaults():
    s = _sampler()                                                 # (default_args has no tester.phase_retrieval: 1024 / 256)
    with pytest.raises(ValueError, match=r"\(B, 513, 360\)"):
        s.predict_pr(torch.zeros(1, 513, 359))
    with pytest.raises(ValueError, match=r"\(B, 513, 360\)"):
        s.predict_pr(torch.zeros(1, 92092))
    with pytest.raises(ValueError, match=r"\(B, 129, 1439\)"):
        s.predict_pr(torch.zeros(1, 513, 360), win_size=256, hop_size=64)
    s = _sampler(phase_retrieval=dict(win_size=512, hop_size=128))
    with pytest.raises(ValueError, match=r"\(B, 257, 720\)"):
        s.predict_pr(torch.zeros(1, 513, 360))
    with pytest.raises(ValueError, match="power of two"):
        s.predict_pr(torch.zeros(1, 513, 360), win_size=1000)
    assert s.degradation is None


def test_fixture_file_keys_and_shapes():
    d = {k: np.asarray(v) for k, v in np.load(os.path.join(G, "edm_sampler_tasks.npz")).items()}
    L, T = 92092, 3
    stride, xs = int(d["stride"]), int(d["x_stride"])
    assert (stride, xs, int(d["win"]), int(d["hop"])) == (16, 2, 1024, 256) and L % int(d["hop"]) != 0
    assert d["t"].shape == (T + 1,) and float(d["t"][-1]) == 0.0
    for task in ("declip", "compsens", "pr"):
        assert d[f"{task}_x"].shape == (1, len(range(0, L, xs))) and d[f"{task}_x"].dtype == np.float32
        assert d[f"{task}_den"].shape == (T, 1, len(range(0, L, stride)))
        assert np.isfinite(d[f"{task}_x"]).all() and np.isfinite(d[f"{task}_den"]).all()
    assert 0.05 <= float(d["declip_clipped"]) <= 0.50
    assert float(d["keep"]) == 0.05 and float(d["xi"]) > 0
    assert os.path.getsize(os.path.join(G, "edm_sampler_tasks.npz")) < 1 << 20
