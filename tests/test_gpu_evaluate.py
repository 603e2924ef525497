"""The formal test end to end on the GPU at the reduced network shapes (Ns = [8,8,8,8,16,16,16], 92092 samples at 22050 Hz, T = 2,
weights from tests/golden/unet_small.npz): testing.evaluate.formal_test_bwe with the known filter and blind over three ~10 s
wavs, its resume rule, and python -m babe_amd.evaluate as a fresh child process with its own time limit (after a child that
faulted, aborted or hung nothing further is started from this module).  Needs a MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import metrics_cases as MC
from tests.train_fixtures import write_wavs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
NS, L, FS = [8, 8, 8, 8, 16, 16, 16], 92092, 22050
_fault = []                                            # why no further child may start
METRICS = ("lsd", "lsd_lf", "lsd_hf")


def child(cmd, timeout=300):
    """One fresh process; a fault, an abort or a time limit ends the module's GPU work (tests/test_gpu_train_cli.py::child)."""
    if _fault:
        pytest.fail(f"not started: an earlier child run of this module {_fault[0]}")
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _fault.append(f"ran into its time limit ({' '.join(cmd[-4:])})")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stderr:
        _fault.append(f"ended with status {r.returncode}")
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r


def state_dict():
    u = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(G, "unet_small.npz")).items()}
    return {k[3:]: v for k, v in u.items() if k.startswith("sd.")}


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from babe_amd.diff_params.edm import EDM
    from babe_amd.evaluate import default_eval_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    d = tmp_path_factory.mktemp("eval")
    paths = write_wavs(str(d / "wavs"), fs=FS, seconds=(10.0, 9.0, 8.0))
    args = default_eval_args(sample_rate=FS, audio_len=L, Ns=NS, T=2)
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(state_dict())
    smp = BlindSampler(net, EDM(args), args, batch_semantics="per_clip")
    return d, paths, smp


def read(path):
    from babe_amd.io import read_audio_file
    x, sr = read_audio_file(path)
    assert sr == FS and x.dtype == torch.float32
    return x


def lines_of(out):
    with open(os.path.join(str(out), "metrics.jsonl")) as f:
        return [json.loads(ln) for ln in f]


def check_outputs(out, paths, blind):
    from babe_amd import metrics as M
    lines = lines_of(out)
    assert [ln["name"] for ln in lines] == [os.path.splitext(os.path.basename(p))[0] for p in paths]
    for ln in lines:
        wav = {k: read(os.path.join(str(out), k, ln["name"] + ".wav")) for k in ("original", "degraded", "reconstructed")}
        assert wav["original"].shape == wav["degraded"].shape == wav["reconstructed"].shape == (ln["samples"],)
        assert os.path.isfile(os.path.join(str(out), "filters", ln["name"] + ".filter_data.pkl")) == blind
        vals = [ln[k + s] for k in METRICS for s in ("", "_degraded")]
        if blind:
            assert len(ln["filter_db_mse"]) == ln["segments"] in (2, 3)
            vals += ln["filter_db_mse"] + [ln["filter_db_mse_mean"]]
        assert all(np.isfinite(v) for v in vals), ln
        # the baseline column, recomputed from the float32 wavs that were written: the same bits
        again = M.lsd(wav["original"].cuda(), wav["degraded"].cuda(), nfft=2048, hop=512)
        assert float(again[0]) == ln["lsd_degraded"], (float(again[0]), ln["lsd_degraded"])
        assert ln["lsd_hf_degraded"] > ln["lsd_lf_degraded"]             # the test filter removes the high band
        assert ln["split_fc"] == 1000.0
    with open(os.path.join(str(out), "summary.json")) as f:
        assert json.load(f) == MC.summary_stats(lines)
    return lines


def test_a_sampler_that_returns_its_observation_reproduces_the_degraded_file(setup, monkeypatch):
    from babe_amd.testing.evaluate import formal_test_bwe
    d, paths, smp = setup
    monkeypatch.setattr(smp, "predict_bwe", lambda y, filt, filt_type: y.clone())
    out = d / "stub"
    s = formal_test_bwe(smp, paths, str(out), blind=False, batch_size=2)
    assert s["n"] == 3
    for ln in lines_of(out):
        deg, rec = read(os.path.join(str(out), "degraded", ln["name"] + ".wav")), read(os.path.join(str(out), "reconstructed", ln["name"] + ".wav"))
        err = float((deg - rec).abs().max())
        print(f"{ln['name']}: max |reconstructed - degraded| = {err:.3e}")
        assert err <= 1e-6                                               # the cross-fade halves sum to one
        for k in METRICS:
            assert abs(ln[k] - ln[k + "_degraded"]) <= MC.BAR, (k, ln[k], ln[k + "_degraded"])


def test_known_filter_run_then_nothing_left_to_do(setup, monkeypatch):
    from babe_amd.testing.evaluate import formal_test_bwe
    d, paths, smp = setup
    out = d / "known"
    s = formal_test_bwe(smp, paths, str(out), blind=False, batch_size=4)
    lines = check_outputs(out, paths, blind=False)
    assert s["n"] == 3 and s == MC.summary_stats(lines) and "filter_db_mse_mean" not in s
    calls = []
    real = smp.predict_bwe
    monkeypatch.setattr(smp, "predict_bwe", lambda *a, **k: calls.append(1) or real(*a, **k))
    before = open(os.path.join(str(out), "summary.json")).read()
    assert formal_test_bwe(smp, paths, str(out), blind=False) == s and calls == []
    assert open(os.path.join(str(out), "summary.json")).read() == before and lines_of(out) == lines


def test_blind_run(setup):
    from babe_amd.testing.evaluate import formal_test_bwe
    d, paths, smp = setup
    out = d / "blind"
    s = formal_test_bwe(smp, paths[1:], str(out), blind=True, batch_size=4)
    check_outputs(out, paths[1:], blind=True)
    assert s["n"] == 2 and np.isfinite(s["filter_db_mse_mean"]["mean"])
    with pytest.raises(ValueError):
        formal_test_bwe(smp, paths, str(out), blind=True, use_AR=True)


def test_command_line_in_a_child_process(setup):
    d, paths, _ = setup
    one = d / "one"
    write_wavs(str(one), fs=FS, seconds=(4.5, 0.1, 0.1))
    os.remove(str(one / "b_int16_stereo.wav"))
    os.remove(str(one / "c_float32_mono.wav"))
    sd = state_dict()
    torch.save({"it": 0, "network": sd, "ema": sd}, str(d / "init.pt"))
    cfg = d / "eval.yaml"
    cfg.write_text(f"exp:\n  sample_rate: {FS}\n  audio_len: {L}\nnetwork:\n  Ns: {NS}\n"
                   f"tester:\n  T: 2\n  formal_test:\n    path: {one}\n    folder: {d / 'cli'}\n    blind: True\n")
    r = child([sys.executable, "-m", "babe_amd.evaluate", "--config", str(cfg), "--ckpt", str(d / "init.pt"), "--batch", "2"])
    printed = json.loads(r.stdout.strip().splitlines()[-1])
    with open(d / "cli" / "summary.json") as f:
        assert printed == json.load(f)
    assert printed["n"] == 1 and np.isfinite(printed["lsd"]["mean"]) and np.isfinite(printed["filter_db_mse_mean"]["mean"])
    assert lines_of(d / "cli")[0]["segments"] == 2
    assert (d / "cli" / "reconstructed" / "a_int16_mono.wav").is_file()
