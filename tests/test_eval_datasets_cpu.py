"""The evaluation flow without a GPU: the test-split datasets on synthetic wavs and a synthetic MAESTRO csv, the command line's
key resolution and its "no items" exit, and the bookkeeping of testing.evaluate.formal_test_bwe with a stub sampler on the CPU
(the LSD call replaced by the float64 statement of tests/metrics_cases.py)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import metrics_cases as MC
from tests.train_fixtures import write_wavs


def whole(path):
    from babe_amd.datasets.segments import open_wav, to_mono_float
    sr, x = open_wav(path)
    return sr, to_mono_float(x)


# ------------------------------------------------------------------------------------------------------------ datasets
def test_audiofolder_test_set(tmp_path):
    from babe_amd.config import to_attr
    from babe_amd.datasets import AudioFolderDatasetTest, resolve
    paths = write_wavs(str(tmp_path / "w"), fs=8000, seconds=(4.0, 3.5, 3.0))
    assert resolve("datasets.audiofolder_test.AudioFolderDatasetTest") is AudioFolderDatasetTest
    ds = AudioFolderDatasetTest(to_attr({"test": {"path": str(tmp_path / "w"), "stereo": False}}), fs=8000, seg_len=10000,
                                num_samples=2, seed=7)
    assert len(ds) == 2 and isinstance(ds, torch.utils.data.Dataset) and not isinstance(ds, torch.utils.data.IterableDataset)
    rng = np.random.RandomState(7)                                 # one draw per file, in the sorted order of the files
    for i, p in enumerate(paths[:2]):
        seg, fs, name = ds[i]
        sr, x = whole(p)
        idx = rng.randint(0, len(x) - 10000)
        assert name == os.path.basename(p) and fs == sr == 8000
        assert seg.dtype == np.float32 and seg.shape == (10000,) and np.array_equal(seg, x[idx:idx + 10000])
    assert [ds[i][2] for i in range(2)] == ["a_int16_mono.wav", "b_int16_stereo.wav"]       # sorted; b is the stereo file
    # a segment longer than the files: tiled, as in the reference
    ds = AudioFolderDatasetTest(to_attr({"test": {"path": str(tmp_path / "w")}}), fs=8000, seg_len=50000, num_samples=8)
    assert len(ds) == 3
    sr, x = whole(paths[2])
    assert np.array_equal(ds[2][0], np.tile(x, 3)[:50000])
    with pytest.raises(ValueError):
        AudioFolderDatasetTest(to_attr({"test": {"path": str(tmp_path / "empty")}}))
    with pytest.raises(NotImplementedError):
        AudioFolderDatasetTest(to_attr({"test": {"path": str(tmp_path / "w"), "stereo": True}}))


def test_maestro_test_chunks(tmp_path):
    from babe_amd.config import to_attr
    from babe_amd.datasets import MaestroDatasetTestChunks, resolve
    root = tmp_path / "maestro"
    fs = 800
    write_wavs(str(root / "2004"), fs=fs, seconds=(12.0, 11.5, 11.0))
    write_wavs(str(root / "2006"), fs=fs, seconds=(12.5, 11.5, 11.0), seed=1)
    rows = [("train", 2004, "2004/c_float32_mono.wav"), ("test", 2006, "2006/b_int16_stereo.wav"),
            ("test", 2004, "2004/b_int16_stereo.wav"), ("validation", 2004, "2004/a_int16_mono.wav"),
            ("test", 2004, "2004/a_int16_mono.wav"), ("test", 2011, "2011/not_there.wav"), ("train", 2006, "2006/a_int16_mono.wav")]
    with open(root / "maestro-v3.0.0.csv", "w") as f:
        f.write("canonical_composer,canonical_title,split,year,midi_filename,audio_filename,duration\n")
        for split, year, name in rows:
            f.write(f'"Composer, A.",Title,{split},{year},{name[:-4]}.midi,{name},12.0\n')
    assert resolve("datasets.maestro_dataset_test.MaestroDatasetTestChunks") is MaestroDatasetTestChunks
    args = to_attr({"path": str(root), "years": [2004, 2006], "load_len": 1000})
    ds = MaestroDatasetTestChunks(args, num_samples=4)
    want = ["2004/a_int16_mono.wav", "2004/b_int16_stereo.wav", "2006/b_int16_stereo.wav"]          # test rows of the years, sorted
    assert ds.filelist == [os.path.join(str(root), w) for w in want] and len(ds) == 3
    for i, w in enumerate(want):
        seg, sr, name = ds[i]
        _, x = whole(os.path.join(str(root), w))                   # (the stereo files: the mean of the two channels)
        assert sr == fs and name == os.path.basename(w)
        assert seg.dtype == np.float32 and seg.shape == (1000,) and np.array_equal(seg, x[10 * fs:10 * fs + 1000])
    assert len(MaestroDatasetTestChunks(args, num_samples=2)) == 2
    assert MaestroDatasetTestChunks(to_attr(dict(args, years=[2006])), num_samples=4).filenames == ["b_int16_stereo.wav"]
    with pytest.raises(ValueError):                                # 10 s + 1500 samples: beyond the end of the 11.5 s file
        MaestroDatasetTestChunks(to_attr(dict(args, load_len=1500)), num_samples=4)
    with pytest.raises(ValueError):
        MaestroDatasetTestChunks(to_attr(dict(args, years=[2018])))


# -------------------------------------------------------------------------------------------------------- command line
def test_command_line_key_resolution_and_no_items_exit(tmp_path, capsys):
    from babe_amd import evaluate as E
    wavs = tmp_path / "wavs"
    write_wavs(str(wavs), fs=8000, seconds=(1.0, 1.0, 1.0))
    cfg = tmp_path / "eval.yaml"
    cfg.write_text(f"exp:\n  sample_rate: 22050\n  audio_len: 92092\nnetwork:\n  Ns: [8, 8, 8, 8, 16, 16, 16]\n"
                   f"tester:\n  T: 2\n  formal_test:\n    path: {wavs}\n    folder: {tmp_path / 'out'}\n    blind: False\n"
                   f"  blind_bwe:\n    test_filter:\n      fc: [1500]\n      A: [-30]\n")
    a = E.load_config(str(cfg), ["tester.formal_test.OLA=128", "tester.bandwidth_extension.filter.fc=2000"])
    ft = a.tester.formal_test
    assert (ft.path, ft.folder, ft.blind, ft.use_AR, ft.OLA) == (str(wavs), str(tmp_path / "out"), False, False, 128)
    assert a.tester.blind_bwe.test_filter == {"fc": [1500], "A": [-30]} and a.tester.T == 2
    assert a.tester.blind_bwe.NFFT == 4096 and a.tester.blind_bwe.initial_conditions.fc[0] == 280      # defaults kept
    assert a.tester.bandwidth_extension.filter.fc == 2000 and a.tester.bandwidth_extension.filter.type == "firwin"
    assert a.exp.sample_rate == 22050 and a.network.Ns == [8, 8, 8, 8, 16, 16, 16]
    d = E.default_eval_args()
    assert d.tester.formal_test.blind is True and d.tester.blind_bwe.test_filter == {"fc": [1000], "A": [-20]}
    items = E.find_items(a)
    assert [os.path.basename(p) for p in items] == ["a_int16_mono.wav", "b_int16_stereo.wav", "c_float32_mono.wav"]
    # a dset_test section is used instead of the folder
    b = E.load_config(str(cfg), ["dset_test.callable=datasets.audiofolder_test.AudioFolderDatasetTest",
                                 f"dset_test.test.path={wavs}", "dset_test.num_samples=2", "exp.audio_len=4000"])
    ds = E.find_items(b)
    assert len(ds) == 2 and ds[0][0].shape == (4000,) and ds[1][2] == "b_int16_stereo.wav"
    # nothing to evaluate: exit status 2, before anything touches a GPU
    assert E.main(["--config", str(cfg), f"tester.formal_test.path={tmp_path / 'nothing'}"]) == 2
    assert E.main(["--config", str(cfg), "dset_test.callable=datasets.audiofolder_test.AudioFolderDatasetTest",
                   f"dset_test.test.path={tmp_path / 'nothing'}"]) == 2
    assert "no item found" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                # use_AR with blind is refused on the command line too
        E.main(["--config", str(cfg), "tester.formal_test.use_AR=True", "tester.formal_test.blind=True"])


# -------------------------------------------------------------------------------------------------------------- driver
FS, SEG = 8000, 12000


class StubSampler:
    """Stands in for BlindSampler on the CPU: halves the signal as its 'filter', returns its observations as the restoration."""

    def __init__(self):
        from babe_amd.evaluate import default_eval_args
        self.args = default_eval_args()
        self.args.exp.sample_rate, self.args.exp.audio_len = FS, SEG
        self.args.tester.blind_bwe.test_filter.fc = [1000, 2000]
        self.args.tester.blind_bwe.test_filter.A = [-20, -40]
        self.calls = []

    def apply_filter_fcA(self, x, fp):
        assert tuple(fp.shape) == (2, 2) and fp.dtype == torch.float32
        return 0.5 * x

    def predict_bwe(self, y, filt, filt_type):
        self.calls.append(("bwe", tuple(y.shape), filt_type))
        return y.clone()

    def predict_blind_bwe(self, y):
        self.calls.append(("blind", tuple(y.shape)))
        return y.clone(), torch.tensor([[900.0, 2100.0], [-18.0, -35.0]]).repeat(y.shape[0], 1, 1)


@pytest.fixture
def cpu_metrics(monkeypatch):
    """babe_amd.metrics' two GPU calls replaced by float64 numpy on the CPU tensors the driver passes."""
    from babe_amd import metrics as M

    def lsd_split(ref, est, fs, fc, nfft=2048, hop=512, floor=1e-10):
        r, e = ref.numpy(), est.numpy()
        ks = M.split_bin(fc, fs, nfft)
        f = lambda lo, hi: torch.from_numpy(MC.lsd64(r, e, nfft, hop, lo, hi, floor)[0])
        return dict(lsd=f(0, nfft // 2 + 1), lsd_lf=f(0, ks), lsd_hf=f(ks, nfft // 2 + 1))

    def filter_db_mse(fp_true, fp_est, fs, nfft):
        return (fp_true.reshape(1, -1) - fp_est.reshape(fp_est.shape[0], -1)).pow(2).mean(-1)

    monkeypatch.setattr(M, "lsd_split", lsd_split)
    monkeypatch.setattr(M, "filter_db_mse", filter_db_mse)


def read_lines(out):
    with open(os.path.join(out, "metrics.jsonl")) as f:
        return [json.loads(ln) for ln in f]


def test_driver_bookkeeping_with_a_stub_sampler(tmp_path, cpu_metrics):
    from babe_amd.io import read_audio_file
    from babe_amd.testing.evaluate import formal_test_bwe
    from babe_amd.testing.long_file import plan_segments
    paths = write_wavs(str(tmp_path / "w"), fs=FS, seconds=(4.0, 3.5, 3.0))
    out = str(tmp_path / "out")
    smp = StubSampler()
    with pytest.raises(ValueError):                                # use_AR + blind: refused before anything is written
        formal_test_bwe(smp, paths, out, blind=True, use_AR=True, device="cpu")
    assert not os.path.exists(out)
    s = formal_test_bwe(smp, paths[:2], out, blind=True, batch_size=2, device="cpu")
    lines = read_lines(out)
    assert [ln["name"] for ln in lines] == ["a_int16_mono", "b_int16_stereo"] and s["n"] == 2
    for ln, p in zip(lines, paths):
        x, fs = read_audio_file(p)
        nseg = len(plan_segments(len(x), SEG, 200, 256))
        assert ln["segments"] == nseg and len(ln["filter_db_mse"]) == nseg and ln["split_fc"] == 1000.0 and ln["blind"] is True
        for sub, want in (("original", x), ("degraded", 0.5 * x), ("reconstructed", 0.5 * x)):
            got, sr = read_audio_file(os.path.join(out, sub, ln["name"] + ".wav"))
            assert sr == FS and got.dtype == torch.float32 and got.shape == x.shape
            assert float((got - want).abs().max()) <= 1e-6        # the stub restores its observations: the cross-fade sums to one
        assert os.path.isfile(os.path.join(out, "filters", ln["name"] + ".filter_data.pkl"))
        # est = ref / 2 in every bin: 2 log10 2
        for k in ("lsd", "lsd_lf", "lsd_hf", "lsd_degraded", "lsd_lf_degraded", "lsd_hf_degraded"):
            assert abs(ln[k] - 2 * np.log10(2.0)) < 1e-6, (k, ln[k])
    assert sum(c[1][0] for c in smp.calls) == sum(ln["segments"] for ln in lines) and {c[0] for c in smp.calls} == {"blind"}
    assert max(c[1][0] for c in smp.calls) <= 2                    # batch_size
    with open(os.path.join(out, "summary.json")) as f:
        on_disk = json.load(f)
    assert on_disk == s == MC.summary_stats(lines)
    # second run over all three files: the two finished items are passed over, yet counted through their lines
    smp.calls.clear()
    s2 = formal_test_bwe(smp, paths, out, blind=True, batch_size=2, device="cpu")
    lines2 = read_lines(out)
    assert lines2[:2] == lines and [ln["name"] for ln in lines2] == ["a_int16_mono", "b_int16_stereo", "c_float32_mono"]
    assert sum(c[1][0] for c in smp.calls) == lines2[2]["segments"]
    assert s2["n"] == 3 and s2 == MC.summary_stats(lines2)
    # third run: nothing left to do, the sampler is not called, summary.json is unchanged
    smp.calls.clear()
    before = open(os.path.join(out, "summary.json")).read()
    assert formal_test_bwe(smp, paths, out, blind=True, device="cpu") == s2 and smp.calls == []
    assert open(os.path.join(out, "summary.json")).read() == before
    # known filter, from a dataset instead of paths
    from babe_amd.config import to_attr
    from babe_amd.datasets import AudioFolderDatasetTest
    ds = AudioFolderDatasetTest(to_attr({"test": {"path": str(tmp_path / "w")}}), fs=FS, seg_len=SEG + 500, num_samples=2)
    out2 = str(tmp_path / "out2")
    s3 = formal_test_bwe(smp, ds, out2, blind=False, device="cpu")
    assert s3["n"] == 2 and {c[0] for c in smp.calls} == {"bwe"} and {c[2] for c in smp.calls} == {"fc_A"}
    assert "filter_db_mse_mean" not in s3 and not os.path.exists(os.path.join(out2, "filters"))
    assert all("segments" not in ln and ln["samples"] == SEG + 500 for ln in read_lines(out2))
