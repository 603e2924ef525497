"""Formal bandwidth-extension test of a prior over a folder or a test split: degrade every item with the configured test filter,
restore it blind or with the known filter, write the audio and the objective metrics.

Restates BlindTester.formal_test_bwe (testing/blind_bwe_tester.py:321-577 of the reference) on the pieces this tree already has:
the degradation is applied to the whole signal at its own rate (:387-391), the result goes fs -> exp.sample_rate (:410), and the
segment loop with its cross-fade (:421-566) is testing/long_file.py.  Like the reference's formal test nothing is normalised
(`normalize_std` scales in and out the way babe_amd.restore does); an item whose reconstruction already exists is passed over
(:378-385).  What the reference leaves to listening tests is measured here: log-spectral distance (babe_amd.metrics, this
project's definition) of the reconstruction and of the degraded signal against the original, whole band and on either side of
the filter's cut-off, and for blind runs the dB error of the estimated filter (testing/blind_bwe_tester_small.py:398-404).

Files under out_dir: original/, degraded/, reconstructed/ <name>.wav (float32, exp.sample_rate), filters/<name>.filter_data.pkl
(blind), metrics.jsonl (one JSON object per item, appended) and summary.json (n, mean and standard deviation of every metric over
ALL lines of metrics.jsonl: items passed over on this run count through the lines earlier runs wrote)."""
import json
import os

import numpy as np
import torch

from .. import metrics as M
from ..io import read_audio_file, write_audio_file, write_filter_data
from ..utils import bandwidth_extension as utils_bwe
from .long_file import restore_file, restore_file_AR

LSD_KW = dict(nfft=2048, hop=512, floor=1e-10)


def is_metric(key):
    """The keys of a metrics.jsonl line that summary.json averages."""
    return key.startswith("lsd") or key == "filter_db_mse_mean"


def formal_filter(args, typefilter):
    """(filter, type, split frequency) of the degradation: 'fc_A' takes tester.blind_bwe.test_filter.{fc, A} as breakpoints
    [2,K] (:335-337); anything else designs tester.bandwidth_extension.filter (:343-346)."""
    if typefilter == "fc_A":
        tf = args.tester.blind_bwe.test_filter
        fc, A = np.atleast_1d(np.asarray(tf.fc, dtype=np.float32)), np.atleast_1d(np.asarray(tf.A, dtype=np.float32))
        return torch.from_numpy(np.stack([fc, A])), "fc_A", float(fc[0])
    ftype = args.tester.bandwidth_extension.filter.type
    if ftype in ("resample", "decimate"):
        raise NotImplementedError(f"formal_test_bwe: a {ftype!r} degradation changes the length of the signal; the metrics compare "
                                  "signals of one length")
    return utils_bwe.prepare_filter(args, args.exp.sample_rate), ftype, float(args.tester.bandwidth_extension.filter.fc)


def _items(items):
    """(name, loader) pairs; loader() -> (float32 tensor [L], fs).  A dataset item is (segment, fs, filename)."""
    if isinstance(items, (list, tuple)):
        for p in items:
            yield os.path.splitext(os.path.basename(p))[0], (lambda p=p: read_audio_file(p))
    else:
        for i in range(len(items)):
            seg, fs, filename = items[i]
            seg = np.asarray(seg, dtype=np.float32)
            seg = seg.mean(axis=0) if seg.ndim == 2 else seg
            yield os.path.splitext(os.path.basename(filename))[0], (lambda seg=seg, fs=fs: (torch.from_numpy(seg.copy()), int(fs)))


def summarize(out_dir):
    """Write and return summary.json from every line of metrics.jsonl."""
    path = os.path.join(out_dir, "metrics.jsonl")
    lines = []
    if os.path.exists(path):
        with open(path) as f:
            lines = list({ln["name"]: ln for ln in (json.loads(t) for t in f if t.strip())}.values())
    summary = {"n": len(lines)}
    for k in sorted({k for ln in lines for k in ln if is_metric(k)}):
        v = np.array([ln[k] for ln in lines if k in ln], dtype=np.float64)
        summary[k] = {"mean": float(v.mean()), "std": float(v.std())}
    with open(os.path.join(out_dir, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1, sort_keys=True)
    return summary


def formal_test_bwe(sampler, items, out_dir, *, blind, typefilter="fc_A", use_AR=False, batch_size=8, lsd_kw=None,
                    normalize_std=None, device="cuda"):
    """sampler: a BlindSampler (its args give exp.sample_rate, exp.audio_len and the tester section).  items: a list of wav paths,
    or a map-style dataset of (segment, fs, filename) (datasets.AudioFolderDatasetTest, MaestroDatasetTestChunks).  blind: restore
    with predict_blind_bwe and record the estimated filters; otherwise with the known test filter, segment batches of
    `batch_size` - or, with use_AR, autoregressively (restore_file_AR); use_AR with blind is a ValueError, as the reference asserts.
    Returns the summary dict (also in out_dir/summary.json)."""
    if use_AR and blind:
        raise ValueError("formal_test_bwe: use_AR needs the known filter (the reference asserts `not blind`)")
    args = sampler.args
    sr = int(args.exp.sample_rate)
    da_filter, ftype, split_fc = formal_filter(args, typefilter)
    filt_dev = da_filter.to(device) if torch.is_tensor(da_filter) else da_filter
    kw = dict(LSD_KW, **(lsd_kw or {}))
    os.makedirs(out_dir, exist_ok=True)
    dirs = {k: os.path.join(out_dir, k) for k in ("original", "degraded", "reconstructed", "filters")}
    for name, load in _items(items):
        if os.path.exists(os.path.join(dirs["reconstructed"], name + ".wav")):
            continue
        x, fs = load()
        D = x.to(device).float().reshape(1, -1)
        if ftype == "fc_A":
            degraded = sampler.apply_filter_fcA(D, filt_dev)
        else:
            degraded = utils_bwe.apply_low_pass(D, filt_dev, ftype)
        if fs != sr:
            from ..resample import resample
            D, degraded = resample(D, fs, sr), resample(degraded, fs, sr)
        orig, y = D[0].contiguous(), degraded[0].contiguous()
        scale = 1.0
        if normalize_std is not None:
            scale = float(normalize_std) / float(y.std())
        if blind:
            out, filt = restore_file(sampler, y * scale, batch_size)
        elif use_AR:
            overlap_s = args.tester.get("formal_test", {}).get("overlap", 0.25)
            out, filt = restore_file_AR(sampler, y * scale, filt_dev, ftype, overlap_s=overlap_s), None
        else:
            out, filt = restore_file(sampler, y * scale, batch_size, blind=False, filt=filt_dev, filt_type=ftype)
        rec = (out / scale).float().contiguous()
        write_audio_file(orig, sr, name, dirs["original"])
        write_audio_file(y, sr, name, dirs["degraded"])
        line = {"name": name, "fs": int(fs), "samples": int(orig.shape[-1]), "blind": bool(blind), "filter_type": ftype,
                "split_fc": split_fc}
        for suffix, est in (("", rec), ("_degraded", y)):
            for k, v in M.lsd_split(orig.unsqueeze(0), est.unsqueeze(0), sr, split_fc, **kw).items():
                line[k + suffix] = float(v[0])
        if blind:
            write_filter_data(filt, dirs["filters"], name)
            line["segments"] = len(filt)
            if ftype == "fc_A":
                mse = M.filter_db_mse(da_filter, torch.stack([f.reshape(2, -1) for _, f in filt]), sr, int(args.tester.blind_bwe.NFFT))
                line["filter_db_mse"] = [float(v) for v in mse]
                line["filter_db_mse_mean"] = float(np.mean(line["filter_db_mse"]))
        with open(os.path.join(out_dir, "metrics.jsonl"), "a") as f:
            f.write(json.dumps(line) + "\n")
        # the reconstruction is written last: its presence is what marks the item as done (a run that dies between the two
        # lines repeats the item, and summarize keeps the later of two lines with one name)
        write_audio_file(rec, sr, name, dirs["reconstructed"])
    return summarize(out_dir)
