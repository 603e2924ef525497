"""Segments per second from ONE MaestroDataset_fs process, reading only the crop (memory-mapped wav) against reading the whole
file for every group of eight crops (what the reference does).  Host work only; no GPU is touched.

    python tools/loader_bench.py [--files 10] [--minutes 10] [--seg 368368] [--segments 400] [--keep DIR]

It writes `--files` wavs of `--minutes` minutes, 16-bit stereo 44.1 kHz (the MAESTRO format, about 106 MB each), with a
maestro-v3.0.0.csv into a temporary directory, then times `--segments` items of each reader after 16 warm-up ones, and prints one
JSON document.  The yardstick: the fastest recorded training step consumes 4 segments per 168 ms, 24 segments/s
(profiles/train_bench_wgrad_bf16.json); the loader shares the host's CPUs with the training process, so `ok` asks the crop
reader for twice that from one process.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NEED = 24.0                                            # segments/s one training process consumes (4 per 168 ms)


def write_set(root, n_files, minutes, fs=44100):
    from scipy.io import wavfile
    os.makedirs(os.path.join(root, "2017"), exist_ok=True)
    rng = np.random.RandomState(0)
    block = (rng.randn(fs * 10, 2) * 3000).astype(np.int16)                    # 10 s of noise, repeated
    x = np.tile(block, (minutes * 6, 1))
    rows = ["canonical_composer,canonical_title,split,year,midi_filename,audio_filename,duration"]
    for i in range(n_files):
        name = f"2017/file_{i:02d}.wav"
        wavfile.write(os.path.join(root, name), fs, np.roll(x, i * 977, axis=0))
        rows.append(f"c,t,train,2017,x.midi,{name},{minutes * 60}")
    with open(os.path.join(root, "maestro-v3.0.0.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")
    return x.nbytes


def rate(root, seg, n, crop_reads):
    from babe_amd.config import to_attr
    from babe_amd.datasets import MaestroDataset_fs
    ds = MaestroDataset_fs(to_attr(dict(path=root, years=[2017], load_len=seg)), seed=42)
    ds.crop_reads = crop_reads
    it = iter(ds)
    for _ in range(16):
        next(it)
    t0 = time.perf_counter()
    for _ in range(n):
        s, sr = next(it)
    dt = time.perf_counter() - t0
    assert s.shape == (seg,) and s.dtype == np.float32 and sr == 44100
    return n / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=10)
    ap.add_argument("--minutes", type=int, default=10)
    ap.add_argument("--seg", type=int, default=368368)
    ap.add_argument("--segments", type=int, default=400)
    ap.add_argument("--keep", default=None, help="write the files here and leave them")
    a = ap.parse_args()
    root = a.keep or tempfile.mkdtemp(prefix="loader_bench_")
    try:
        nbytes = write_set(root, a.files, a.minutes)
        crop = rate(root, a.seg, a.segments, True)
        whole = rate(root, a.seg, max(a.segments // 4, 16), False)
    finally:
        if not a.keep:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps({"files": a.files, "file_MB": round(nbytes / 1e6, 1), "segment_samples": a.seg,
                      "crop_reader_segments_per_s": round(crop, 1), "whole_file_reader_segments_per_s": round(whole, 1),
                      "needed_segments_per_s": NEED, "bar_segments_per_s": 2 * NEED, "ok": bool(crop >= 2 * NEED),
                      "cpus_available": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None}, indent=1))


if __name__ == "__main__":
    main()
