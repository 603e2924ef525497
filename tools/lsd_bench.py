"""Time of the log-spectral distance at an evaluation batch's shape, B = 8 segments of 368368 samples, nfft 2048, hop 512:
babe_lsd_frames (csrc/metrics.hip, frame values + clip means, two launches) against the same quantity composed from two
torch.stft calls and torch element-wise ops.  Each variant is timed with device events over windows of N calls after a warm-up,
the two alternated; the median window is reported, with the spread.  The outputs are compared first.

    python tools/lsd_bench.py [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L, NFFT, HOP, FLOOR = 8, 368368, 2048, 512, 1e-10
N, WINDOWS, WARM = 200, 11, 20


def window_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from babe_amd._lib import check, lib, ptr, stream
    gen = torch.Generator().manual_seed(0)
    ref = (0.1 * torch.randn(B, L, generator=gen)).cuda()
    est = (ref + 0.01 * torch.randn(B, L, generator=gen).cuda()).contiguous()
    T = lib().babe_lsd_num_frames(L, NFFT, HOP)
    frames, clip = torch.empty(B, T, device="cuda"), torch.empty(B, device="cuda")
    win = torch.hann_window(NFFT, device="cuda")
    s = stream()

    def fused():
        check(lib().babe_lsd_frames(ptr(ref), L, ptr(est), L, L, B, NFFT, HOP, 0, NFFT // 2 + 1, FLOOR, ptr(frames), ptr(clip), s),
              "lsd_frames")
        return clip

    def composed():
        kw = dict(n_fft=NFFT, hop_length=HOP, window=win, center=False, return_complex=True)
        pr = torch.stft(ref, **kw).abs().square().clamp_min(FLOOR)
        pe = torch.stft(est, **kw).abs().square().clamp_min(FLOOR)
        return (torch.log10(pr) - torch.log10(pe)).square().mean(1).sqrt().mean(-1)

    a_, b_ = fused().clone(), composed()
    res = {"device": torch.cuda.get_device_name(0), "B": B, "L": L, "nfft": NFFT, "hop": HOP, "frames": int(T),
           "calls_per_window": N, "windows": WINDOWS, "max_abs_diff_fused_vs_torch": float((a_ - b_).abs().max())}
    for fn in (fused, composed):
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    tf, tc = [], []
    for _ in range(WINDOWS):
        tf.append(window_us(fused))
        tc.append(window_us(composed))
    res.update(fused_us_median=round(statistics.median(tf), 2), fused_us_min_max=[round(min(tf), 2), round(max(tf), 2)],
               torch_us_median=round(statistics.median(tc), 2), torch_us_min_max=[round(min(tc), 2), round(max(tc), 2)])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
