#!/usr/bin/env python3
"""The band kernels of a design with 8192-point bands (48 kHz, audio_len = 384000: T_oct = 128 .. 8192) under a kernel trace.
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/cqt_long_bands_trace.py run      launches them at B = 1 and B = 32
    python tools/cqt_long_bands_trace.py summary <dir>                                           time per launch and bytes per second
One analysis call (CQT.fwd's: analytic window) and one synthesis call (CQT.bwd's: dual window from the table) are two launches each:
band_fft_kernel over the workgroups of the six short octaves, band_fft13_kernel over the 64 bands of the top octave.
Algorithmic bytes of a launch, per clip: 8 M per band on the spectrum side (the band's window length), 8 T on the coefficient
side, 4 M more where the window comes from the table."""
import collections
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FS, L = 48000, 384000
BATCHES = (1, 32)


def design():
    from babe_amd.cqt import design_bands
    d = design_bands(FS, L)
    return d["M"], d["T"]


def run():
    import torch
    from babe_amd.cqt import CQT_nsgt
    cq = CQT_nsgt(7, 64, "oct", ("kaiser", 1), FS, L, device="cuda")
    assert cq.T_oct[-1] == 8192
    for B in BATCHES:
        spec = cq.fft.rfft(torch.randn(B, L, device="cuda"))
        coefs = cq.alloc_coefs(B)
        for _ in range(30):
            cq.analysis(spec, cq.win_fwd, coefs)
            cq.synthesis_spec(coefs, cq.win_bwd, 2.0 / L)
        torch.cuda.synchronize()


def summary(path):
    M, T = design()
    long_ = T == 8192
    # bytes per clip: (analysis, synthesis) x (short, long)
    by = {("band_fft_kernel<0", False): 8 * (M[~long_].sum() + T[~long_].sum()), ("band_fft13_kernel<0", True): 8 * (M[long_].sum() + T[long_].sum()),
          ("band_fft_kernel<1", False): 8 * T[~long_].sum() + 12 * M[~long_].sum(), ("band_fft13_kernel<1", True): 8 * T[long_].sum() + 12 * M[long_].sum()}
    rows = collections.defaultdict(list)
    for p in glob.glob(path + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(p)):
            for (key, _), b in by.items():
                if key in r["Kernel_Name"]:
                    gx = int(r.get("Grid_Size_X") or r.get("Grid_Size_x") or 1) // int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size_x") or 1)
                    gy = int(r.get("Grid_Size_Y") or r.get("Grid_Size_y") or 1)
                    rows[(key, gy, gx, int(b))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    print(f"# fs = {FS}, audio_len = {L}: {int(long_.sum())} bands of 8192 points (M = {int(M[long_].min())} .. {int(M[long_].max())}), "
          f"{int((~long_).sum())} shorter bands; rocprofv3 --kernel-trace, trimmed mean of the kernels' own durations")
    print("# kernel<MODE> (0 analysis, analytic window; 1 synthesis, window table)   clips  workgroups/clip   launches   us per launch   algorithmic MB   TB/s")
    for (k, gy, gx, b), v in sorted(rows.items(), key=lambda kv: (kv[0][1], kv[0][0][-1], kv[0][0])):
        v = sorted(v)[len(v) // 10: len(v) - len(v) // 10 or None] or v
        us = sum(v) / len(v)
        print(f"{k + '>':24s} {gy:5d} {gx:8d} {len(v):12d} {us:14.2f} {gy * b / 1e6:14.2f} {gy * b / us / 1e6:10.3f}")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "summary":
        summary(sys.argv[2])
    else:
        sys.exit(__doc__)
