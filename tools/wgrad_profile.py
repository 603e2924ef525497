"""Driver for profiling the conv weight-gradient kernel (csrc/wgrad.hip) under rocprofv3: the (5,3) main-block layer shapes of
levels 3-6 at the reference training geometry (B = 4, L = 368368), REPS calls each.  See profiles/wgrad_profile.txt.
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/wgrad_profile.py
    rocprofv3 --kernel-trace --pmc <counters> -d OUT -- python tools/wgrad_profile.py      (one counter group per run)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, REPS = 4, 3
LEVELS = [(3, 128, 256, 512), (4, 128, 320, 256), (5, 256, 384, 128), (6, 256, 448, 64)]    # (level, C, F, T)


def main():
    from babe_amd import ops
    for lv, C, F, T in LEVELS:
        x = torch.randn(B, C, F, T, device="cuda")
        g = torch.randn(B, C, F, T, device="cuda")
        rows = torch.empty(B, C * C * 15, device="cuda")
        ws = torch.empty(ops.conv_wgrad_workspace(x, g, 5, 3, 2), device="cuda")
        for _ in range(REPS):
            ops.conv_wgrad_rows(x, g, 5, 3, rows, dil=2, ws=ws)
        torch.cuda.synchronize()
        print(f"level {lv}: C={C} F={F} T={T} grid={(C // 64) * (C // 32)} tiles", flush=True)


if __name__ == "__main__":
    main()
