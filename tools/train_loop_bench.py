"""What training.Trainer.training_loop adds to the bare optimizer step at the reference geometry (full width, B = 4,
L = 368368, 44.1 kHz): mean iteration time over `--its` iterations after `--warmup` ones, split into get_batch (file reads, the
host-to-device copy, resampling), the step itself, update_ema and the log line, with a synchronisation around every phase so that
the parts add up.  Compare with `step_ms` of tools/train_bench.py run next to it with the same --precision / --wgrad.  Prints one
JSON document (profiles/train_loop.json).

    python tools/train_loop_bench.py [--B 4] [--L 368368] [--its 20] [--warmup 3] [--wgrad {f32,bf16}] [--precision {f32,bf16}]
                                     [--num-workers 0] [--fused-tail | --torch-fused]

--fused-tail: optim.FusedAdamEMA (norm, clipping, Adam and the EMA in the library's kernels; update_ema_ms is then 0 and the
tail's time is part of train_step_ms).  --torch-fused: torch.optim.Adam(fused=True) with clip_grad_norm_ and update_ema as they are.
Compare train_step_ms + update_ema_ms between runs; tail_kernel_ms (--fused-tail) is the HIP-event time of the tail's launches
alone, with the fraction of the 6.29 TB/s copy rate its 40 bytes per parameter come to.

The data are four one-minute 16-bit stereo wavs written to a temporary directory and read through AudioFolderDataset.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--L", type=int, default=368368)
    ap.add_argument("--its", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--wgrad", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--precision", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--num-workers", type=int, default=0)
    ap.add_argument("--fused-tail", action="store_true")
    ap.add_argument("--torch-fused", action="store_true")
    a = ap.parse_args()
    from scipy.io import wavfile
    from babe_amd.config import default_train_args
    from babe_amd.datasets import AudioFolderDataset
    from babe_amd.diff_params.edm import EDM
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    from babe_amd.training import Trainer
    from tests.golden_weights import FULL_DILS, FULL_NS

    root = tempfile.mkdtemp(prefix="train_loop_bench_")
    try:
        rng = np.random.RandomState(0)
        for i in range(4):
            wavfile.write(os.path.join(root, f"f{i}.wav"), 44100, (rng.randn(44100 * 60, 2) * 3000).astype(np.int16))
        args = default_train_args(sample_rate=44100, audio_len=a.L)
        args.exp.update(batch=a.B, num_workers=a.num_workers, model_dir=root, exp_name="bench")
        args.dset.update(name="audiofolder", callable="datasets.audiofolder.AudioFolderDataset", path=root)
        args.logging.update(log_interval=1, save_model=False)
        torch.manual_seed(0)
        ds = AudioFolderDataset(args.dset, fs=44100, seg_len=a.L, seed=42)
        loader = torch.utils.data.DataLoader(ds, batch_size=a.B, num_workers=a.num_workers)
        net = Unet_CQT_oct_with_attention(args, "cuda", precision=a.precision)
        net.load_state_dict(init_state_dict(FULL_NS, FULL_DILS, seed=0))
        net.set_trainable(True, wgrad=a.wgrad)
        if a.fused_tail:
            from babe_amd.optim import FusedAdamEMA
            opt = FusedAdamEMA(net.parameters(), lr=args.exp.lr)
        else:
            opt = torch.optim.Adam(net.parameters(), lr=args.exp.lr, **({"fused": True} if a.torch_fused else {}))
        tr = Trainer(args, loader, net, opt, EDM(args), device="cuda")
        tr.sync_timers = True
        tr.training_loop(total_its=a.warmup)
        for k in tr.timers:
            tr.timers[k] = 0.0 if k != "its" else 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.training_loop(total_its=a.warmup + a.its)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        n = tr.timers["its"]
        res = {"B": a.B, "L": a.L, "precision": a.precision, "wgrad": a.wgrad, "num_workers": a.num_workers, "iterations": n,
               "tail": "fused" if a.fused_tail else "torch-fused-adam" if a.torch_fused else "torch", "iteration_ms": round(1e3 * wall / n, 2)}
        for k in ("get_batch", "train_step", "update_ema", "log"):
            res[k + "_ms"] = round(1e3 * tr.timers[k] / n, 2)
        # one log line WITH the band energies (every logging.freq_cqt_logging-th iteration; none falls into the timed ones)
        x = torch.randn(a.B, a.L, device="cuda")
        net.CQTransform.band_energy(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        net.CQTransform.band_energy(x).mean(0).cpu()
        res["band_energy_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
        if a.fused_tail:
            # the tail's launches alone (the table's 29 KB copy included), between HIP events: the gradients of the last iteration
            # are still there; a matrix product in front keeps the GPU busy until step() has queued everything
            ex = args.exp
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            big = torch.randn(8192, 8192, device="cuda")
            ms = []
            for _ in range(5):
                big @ big
                ev[0].record()
                opt.step(max_grad_norm=ex.max_grad_norm, ema_s=ex.ema_rate)
                ev[1].record()
                torch.cuda.synchronize()
                ms.append(ev[0].elapsed_time(ev[1]))
            nparam = sum(p.numel() for p in net.parameters())
            res["tail_kernel_ms"] = round(min(ms), 4)
            res["tail_bytes"] = 40 * nparam
            res["tail_fraction_of_6.29TBps"] = round(40 * nparam / (min(ms) * 1e-3) / 6.29e12, 3)
        print(json.dumps(res, indent=1))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
