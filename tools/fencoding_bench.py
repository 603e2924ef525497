"""Cost of the folded frequency encodings (use_fencoding, csrc/fenc.hip): one full-width score evaluation (UNet forward +
input-VJP, the product of every sampler step) at the benchmark's segment (44.1 kHz, L = 368368, B = 1), encodings off and on, on
the default sequencer.  Per configuration: HIP-event time of `reps` evaluations after warm-up, repeated `blocks` times (median
and min..max over the blocks), and a SHA-256 of the output and the input gradient, so that the `off` result can be compared bit
for bit between two commits.  `--off-only` touches nothing the option added and so runs on a commit without it.
Prints one JSON object."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

L = 368368


def score_eval(fenc, reps, blocks):
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    args = default_args(sample_rate=44100, audio_len=L)
    kw = {}
    if fenc:
        args.network.use_fencoding = True
        kw["use_fencoding"] = True
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(init_state_dict(args.network.Ns, args.network.num_dils, seed=0, gate_scale=1.0, **kw))
    g = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(1, L, generator=g)).cuda()
    w = torch.randn(1, L, generator=g).cuda()
    cn = torch.full((1, 1), -0.4, device="cuda")
    for _ in range(3):
        y = net.fwd_nograd(x, cn)
        gx = net.vjp(w)
    torch.cuda.synchronize()
    digest = hashlib.sha256(y.cpu().numpy().tobytes() + gx.cpu().numpy().tobytes()).hexdigest()[:16]
    ts = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            net.fwd_nograd(x, cn)
            net.vjp(w)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    del net
    torch.cuda.empty_cache()
    return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), sha256_y_gx=digest)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=7)
    a = ap.parse_args()
    res = dict(L=L, B=1, reps=a.reps, blocks=a.blocks, off=score_eval(False, a.reps, a.blocks))
    if not a.off_only:
        res["on"] = score_eval(True, a.reps, a.blocks)
        res["on_minus_off_pct"] = round(100 * (res["on"]["ms_median"] / res["off"]["ms_median"] - 1), 2)
    res["date"] = time.strftime("%Y-%m-%d")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
