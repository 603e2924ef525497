"""Time-attention measurements (csrc/attention.hip) at the benchmark's segment (44.1 kHz, L = 368368).

1. Kernel time of babe_attn_fwd and babe_attn_vjp from HIP events after warm-up, at each level's (F, T) (F = 64 (i+1),
   T = 4096 >> i, H = 8), B = 1 and 2, with the algorithmic FLOP counted from the shapes and the share of the fp32 MFMA peak
   (157.3 TFLOP/s).  Forward: QK^T + PV = 4 B H F T^2.  VJP: the kernels recompute S twice (query and key side), so the
   algorithmic count is the textbook 2.5x the forward (S, dP, dQ, dK, dV = 10 B H F T^2).
2. One score evaluation (UNet forward + input-VJP, the product of the blind sampler's every step) of the full-width network
   with attention_layers [0,0,0,0,1,1,1,1] against the same network with attention off, B = 1, both on the Python sequencer
   (BABE_EVAL_C=0, BABE_UNET_C=0).
--attention-precision f32|bf16 (default: none of the below, the fp32 measurement as it always was):
1. times babe_attn_fwd_bf16 / babe_attn_vjp_bf16 (csrc/attention_bf16.hip) under 'bf16' - the VJP there recomputes S three times,
   the algorithmic count stays the textbook one; the peak share is then of the bf16 MFMA peak (16 x the fp32 one);
2. times the full-width precision='bf16' network with [0,0,0,0,1,1,1,1] and the attention core in the named arithmetic against
   the attention-free precision='bf16' network.
Prints one JSON object."""
import argparse
import json
import os
import sys
import time

os.environ["BABE_EVAL_C"] = "0"
os.environ["BABE_UNET_C"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from babe_amd import ops  # noqa: E402

PEAK = {"f32": 157.3e12, "bf16": 16 * 157.3e12}
H = 8


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def kernels(prec="f32"):
    rows = []
    for lvl in range(8):
        i = min(lvl, 6)
        F, T = 64 * (i + 1), 4096 >> i
        for B in (1, 2):
            g = torch.Generator(device="cuda").manual_seed(lvl)
            qk = torch.randn(B, 2 * H * F, T, device="cuda", generator=g) / F ** 0.25
            a = torch.randn(B, H, F, T, device="cuda", generator=g)
            dout = torch.randn(B, H, F, T, device="cuda", generator=g)
            bucket = ops.attn_buckets(T).cuda()
            emb = torch.randn(32, H, device="cuda", generator=g)
            out, lse = torch.empty_like(a), torch.empty(B, H, T, device="cuda")
            dqk, dv = torch.empty_like(qk), torch.empty_like(a)
            s = F ** -0.5
            tf = timed(lambda: ops.attn_fwd(qk, a, out, lse, s, bucket=bucket, emb=emb, precision=prec))
            tb = timed(lambda: ops.attn_vjp(qk, a, out, lse, dout, dqk, dv, s, bucket=bucket, emb=emb, precision=prec))
            ff, fb = 4.0 * B * H * F * T * T, 10.0 * B * H * F * T * T
            rows.append(dict(level="mid" if lvl == 7 else lvl, F=F, T=T, B=B, fwd_us=round(tf * 1e6, 1), vjp_us=round(tb * 1e6, 1),
                             fwd_gflop=round(ff / 1e9, 3), vjp_gflop=round(fb / 1e9, 3),
                             fwd_peak_share=round(ff / tf / PEAK[prec], 4), vjp_peak_share=round(fb / tb / PEAK[prec], 4)))
            print(rows[-1], file=sys.stderr, flush=True)
    return rows


def score_eval(layers, reps=5, precision="f32", attention_precision=None):
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    from tests.attention_weights import attention_dict
    L = 368368
    args = default_args(sample_rate=44100, audio_len=L)
    args.network.attention_layers = list(layers)
    args.network.attention_dict = attention_dict()
    net = Unet_CQT_oct_with_attention(args, "cuda", precision=precision, attention_precision=attention_precision)
    net.load_state_dict(init_state_dict(args.network.Ns, args.network.num_dils, seed=0, gate_scale=1.0, attention_layers=layers,
                                        attention_dict=args.network.attention_dict))
    g = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(1, L, generator=g)).cuda()
    w = torch.randn(1, L, generator=g).cuda()
    cn = torch.full((1, 1), -0.4, device="cuda")

    def step():
        net.fwd_nograd(x, cn)
        net.vjp(w)
    t = timed(step, warm=2, reps=reps)
    del net
    torch.cuda.empty_cache()
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--attention-precision", choices=["f32", "bf16"], default=None)
    a = ap.parse_args()
    core = a.attention_precision
    res = dict(kernels=kernels(core or "f32"))
    net_prec = "f32" if core is None else "bf16"
    t_off = score_eval([0] * 8, precision=net_prec)
    t_on = score_eval([0, 0, 0, 0, 1, 1, 1, 1], precision=net_prec, attention_precision=core)
    res["score_eval_s"] = dict(attention_off=round(t_off, 5), attention_last_two=round(t_on, 5),
                               added_pct=round(100 * (t_on / t_off - 1), 2))
    res["network_precision"], res["attention_precision"] = net_prec, core or "f32"
    res["date"] = time.strftime("%Y-%m-%d")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
