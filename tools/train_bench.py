"""One training step of the full-width CQTDiff+ prior at the reference geometry (B=4, L=368368, 44.1 kHz), split into forward,
input-VJP, parameter-gradient work (and the conv weight-gradient calls in it), reductions and repack, plus the conv weight-gradient kernel's rate per level against the matching peak: 157.3
TFLOP/s measured fp32 MFMA peak for --wgrad f32, the 2.5 PFLOP/s dense bf16 SPEC figure for --wgrad bf16.  Prints one JSON
document (profiles/train_bench.json, profiles/train_bench_wgrad_bf16.json).

    python tools/train_bench.py [--B 4] [--L 368368] [--reps 3] [--attention-layers 0,0,0,0,1,1,1,1]
                                [--wgrad {f32,bf16}] [--precision {f32,bf16}] [--attention-precision {f32,bf16}]

--wgrad: arithmetic of the conv weight gradients (set_trainable(True, wgrad=...)); --precision: the network's conv arithmetic
(forward and input-VJP); --precision bf16 --wgrad bf16 is the full mixed-precision step.

--attention-layers: train a network with time-attention layers (set_trainable(True, attention=True)); the report then also has the
qk weight-gradient launches of one backward (babe_attn_qk_wgrad, one per attention block after the lane join): their summed time
and share of the step.

--attention-precision: arithmetic of the attention core (the network's attention_precision).  bf16 trains on the bf16 core
(set_trainable(True, attention='bf16')); with --wgrad bf16 the qk weight gradients then run on babe_attn_qk_wgrad_bf16.  The
report's attn_qk_wgrad_kernel names the entry point that ran.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK = {"f32": (157.3e12, "fp32 MFMA peak, measured"), "bf16": (2.5e15, "dense bf16 MFMA, spec")}


def timed(fn, reps):
    """median ms of fn() over reps runs (HIP events on the current stream, synchronised)."""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--L", type=int, default=368368)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--attention-layers", default=None, help="8 comma-separated flags, e.g. 0,0,0,0,1,1,1,1")
    ap.add_argument("--wgrad", choices=["f32", "bf16"], default="f32", help="conv weight-gradient arithmetic")
    ap.add_argument("--precision", choices=["f32", "bf16"], default="f32", help="the network's conv arithmetic")
    ap.add_argument("--attention-precision", choices=["f32", "bf16"], default=None,
                    help="arithmetic of the attention core (needed for attention layers in a --precision bf16 network)")
    a = ap.parse_args()
    att = [int(v) for v in a.attention_layers.split(",")] if a.attention_layers else None
    from babe_amd import ops
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    from tests.golden_weights import FULL_DILS, FULL_NS

    args = default_args(sample_rate=44100, audio_len=a.L)
    adict = None
    if att:
        adict = dict(num_heads=8, attn_dropout=0.0, bias_qkv=False, N=0, rel_pos_num_buckets=32, rel_pos_max_distance=64,
                     use_rel_pos=True, Nproj=8)
        args.network.attention_layers, args.network.attention_dict = att, adict
    net = Unet_CQT_oct_with_attention(args, "cuda", precision=a.precision, attention_precision=a.attention_precision)
    net.load_state_dict(init_state_dict(FULL_NS, FULL_DILS, seed=0, attention_layers=att, attention_dict=adict))
    net.set_trainable(True, attention="bf16" if net.bf16_attention else bool(att), wgrad=a.wgrad)
    gen = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(a.B, a.L, generator=gen)).cuda()
    cn = torch.linspace(-1, 0.5, a.B).reshape(a.B, 1).cuda()
    w = torch.randn(a.B, a.L, generator=gen).cuda()
    res = {"B": a.B, "L": a.L, "lanes": min(a.B, net.MAX_LANES) if net.concurrent_lanes_ok else 1, "attention_layers": att,
           "precision": a.precision, "wgrad": a.wgrad, "attention_precision": a.attention_precision}

    # input-VJP alone (the sampler's path) and the forward without training state
    def fwd_vjp():
        net.fwd_nograd(x, cn)
        net.vjp(w)
    t_fwd_vjp = timed(fwd_vjp, a.reps)
    res["forward_ms"] = timed(lambda: net.fwd_nograd(x, cn, train=True), a.reps)
    res["input_vjp_ms"] = t_fwd_vjp - timed(lambda: net.fwd_nograd(x, cn), a.reps)

    # the parameter-gradient backward: input-VJP + parameter-gradient work + reductions (param_grads timed on its own); the conv
    # weight-gradient calls themselves (babe_conv_wgrad_rows, partial + chunk-sum kernels) timed per call on their lane's stream
    from babe_amd.networks import unet_engine as ue
    wg_ev = []
    orig_wg = ue.UnetEngine._wg

    def wg(self, *args, **kw):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        orig_wg(self, *args, **kw)
        e.record()
        wg_ev.append((s, e))
    ue.UnetEngine._wg = wg
    qk_ev, qk_kernels = [], set()
    orig_qk = ops.attn_qk_wgrad

    def qk_wgrad(*args, **kw):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = orig_qk(*args, **kw)
        e.record()
        qk_ev.append((s, e))
        qk_kernels.add("babe_attn_qk_wgrad" + ("_bf16" if kw.get("precision", "f32") == "bf16" else ""))
        return out
    ops.attn_qk_wgrad = qk_wgrad
    eng = net.engine()
    red = []
    orig = eng.param_grads

    def param_grads(pg, keep):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = orig(pg, keep)
        e.record()
        red.append((s, e))
        return out
    eng.param_grads = param_grads
    bwd = []
    for _ in range(a.reps):
        net.fwd_nograd(x, cn, train=True)
        bwd.append(timed(lambda: net._vjp_train(w), 1))
    torch.cuda.synchronize()
    eng.param_grads = orig
    ue.UnetEngine._wg = orig_wg
    ops.attn_qk_wgrad = orig_qk
    res["train_backward_ms"] = sorted(bwd)[len(bwd) // 2]
    res["reductions_ms"] = sorted(s.elapsed_time(e) for s, e in red)[len(red) // 2]
    # everything the parameter gradients add to the backward: conv weight gradients, the recomputed GELU, the GroupNorm / FiLM
    # reductions, the zero-fill of the gradient buffers (the FiLM / MLP backward is in reductions_ms)
    res["param_grad_work_ms"] = res["train_backward_ms"] - res["input_vjp_ms"] - res["reductions_ms"]
    # sum over the conv weight-gradient calls of one backward (calls of the two lanes overlap in time, so this sum can exceed
    # their share of the wall time)
    res["wgrad_calls_per_backward"] = len(wg_ev) // a.reps
    res["wgrad_calls_ms_sum"] = sum(s.elapsed_time(e) for s, e in wg_ev) / a.reps
    sd = net._engine_sd()
    res["repack_ms"] = timed(lambda: eng.refresh(sd), a.reps)

    # full step through autograd + Adam (loss = <net(x), w>)
    opt = torch.optim.Adam(net.parameters(), lr=1e-6)

    def step():
        opt.zero_grad()
        y = net(x, cn)
        (y * w).sum().backward()
        opt.step()
    step()
    res["step_ms"] = timed(step, a.reps)
    if att:                                            # the launches run back to back on one stream: their times add up
        res["attn_qk_wgrad_kernel"] = "+".join(sorted(qk_kernels))
        res["attn_qk_wgrad_calls_per_backward"] = len(qk_ev) // a.reps
        res["attn_qk_wgrad_ms_sum"] = sum(s.elapsed_time(e) for s, e in qk_ev) / a.reps
        res["attn_qk_wgrad_share_of_step"] = round(res["attn_qk_wgrad_ms_sum"] / res["step_ms"], 4)

    # weight-gradient kernel per level: the (5,3) H convs of the main blocks at this geometry, B rows per call
    Ts = [c.shape[-1] for c in net.CQTransform.fwd_planar(x[:1])][::-1]
    lv = []
    for i, N in enumerate(FULL_NS):
        F, T = 64 * (i + 1), Ts[i]
        xa = torch.randn(a.B, N, F, T, device="cuda")
        g = torch.randn(a.B, N, F, T, device="cuda")
        rows = torch.empty(a.B, N * N * 15, device="cuda")
        ws = torch.empty(ops.conv_wgrad_workspace(xa, g, 5, 3, 1, precision=a.wgrad), device="cuda")
        ms = timed(lambda: ops.conv_wgrad_rows(xa, g, 5, 3, rows, dil=2, ws=ws, precision=a.wgrad), a.reps + 2)
        fl = 2.0 * a.B * N * N * 15 * F * T
        lv.append({"level": i, "C": N, "F": F, "T": T, "ms": round(ms, 4), "tflops": round(fl / ms / 1e9, 2),
                   "frac_peak": round(fl / ms / 1e9 / (PEAK[a.wgrad][0] / 1e12), 3)})
        del xa, g, rows, ws
    res["wgrad_levels"] = lv
    res["wgrad_levels_peak_tflops"], res["wgrad_levels_peak_is"] = PEAK[a.wgrad][0] / 1e12, PEAK[a.wgrad][1]
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
