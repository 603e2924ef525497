"""What the one-call library path gains under bf16, at the benchmark's shape - full-width network, L = 368368, T = 35, one clip:

    python tools/bf16_library_bench.py [--T 35] [--reps 3] [--out profiles/bf16_library_run.txt]

  load      babe_model_load_ex per precision: wall time, the loader's own split, arena bytes
  run       babe_sample_bwe on the bf16 model against BlindSampler(bf16 network, loop="python") in ONE process, alternated after
            one warm-up run each, both on the library's noise generator under one seed (the results are compared bit for bit);
            a run's time is a host clock around the call, ended by a device synchronise
  enqueue   host time per score evaluation: the library run's is the time babe_sample_bwe takes to RETURN (it enqueues the whole
            run and waits for nothing) over its 2T - 1 evaluations; the Python loop waits inside a run, so its figure is the host
            time to enqueue one UNet forward + input-VJP through the Python sequencer (tools/host_enqueue_time.py's measure),
            next to the same pair through the C sequencer over the same engine
`python bench.py --precision bf16` is the project's own number for the Python bf16 loop.  Needs a MI355X."""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=35)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    from babe_amd import model_file
    from babe_amd._cabi import SampleDesc
    from babe_amd._lib import check, lib, ptr, stream
    from babe_amd.config import default_args
    from babe_amd.diff_params.edm import EDM
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    from babe_amd.networks.unet_c import CUnet
    from babe_amd.testing import sample_c
    from babe_amd.testing.blind_bwe_sampler import BlindSampler
    from babe_amd.testing.model_c import LibraryModel
    os.environ.setdefault("BABE_CQT_C", "1")            # the Python loop on the library's CQT plan: the same tables on both sides
    args = default_args(T=a.T)
    Lseg, fs, T = args.exp.audio_len, args.exp.sample_rate, a.T
    sd = init_state_dict(list(args.network.Ns), args.network.num_dils, seed=0, gate_scale=1.0)
    lines = [f"device: {torch.cuda.get_device_name(0)}; Ns={list(args.network.Ns)} L={Lseg} fs={fs} T={T} B=1; one process"]
    torch.zeros(1, device="cuda")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "model.babe")
        model_file.export(sd, args, path)
        LibraryModel(path, "f32").close()                # (the page cache, the runtime and the pack kernels' code objects warm)
        for prec in ("f32", "bf16", "bf16x3"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = LibraryModel(path, prec)
            wall = time.perf_counter() - t0
            info = m.info
            lines.append(f"babe_model_load_ex {prec:6s}: {1e3 * wall:7.1f} ms (read+parse {info.load_ms[0]:.1f} | stage+upload "
                         f"{info.load_ms[1]:.1f} | pack+CQT plan+wait {info.load_ms[2]:.1f}); arena {info.device_bytes / 2**20:.1f} MiB, "
                         f"CQT tables {info.cqt_device_bytes / 2**20:.1f} MiB")
            m.close()
        model = LibraryModel(path, "bf16")

        net = Unet_CQT_oct_with_attention(args, "cuda", precision="bf16")
        net.load_state_dict(sd)
        g = torch.Generator().manual_seed(5)
        y = (0.1 * torch.randn(1, Lseg, generator=g)).cuda()
        smp = BlindSampler(net, EDM(args), args, loop="python", noise_device="philox", seed=a.seed)
        rows, t0_, _ = sample_c.steps_from(smp.diff_params, T, smp.order, smp.start_sigma, 1.0)
        state = lib().babe_unet_state_create()
        d = SampleDesc()
        d.eval = model.eval_desc(state)
        params0 = smp._init_params(1, y.device)
        d.eval.K, d.eval.blind = int(params0.shape[-1]), 1
        d.T, d.steps, d.t0, d.warm_start = T, rows, t0_, int(smp.start_sigma is not None)
        need = lib().babe_sample_workspace_bytes(C.byref(d), 1)
        assert need > 0, lib().babe_last_error()
        ws = torch.empty(need, device="cuda", dtype=torch.uint8)

        def run_library():
            p, x = params0.clone().contiguous(), torch.empty_like(y)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            check(lib().babe_sample_bwe(C.byref(d), ptr(y), ptr(p), ptr(x), None, a.seed, 0, None, None, ptr(ws), need, 1, stream()), "sample_bwe")
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, t1 - t0, x, p

        def run_python():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x, p = smp.predict_blind_bwe(y)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, None, x, p

        runs = {"library": run_library, "python": run_python}
        out = {k: f()[2:] for k, f in runs.items()}                               # warm-up
        same = torch.equal(out["python"][0], out["library"][0]) and torch.equal(out["python"][1].reshape(-1), out["library"][1].reshape(-1))
        times, enq = {k: [] for k in runs}, []
        for _ in range(a.reps):
            for k, f in runs.items():
                t, e = f()[:2]
                times[k].append(t)
                if e is not None:
                    enq.append(e)
        audio = Lseg / fs
        for k in runs:
            t = times[k]
            name = "babe_sample_bwe, bf16 model" if k == "library" else "Python bf16 loop       "
            lines.append(f"{name}: median {statistics.median(t):7.3f} s (min {min(t):.3f}, max {max(t):.3f}, {len(t)} runs) = "
                         f"{audio / statistics.median(t):.3f} audio-sec/s")
        lines.append(f"    results bit-equal between the two: {same}")
        nev = 2 * T - 1
        lines.append(f"babe_sample_bwe returns after {1e3 * statistics.median(enq):.1f} ms = {1e3 * statistics.median(enq) / nev:.2f} ms of host time per "
                     f"evaluation ({nev} evaluations: CQT, UNet forward + VJP, STFT guidance, filter fit)")
        lib().babe_unet_state_destroy(state)

        # one UNet forward + input-VJP: host time to enqueue it, and wall time with the drain
        eng = net.engine()
        x = torch.randn(1, Lseg, device="cuda")
        co = [c.contiguous() for c in net.CQTransform.fwd_planar(x)]
        film = eng.embed(torch.full((1, 1), 0.3, device="cuda"))
        gouts = [torch.randn_like(c) for c in co]
        cu = CUnet(eng)
        for name, f in (("Python sequencer", lambda: (eng.forward(co, film), eng.vjp(gouts))), ("C sequencer     ", lambda: (cu.fwd(co, film), cu.vjp(gouts)))):
            for _ in range(2):
                f()
            torch.cuda.synchronize()
            n = 5
            t0 = time.perf_counter()
            for _ in range(n):
                f()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            lines.append(f"UNet forward + VJP, bf16 engine, {name}: host enqueue {1e3 * (t1 - t0) / n:6.2f} ms, wall with the drain "
                         f"{1e3 * (t2 - t0) / n:6.2f} ms per evaluation")
        model.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
