"""The denoiser pre-pass from the library against the Python path, on one GPU:

    python tools/denoiser_library_bench.py [--out result.json] [--seconds 30] [--rounds 5]

The shipped configuration (depth 6, 3 dense layers, 2 stages, SAM, frequency encoding: 72.59 M parameters, synthetic weights - the
timings do not depend on the values) on `--seconds` of audio at 22.05 kHz, 5 s segments: the workload of
profiles/r01_denoiser_layers.txt.  Records
  apply_denoiser   DenoiserPrepass.apply_denoiser (Python sequencer) and babe_denoise_signal (library sequencer), ALTERNATING
                   round by round in one process: wall time of a synchronised call, and host enqueue time (the call's return,
                   before the wait) - the kernels are the same, the sequencer is what differs;
  load             babe_denoiser_load of the exported file (wall, and its own split) next to Python's
                   MultiStage_denoise + load_state_dict(model_file.read) + engine build, synchronised;
  equal            whether the two results agree in every bit.
Prints a summary (profiles/denoiser_library.txt keeps one) and, with --out, writes every figure as one JSON document."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from babe_amd import model_file
    from babe_amd.networks.denoiser import MultiStage_denoise, init_state_dict
    from babe_amd.testing.denoise import DenoiserPrepass
    from babe_amd.testing.denoiser_c import LibraryDenoiser
    cfg = dict(depth=6, num_tfc=3, num_stages=2, use_SAM=True, use_fencoding=True, f_dim=513)
    dargs = dict(cfg, sample_rate_denoiser=22050, segment_size=5, stft_win_size=1024, stft_hop_size=256)
    res = dict(device=torch.cuda.get_device_name(), seconds=a.seconds, rounds=a.rounds)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "denoiser.babe")
        sd = init_state_dict(cfg, seed=0)
        res["file_bytes"] = model_file.export_denoiser(sd, dargs, path)
        torch.zeros(1, device="cuda")
        torch.cuda.synchronize()
        t = time.perf_counter()
        lib_dn = LibraryDenoiser(path)
        wall = time.perf_counter() - t
        info = lib_dn.info
        res["load_library"] = dict(wall_s=wall, read_s=info.load_ms[0] / 1e3, upload_s=info.load_ms[1] / 1e3, pack_s=info.load_ms[2] / 1e3,
                                   device_bytes=info.device_bytes, params=info.params)
        t = time.perf_counter()
        net = MultiStage_denoise(cfg)
        net.load_state_dict(model_file.read(path)[1])
        net.to("cuda")
        net.engine()
        torch.cuda.synchronize()
        res["load_python"] = dict(wall_s=time.perf_counter() - t)
    pp = DenoiserPrepass(net, dargs, "cuda")
    x = 0.1 * torch.randn(1, int(22050 * a.seconds), device="cuda")
    paths = {"python": pp.apply_denoiser, "library": lib_dn.apply_denoiser}
    last = {}
    for fn in paths.values():                       # warm-up: buffers, workspaces, code objects
        fn(x)
    torch.cuda.synchronize()
    times = {k: dict(wall_ms=[], enqueue_ms=[]) for k in paths}
    for _ in range(a.rounds):
        for name, fn in paths.items():
            t0 = time.perf_counter()
            last[name] = fn(x)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            times[name]["wall_ms"].append((t2 - t0) * 1e3)
            times[name]["enqueue_ms"].append((t1 - t0) * 1e3)
    res["apply_denoiser"] = times
    res["equal"] = bool(torch.equal(last["python"], last["library"]))
    lib_dn.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    med = lambda v: sorted(v)[len(v) // 2]
    for name in paths:
        print(f"apply_denoiser {a.seconds:g} s @ 22.05 kHz, {name:8s}: wall {med(times[name]['wall_ms']):8.2f} ms  "
              f"host enqueue {med(times[name]['enqueue_ms']):8.2f} ms  (median of {a.rounds}; all wall: "
              + " ".join(f"{v:.2f}" for v in times[name]["wall_ms"]) + ")")
    print(f"bit-identical: {res['equal']}")
    ll = res["load_library"]
    print(f"load, library: {ll['wall_s'] * 1e3:.1f} ms (read+parse {ll['read_s'] * 1e3:.1f}, staging+upload {ll['upload_s'] * 1e3:.1f}, "
          f"pack+wait {ll['pack_s'] * 1e3:.1f}), {ll['device_bytes'] / 2 ** 20:.1f} MiB on the device, {ll['params']} parameters")
    print(f"load, python : {res['load_python']['wall_s'] * 1e3:.1f} ms (MultiStage_denoise + load_state_dict + engine build)")


if __name__ == "__main__":
    main()
