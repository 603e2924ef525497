"""Load time of a network from a model file, library against Python, on one GPU:

    python tools/model_load_bench.py [--out profiles/model_load.json] [--precision f32|bf16|bf16x3]
                                     [--sample-rate 44100 --audio-len 368368] [key.sub=value ...]

Exports the configured network (random weights: the timings do not depend on the values) to a temporary model file, then records
  library   babe_model_load_ex at --precision: wall time, its own split (read + parse + validate | staging + upload | pack + CQT plan + the wait),
            device bytes held (arena, CQT tables)
  python    constructing Unet_CQT_oct_with_attention (same precision) + load_state_dict(model_file.read) + the first c_plan(), synchronised:
            wall time, device bytes torch holds afterwards
in one process, the library first (its file read warms the page cache for the Python side; the read time is listed on its own),
and writes one JSON document."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "model_load.json"))
    ap.add_argument("--sample-rate", type=int, default=44100)
    ap.add_argument("--audio-len", type=int, default=368368)
    ap.add_argument("--precision", default="f32", choices=("f32", "bf16", "bf16x3"))
    ap.add_argument("overrides", nargs="*")
    a = ap.parse_args()
    import torch
    from babe_amd import model_file
    from babe_amd.config import apply_overrides, default_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, init_state_dict
    from babe_amd.testing.model_c import LibraryModel
    args = apply_overrides(default_args(sample_rate=a.sample_rate, audio_len=a.audio_len), a.overrides)
    nw = args.network
    res = dict(config=dict(sample_rate=a.sample_rate, audio_len=a.audio_len, precision=a.precision, Ns=list(nw.Ns), num_dils=list(nw.num_dils)),
               device=torch.cuda.get_device_name())
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "model.babe")
        t = time.perf_counter()
        res["file_bytes"] = model_file.export(init_state_dict(list(nw.Ns), list(nw.num_dils), nw.emb_dim), args, path)
        res["export_s"] = time.perf_counter() - t
        torch.cuda.init()
        torch.zeros(1, device="cuda")
        torch.cuda.synchronize()
        t = time.perf_counter()
        m = LibraryModel(path, a.precision)
        wall = time.perf_counter() - t
        info = m.info
        res["library"] = dict(wall_s=wall, read_s=info.load_ms[0] / 1e3, upload_s=info.load_ms[1] / 1e3, pack_s=info.load_ms[2] / 1e3,
                              device_bytes=info.device_bytes, cqt_device_bytes=info.cqt_device_bytes, params=info.params)
        m.close()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        t = time.perf_counter()
        net = Unet_CQT_oct_with_attention(args, "cuda", precision=a.precision)
        t1 = time.perf_counter()
        net.load_state_dict(model_file.read(path)[1])
        t2 = time.perf_counter()
        net.engine().c_plan()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        res["python"] = dict(wall_s=t3 - t, construct_s=t1 - t, read_and_load_state_dict_s=t2 - t1, engine_and_plan_s=t3 - t2,
                             device_bytes=torch.cuda.memory_allocated() - base)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
