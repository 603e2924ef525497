"""Write the denoiser weights file a host without Python loads (babe_amd/model_file.py::export_denoiser, babe_denoiser_load):

    python -m babe_amd.export_denoiser --out denoiser.babe [--ckpt weights.pt] [key=value ...]

--ckpt: a reference denoiser checkpoint (a state_dict, or a mapping holding one under "state_dict" / "model"); without it the
network has the synthetic weights of networks.denoiser.init_state_dict (useful only to exercise the path).  key=value: leaves of
the configuration's tester.denoiser node; the defaults are the shipped network's (conf/tester/blind_bwe_denoise*.yaml).  Needs
no GPU."""
import argparse
import ast
import sys

DEFAULTS = dict(depth=6, num_tfc=3, num_stages=2, use_SAM=True, use_fencoding=True, f_dim=513, sample_rate_denoiser=22050,
                segment_size=5, stft_win_size=1024, stft_hop_size=256)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--ckpt")
    ap.add_argument("overrides", nargs="*", help="key=value")
    a = ap.parse_args(argv)
    import torch
    from . import model_file
    from .networks.denoiser import init_state_dict
    dargs = dict(DEFAULTS)
    for ov in a.overrides:
        k, _, v = ov.partition("=")
        try:
            dargs[k] = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            dargs[k] = v
    cfg = {k: dargs[k] for k in ("depth", "num_tfc", "num_stages", "use_SAM", "use_fencoding", "f_dim")}
    sd = init_state_dict(cfg)
    if a.ckpt:
        state = torch.load(a.ckpt, map_location="cpu", weights_only=False)
        for key in ("state_dict", "model"):
            if isinstance(state, dict) and key in state and isinstance(state[key], dict):
                state = state[key]
        bad = [k for k in sd if k not in state or tuple(state[k].shape) != tuple(sd[k].shape)]
        if bad:
            sys.exit(f"{a.ckpt}: does not fit the configured denoiser ({len(bad)} keys, first: {bad[0]})")
        sd = {k: state[k] for k in sd}
    n = model_file.export_denoiser(sd, dargs, a.out)
    print(f"{a.out}: {n} bytes, {len(sd)} tensors, {sum(v.numel() for v in sd.values())} parameters")


if __name__ == "__main__":
    main()
