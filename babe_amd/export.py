"""Write the model file a host without Python loads (babe_amd/model_file.py, babe_model_load):

    python -m babe_amd.export --out model.babe [--ckpt weights.pt] [--sample-rate 44100] [--audio-len 368368] [--T 35]
                              [key.sub=value ...]

--ckpt: a reference checkpoint (its EMA weights, as `restore` loads them); without it the network has the random weights a
freshly constructed one has, as `restore` without --ckpt (useful only to exercise the path).  key.sub=value: overrides of the
configuration (config.apply_overrides), e.g. network.Ns=[8,8,8,8,16,16,16] tester.posterior_sampling.xi=0.3.  Needs no GPU."""
import argparse
import sys


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--ckpt")
    ap.add_argument("--T", type=int, default=35)
    ap.add_argument("--sample-rate", type=int, default=44100)
    ap.add_argument("--audio-len", type=int, default=368368)
    ap.add_argument("overrides", nargs="*", help="key.sub=value")
    a = ap.parse_args(argv)
    import torch
    from . import model_file
    from .config import apply_overrides, default_args
    from .io import ema_state_dict
    from .networks.cqtdiff_plus import init_state_dict
    args = apply_overrides(default_args(sample_rate=a.sample_rate, audio_len=a.audio_len, T=a.T), a.overrides)
    nw = args.network
    layers = nw.attention_layers if any(nw.attention_layers or []) else None
    sd = init_state_dict(list(nw.Ns), list(nw.num_dils), nw.emb_dim, attention_layers=layers,
                         attention_dict=nw.attention_dict if layers else None, use_fencoding=bool(nw.use_fencoding))
    if a.ckpt:
        state = torch.load(a.ckpt, map_location="cpu", weights_only=False)
        loaded = ema_state_dict(state, set(sd))
        bad = [k for k in sd if k not in loaded or tuple(loaded[k].shape) != tuple(sd[k].shape)]
        if bad:
            sys.exit(f"{a.ckpt}: does not fit the configured network ({len(bad)} keys, first: {bad[0]})")
        sd = {k: loaded[k] for k in sd}
    n = model_file.export(sd, args, a.out)
    print(f"{a.out}: {n} bytes, {len(sd)} tensors, {sum(v.numel() for v in sd.values())} parameters")


if __name__ == "__main__":
    main()
