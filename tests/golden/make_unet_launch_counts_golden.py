"""Record the launch table of the CQTDiff+ UNet's Python sequencer: the library's always-on launches-per-slot counters
(_lib.dispatch_counts) after one forward plus VJP, for four configurations of the reduced network.

    python tests/golden/make_unet_launch_counts_golden.py [OUT]      # writes tests/golden/unet_launch_counts.json (needs a GPU)

The counters count launches as they are issued, whatever the stream, so the table of one commit can be compared exactly with
another's: tests/test_gpu_unet_state.py imports this module for the configurations and compares what the engine launches with
the table.  Regenerate the table only when the launch stream is MEANT to change.  No reference import: weights come from
tests/golden/unet_small.npz and from seeds.
"""
import contextlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "unet_launch_counts.json")
NS, DILS = [8, 8, 8, 8, 16, 16, 16], [2, 3, 4, 5, 6, 7, 7]
L, FS = 92092, 22050


def small_sd():
    u = np.load(os.path.join(HERE, "unet_small.npz"))
    return {k[3:]: torch.from_numpy(np.asarray(u[k])) for k in u.files if k.startswith("sd.")}


def _net(sd, **network):
    from babe_amd.config import default_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    args = default_args(sample_rate=FS, audio_len=L, Ns=list(NS))
    for k, v in network.items():
        args.network[k] = v
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(sd, strict=True)
    net.MAX_LANES = 2
    net.engine()                            # packing the weights is not part of the evaluation
    return net


def _inputs(B, seed):
    gen = torch.Generator().manual_seed(seed)
    x = (0.1 * torch.randn(B, L, generator=gen)).cuda()
    cn = torch.linspace(-0.4, 0.3, B).reshape(B, 1).cuda()
    return x, cn, torch.randn(B, L, generator=gen).cuda()


def _count(fn):
    from babe_amd._lib import dispatch_counts
    torch.cuda.synchronize()
    dispatch_counts(reset=True)
    fn()
    torch.cuda.synchronize()
    return dispatch_counts(reset=True)


def _evaluation(net, B, seed):
    x, cn, w = _inputs(B, seed)
    return _count(lambda: (net.fwd_nograd(x, cn), net.vjp(w)))


def small_b1():
    return _evaluation(_net(small_sd()), 1, 1)


def small_b2_two_lanes():
    return _evaluation(_net(small_sd()), 2, 2)


def training_step():
    """Forward and backward of <net(x), w> with every trainable parameter requiring grad, B = 2 on two lanes."""
    net = _net(small_sd()).set_trainable(True)
    x, cn, w = _inputs(2, 3)
    return _count(lambda: (net(x, cn) * w).sum().backward())


def attention():
    """attention_layers [0,0,0,0,1,1,1,1] with relative-position buckets (the fixture 'a' of tests/attention_weights.py)."""
    from tests.attention_weights import LAST_TWO, attention_dict, attention_sd
    ad = attention_dict()
    return _evaluation(_net(attention_sd(NS, DILS, LAST_TWO, ad), attention_layers=list(LAST_TWO), attention_dict=ad), 1, 4)


CASES = {"small_b1": small_b1, "small_b2_two_lanes": small_b2_two_lanes, "training_step": training_step, "attention": attention}


@contextlib.contextmanager
def selected_forms(**select):
    """Run the body under these forms (babe_amd/forms.py) and put back what was selected before, whatever the body does."""
    from babe_amd.forms import FORMS
    keep = {name: getattr(FORMS, name) for name in select}
    try:
        for name, value in select.items():
            setattr(FORMS, name, value)
        yield
    finally:
        for name, value in keep.items():
            setattr(FORMS, name, value)


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    # the table is the Python sequencer's, with the default two-launch GroupNorm statistics
    with selected_forms(unet_c=False, gn_fused=False):
        table = {name: fn() for name, fn in CASES.items()}
    with open(out, "w") as fh:
        json.dump(table, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(f"{out}: " + ", ".join(f"{k}: {sum(v.values())} launches" for k, v in table.items()))
