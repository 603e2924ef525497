"""Generate the frequency-encoding golden vectors (tests/golden/fencoding_*.npz) by IMPORTING the reference with
args.network.use_fencoding = True.

Run in the build container only (needs the reference sources, see oracle/ref_shim.py):
    python tests/golden/make_fencoding_golden.py [a b]
Weights: tests/fencoding_weights.py (babe_amd's init_state_dict(seed, use_fencoding=True)), loaded into the reference network.  The
`embeddings` tables are NOT taken from there: the seeded RFF_freq is written into each of the reference's AddFreqEncodingRFF modules
and its own build_RFF_embedding() rebuilds the table, which is what the fixture stores and what the reference then runs with.
Reduced width Ns = [8,8,8,8,16,16,16], 22.05 kHz, L = 92092.  Data only:
  a: B = 2 - the seven embeddings, y, the reference's parameter names (with shapes) and trainable list, and per trainable tensor
     the gradient norm and four seeded projections (the scheme of train.npz); the input-VJP gx for the same seeded cotangent is
     fencoding_a_vjp.npz;
  b: attention_layers [0,0,0,0,1,1,1,1] as well, B = 1 - y and gx.
"""
import contextlib
import importlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from oracle.nsgt import CQT_nsgt  # noqa: E402

ref_shim.install(CQT_nsgt)
torch.set_num_threads(8)

from tests.attention_weights import SMALL_NS  # noqa: E402
from tests.fencoding_weights import FIXTURES, FS, L, fencoding_sd  # noqa: E402

net_mod = importlib.import_module("networks.cqtdiff+")
SEEDS = {"a": 6100, "b": 6200}
DIR_SEED = 778


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def save(name, **kw):
    np.savez_compressed(os.path.join(HERE, name), **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in kw.items()})
    print("wrote", name, os.path.getsize(os.path.join(HERE, name)) // 1024, "KiB")


def ref_net(name):
    layers, adict, _ = FIXTURES[name]
    args = ref_shim.load_args(exp="maestro22k_8s")
    args.exp.audio_len, args.exp.sample_rate = L, FS
    args.network.Ns = list(SMALL_NS)
    args.network.use_fencoding = True
    if layers:
        args.network.attention_layers = list(layers)
        args.network.attention_dict = ref_shim.to_attr(dict(adict))
    with quiet():
        net = net_mod.Unet_CQT_oct_with_attention(args, "cpu")
    sd = fencoding_sd(name)
    embs = []
    for i, fe in enumerate(net.freq_encodings):          # the reference builds each table from the seeded frequencies
        fe.RFF_freq.data.copy_(sd[f"freq_encodings.{i}.RFF_freq"])
        embs.append(fe.build_RFF_embedding().clone())
        sd[f"freq_encodings.{i}.embeddings"] = embs[-1]
    net.load_state_dict(sd, strict=True)
    return net, torch.stack(embs)


def run(name):
    net, embs = ref_net(name)
    B = FIXTURES[name][2]
    g = torch.Generator().manual_seed(SEEDS[name])
    x = (0.1 * torch.randn(B, L, generator=g)).requires_grad_(True)
    cn = torch.tensor([[-0.4], [0.3]])[:B]
    w = torch.randn(B, L, generator=g)
    with quiet():
        y = net(x, cn)
    out = dict(seed=SEEDS[name], cnoise=cn, y=y.detach())
    if name == "b":
        out["gx"], = torch.autograd.grad((y * w).sum(), x)
        return save("fencoding_b.npz", **out)
    params = [f"{k}:{'x'.join(str(s) for s in p.shape)}" for k, p in net.named_parameters()]
    trainable = [k for k, p in net.named_parameters() if p.requires_grad]
    ps = dict(net.named_parameters())
    gr = torch.autograd.grad((y * w).sum(), [x] + [ps[k] for k in trainable])
    gd = torch.Generator().manual_seed(DIR_SEED)
    norms, projs = [], []
    for k, t in zip(trainable, gr[1:]):
        d = torch.randn(4, t.numel(), generator=gd).double()
        norms.append(float(t.double().norm()))
        projs.append((d @ t.double().reshape(-1)).numpy())
    save("fencoding_a_vjp.npz", seed=SEEDS[name], gx=gr[0])          # (a file of its own: each stays below the 1 MiB limit)
    save("fencoding_a.npz", embeddings=embs, params=np.array(params), trainable=np.array(trainable),
         grad_norm=np.array(norms), grad_proj=np.stack(projs), dir_seed=DIR_SEED, **out)


if __name__ == "__main__":
    for w in sys.argv[1:] or ["a", "b"]:
        run(w)
