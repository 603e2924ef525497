"""Generate tests/golden/attention_train.npz by IMPORTING the reference (training side of the time-attention networks).

Run in the build container only (needs the reference checkout, see oracle/ref_shim.py):
    python tests/golden/make_attention_train_golden.py
Weights: the seeded attention fixtures of tests/attention_weights.py (gate2 is O(1) there, so the attention branch is visible),
loaded into the reference network; the gradient is the reference network's own autograd.grad of <net(x, cnoise), w>.
Two configurations (keys prefixed "a." and "b."):
  a: fixture "a" - reduced width, L = 92092, attention_layers [0,0,0,0,1,1,1,1], relative position bias on, B = 2;
  b: fixture "b" - attention on all 8 levels, use_rel_pos=False, bias_qkv=True, B = 1, L = 92092 (recorded as "b.L").
Stored per configuration (data only; inputs and directions are re-derived from the seeds stored beside them):
  * the reference's trainable set (named_parameters with requires_grad), in order;
  * per trainable tensor the gradient's norm and 4 projections.  Directions come from ONE torch.Generator().manual_seed(dir_seed),
    tensor by tensor in the stored key order: torch.randn(4, numel) for every tensor except the attn_block.qk.weight tensors
    [2HF, HF, 1], which take 4 rank-1 directions u v^T with u = torch.randn(4, 2HF) then v = torch.randn(4, HF), i.e. u^T G v
    (a Gaussian direction of a 25.7 M-element tensor would be 100 MB each).
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

from tests.attention_weights import FIXTURES, fixture_sd  # noqa: E402

net_mod = importlib.import_module("networks.cqtdiff+")

CONFIGS = {"a": ("a", 2, 6100, 6177), "b": ("b", 1, 6200, 6277)}       # name -> (fixture, B, grad seed, direction seed)


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def grads(name):
    fixture, B, grad_seed, dir_seed = CONFIGS[name]
    Ns, fs, L, layers, adict = FIXTURES[fixture]
    args = ref_shim.load_args(exp="maestro22k_8s" if fs == 22050 else "maestro44k_8s")
    args.exp.audio_len, args.exp.sample_rate = L, fs
    args.network.Ns = list(Ns)
    args.network.attention_layers = list(layers)
    args.network.attention_dict = ref_shim.to_attr(dict(adict))
    with quiet():
        net = net_mod.Unet_CQT_oct_with_attention(args, "cpu")
    net.load_state_dict(fixture_sd(fixture), strict=True)
    trainable = [k for k, p in net.named_parameters() if p.requires_grad]
    g = torch.Generator().manual_seed(grad_seed)
    x = 0.1 * torch.randn(B, L, generator=g)
    cn = torch.linspace(-0.4, 0.3, B).reshape(B, 1) if B > 1 else torch.tensor([[-0.4]])
    w = torch.randn(B, L, generator=g)
    with quiet():
        y = net(x, cn)
    ps = dict(net.named_parameters())
    gr = torch.autograd.grad((y * w).sum(), [ps[k] for k in trainable])
    gd = torch.Generator().manual_seed(dir_seed)
    norms, projs = [], []
    for k, t in zip(trainable, gr):
        t = t.double()
        norms.append(float(t.norm()))
        if k.endswith("attn_block.qk.weight"):
            u = torch.randn(4, t.shape[0], generator=gd).double()
            v = torch.randn(4, t.shape[1], generator=gd).double()
            projs.append(torch.einsum("ko,oi,ki->k", u, t.reshape(t.shape[0], t.shape[1]), v).numpy())
        else:
            d = torch.randn(4, t.numel(), generator=gd).double()
            projs.append((d @ t.reshape(-1)).numpy())
    p = name + "."
    return {p + "trainable": np.array(trainable), p + "grad_norm": np.array(norms), p + "grad_proj": np.stack(projs),
            p + "grad_seed": grad_seed, p + "dir_seed": dir_seed, p + "cnoise": cn.numpy(), p + "B": B, p + "L": L,
            p + "fixture": np.array(fixture)}


if __name__ == "__main__":
    out = {}
    for name in CONFIGS:
        out.update(grads(name))
        print("done", name, flush=True)
    path = os.path.join(HERE, "attention_train.npz")
    np.savez_compressed(path, **out)
    print("wrote attention_train.npz", os.path.getsize(path), "bytes")
