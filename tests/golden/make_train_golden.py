"""Generate tests/golden/train.npz by IMPORTING the reference (training side).

Run in the build container only (needs the reference checkout, see oracle/ref_shim.py):
    python tests/golden/make_train_golden.py
Contents (data only; inputs are re-derived from the seeds stored beside them):
  * the reference network's trainable set (named_parameters with requires_grad) and all parameter names;
  * on the weights of unet_small.npz: the gradient of <net(x, cnoise), w> (B = 2, seeded x, w) w.r.t. every trainable tensor,
    stored compactly as the norm and the projections onto 4 Gaussian directions per tensor (directions drawn from
    torch.Generator().manual_seed(DIR_SEED), tensor by tensor in the stored key order, torch.randn(4, numel));
  * the reference EDM.loss_fn with a stub network (net(x, c) = STUB_A * x + STUB_B * c) after torch.manual_seed(LOSS_SEED):
    sigma, noise, input, target, cnoise, error**2, and the diff_params it ran with.
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

edm_mod = importlib.import_module("diff_params.edm")
net_mod = importlib.import_module("networks.cqtdiff+")

SMALL_NS = [8, 8, 8, 8, 16, 16, 16]
GRAD_SEED, DIR_SEED, LOSS_SEED = 31, 777, 123
STUB_A, STUB_B = 0.5, -0.25


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def grads():
    args = ref_shim.load_args(exp="maestro22k_8s")
    args.exp.audio_len, args.exp.sample_rate = 92092, 22050
    args.network.Ns = list(SMALL_NS)
    with quiet():
        net = net_mod.Unet_CQT_oct_with_attention(args, "cpu")
    u = np.load(os.path.join(HERE, "unet_small.npz"))
    net.load_state_dict({k[3:]: torch.from_numpy(np.asarray(u[k])) for k in u.files if k.startswith("sd.")})
    params = [k for k, _ in net.named_parameters()]
    trainable = [k for k, p in net.named_parameters() if p.requires_grad]
    g = torch.Generator().manual_seed(GRAD_SEED)
    L = args.exp.audio_len
    x = 0.1 * torch.randn(2, L, generator=g)
    cn = torch.tensor([[-0.4], [0.3]])
    w = torch.randn(2, L, generator=g)
    with quiet():
        y = net(x, cn)
    ps = dict(net.named_parameters())
    gr = torch.autograd.grad((y * w).sum(), [ps[k] for k in trainable])
    gd = torch.Generator().manual_seed(DIR_SEED)
    norms, projs = [], []
    for k, t in zip(trainable, gr):
        d = torch.randn(4, t.numel(), generator=gd).double()
        norms.append(float(t.double().norm()))
        projs.append((d @ t.double().reshape(-1)).numpy())
    return dict(params=np.array(params), trainable=np.array(trainable), grad_norm=np.array(norms), grad_proj=np.stack(projs),
                grad_seed=GRAD_SEED, dir_seed=DIR_SEED, grad_cnoise=cn.numpy())


def loss():
    args = ref_shim.load_args()
    e = edm_mod.EDM(args)
    rec = {}
    orig_prior, orig_prep = e.sample_prior, e.prepare_train_preconditioning

    def prior(shape, sigma):
        n = orig_prior(shape, sigma)
        rec["noise"] = n.clone()
        return n

    def prep(x, sigma):
        i, t, c = orig_prep(x, sigma)
        rec["input"], rec["target"], rec["cnoise"] = i.clone(), t.clone(), c.clone()
        return i, t, c

    e.sample_prior, e.prepare_train_preconditioning = prior, prep
    x = torch.randn(3, 50, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(LOSS_SEED)
    with quiet():
        err, sigma = e.loss_fn(lambda a, c: STUB_A * a + STUB_B * c, x)
    dp = args.diff_params
    return {"loss_x": x, "loss_sigma": sigma, "loss_noise": rec["noise"], "loss_input": rec["input"], "loss_target": rec["target"],
            "loss_cnoise": rec["cnoise"], "loss_err2": err, "loss_seed": LOSS_SEED, "stub": np.array([STUB_A, STUB_B]),
            "dp": np.array([dp.sigma_min, dp.sigma_max, dp.get("ro_train", dp.ro), dp.sigma_data])}


if __name__ == "__main__":
    out = grads()
    out.update({k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in loss().items()})
    np.savez_compressed(os.path.join(HERE, "train.npz"), **out)
    print("wrote train.npz", os.path.getsize(os.path.join(HERE, "train.npz")), "bytes")
