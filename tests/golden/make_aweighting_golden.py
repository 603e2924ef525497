"""Generate tests/golden/aweighting.npz by IMPORTING the reference (the A-weighted training loss).

Run in the build container only (needs the reference checkout, see oracle/ref_shim.py):
    python tests/golden/make_aweighting_golden.py
Contents (data only):
  * the reference FIRFilter's taps (utils/training_utils.py:71-122) for "aw" at fs = 44100 and 22050 (101 taps) and at 16000 with 51
    taps, and for "hp" and "fd" (coef 0.85);
  * the reference EDM.loss_fn with diff_params.aweighting = {use_aweighting: True, ntaps: 101} (conf/diff_params/edm.yaml otherwise,
    exp maestro22k_8s: fs = 22050) and the stub network of make_train_golden.loss() (net(x, c) = STUB_A * x + STUB_B * c) after
    torch.manual_seed(LOSS_SEED), for x of shape [3, 400] and [3, 50] (shorter than the filter): x, sigma, noise, input, target,
    cnoise, error**2, and the diff_params it ran with;
  * the asymmetric filters applied: FIRFilter("hp", ntaps=3) and ("fd", ntaps=3) on a seeded [2, 37] tensor (ntaps = 3 because
    forward() pads by ntaps//2 whatever the filter: at the default 101 a 3-tap filter returns L + 98 samples);
  * the two diff_params files of the reference that switch A-weighting on, parsed and dumped again as YAML text (settings only).
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
tu_mod = importlib.import_module("utils.training_utils")

LOSS_SEED, X_SEED, ASYM_SEED = 123, 1, 11
STUB_A, STUB_B = 0.5, -0.25
FILTERS = {"aw_44100_101": dict(filter_type="aw", fs=44100), "aw_22050_101": dict(filter_type="aw", fs=22050),
           "aw_16000_51": dict(filter_type="aw", fs=16000, ntaps=51), "hp": dict(filter_type="hp"), "fd": dict(filter_type="fd")}


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def taps():
    return {"taps_" + k: tu_mod.FIRFilter(**kw).fir.weight.data.reshape(-1).numpy() for k, kw in FILTERS.items()}


def loss(tag, L):
    args = ref_shim.load_args(exp="maestro22k_8s")
    args.diff_params.aweighting.use_aweighting = True
    args.diff_params.aweighting.ntaps = 101
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
    x = torch.randn(3, L, generator=torch.Generator().manual_seed(X_SEED))
    torch.manual_seed(LOSS_SEED)
    with quiet():
        err, sigma = e.loss_fn(lambda a, c: STUB_A * a + STUB_B * c, x)
    dp = args.diff_params
    out = {"x": x, "sigma": sigma, "noise": rec["noise"], "input": rec["input"], "target": rec["target"], "cnoise": rec["cnoise"],
           "err2": err}
    out = {f"{tag}_{k}": v for k, v in out.items()}
    out.update(loss_seed=LOSS_SEED, stub=np.array([STUB_A, STUB_B]), loss_fs=args.exp.sample_rate, loss_ntaps=101,
               dp=np.array([dp.sigma_min, dp.sigma_max, dp.get("ro_train", dp.ro), dp.sigma_data]))
    return out


def asym():
    e = torch.randn(2, 37, generator=torch.Generator().manual_seed(ASYM_SEED))
    out = {"asym_in": e}
    for ft in ("hp", "fd"):
        out["asym_" + ft] = tu_mod.FIRFilter(ft, ntaps=3)(e)
    return out


def confs():
    import yaml
    rd = lambda n: yaml.safe_load(open(os.path.join(ref_shim.REF, "conf", "diff_params", n + ".yaml")))
    return {"conf_" + n: np.array(yaml.safe_dump(rd(n))) for n in ("edm_aweighting", "PD_edm_tapehiss")}


if __name__ == "__main__":
    out = dict(source=np.array("reference utils.training_utils.FIRFilter and diff_params.edm.EDM.loss_fn, imported"))
    for part in (taps(), loss("long", 400), loss("short", 50), asym(), confs()):
        out.update({k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in part.items()})
    path = os.path.join(HERE, "aweighting.npz")
    np.savez_compressed(path, **out)
    print("wrote aweighting.npz", os.path.getsize(path), "bytes")
