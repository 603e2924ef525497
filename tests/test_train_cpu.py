"""Training helpers on the CPU: the EDM training draws, preconditioning and loss against the reference's own outputs
(tests/golden/train.npz, written by tests/golden/make_train_golden.py from diff_params/edm.py:88-96, :161-206), the trainable
set against the reference network's, train_step / update_ema on a stub network, the checkpoint round trip."""
import os

import numpy as np
import torch

from babe_amd.config import default_args
from babe_amd.diff_params.edm import EDM


class Stub(torch.nn.Module):
    """net(x, cnoise) = a * x + b * cnoise, the parameters a, b trainable."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.tensor(0.5))
        self.b = torch.nn.Parameter(torch.tensor(-0.25))

    def forward(self, x, cnoise):
        return self.a * x + self.b * cnoise


def fixture():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "train.npz"))


def fixture_edm(g):
    args = default_args()
    dp = args.diff_params
    dp.sigma_min, dp.sigma_max, dp.ro_train, dp.sigma_data = (float(v) for v in g["dp"])
    return EDM(args)


def test_loss_fn_vs_reference_fixture():
    g = fixture()
    edm = fixture_edm(g)
    a, b = (float(v) for v in g["stub"])
    seen = {}

    def stub(inp, cnoise):
        seen["input"], seen["cnoise"] = inp, cnoise
        return a * inp + b * cnoise
    x = torch.from_numpy(g["loss_x"])
    torch.manual_seed(int(g["loss_seed"]))
    err, sigma = edm.loss_fn(stub, x)
    t = lambda k: torch.from_numpy(np.asarray(g[k]))
    assert torch.equal(sigma, t("loss_sigma"))
    assert torch.allclose(seen["input"], t("loss_input"), rtol=1e-6, atol=1e-7)
    assert torch.allclose(seen["cnoise"], t("loss_cnoise"), rtol=1e-6, atol=1e-7)
    assert torch.allclose(err, t("loss_err2"), rtol=1e-5, atol=1e-7)
    # the draws one by one: sample_ptrain_safe (torch.rand), then the noise (torch.randn), then the preconditioning
    torch.manual_seed(int(g["loss_seed"]))
    s = edm.sample_ptrain_safe(x.shape[0]).unsqueeze(-1)
    assert torch.equal(s, t("loss_sigma"))
    inp, target, cn = edm.prepare_train_preconditioning(x, s)
    torch.manual_seed(int(g["loss_seed"]))
    torch.rand(x.shape[0])
    assert torch.allclose(torch.randn(x.shape) * s, t("loss_noise"), rtol=1e-6, atol=1e-7)
    assert torch.allclose(inp, t("loss_input"), rtol=1e-6, atol=1e-7)
    assert torch.allclose(target, t("loss_target"), rtol=1e-5, atol=1e-6)


def test_set_trainable_is_the_reference_trainable_set():
    """set_trainable on a module with every parameter of the reference network (param_specs; the device-free part of the
    module) marks exactly the parameters the reference network has requires_grad on."""
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention, _attach, init_state_dict
    g = fixture()
    m = torch.nn.Module()
    for k, v in init_state_dict([8, 8, 8, 8, 16, 16, 16], [2, 3, 4, 5, 6, 7, 7]).items():
        _attach(m, k, v, is_buffer=k.endswith(".kernel"))
    assert set(k for k, _ in m.named_parameters()) == set(g["params"].tolist())
    Unet_CQT_oct_with_attention.set_trainable(m)
    assert set(k for k, p in m.named_parameters() if p.requires_grad) == set(g["trainable"].tolist())
    Unet_CQT_oct_with_attention.set_trainable(m, False)
    assert not any(p.requires_grad for p in m.parameters())


def test_train_step_ramp_clip_and_ema():
    from babe_amd import training
    torch.manual_seed(0)
    edm = EDM(default_args())
    net, ema = Stub(), Stub()
    opt = torch.optim.Adam(net.parameters(), lr=1.0)
    x = torch.randn(2, 40)
    before = [p.detach().clone() for p in net.parameters()]
    loss, err, sigma = training.train_step(net, opt, edm, lambda: x, it=5, lr=2e-3, lr_rampup_it=10,
                                           num_accumulation_rounds=2, max_grad_norm=1.0)
    assert opt.param_groups[0]["lr"] == 2e-3 * 0.5
    assert all(not torch.equal(p, q) for p, q in zip(net.parameters(), before))
    assert torch.isfinite(loss)
    training.update_ema(ema, net, it=1, batch=2, ema_rampup=10)       # s = 0.2
    assert torch.allclose(ema.a, 0.2 * 0.5 + 0.8 * net.a)


def test_save_checkpoint_round_trip(tmp_path):
    from babe_amd import training
    from babe_amd.io import ema_state_dict
    net, ema = Stub(), Stub()
    with torch.no_grad():
        ema.a.fill_(3.0)
    opt = torch.optim.Adam(net.parameters())
    args = default_args()
    args.exp.exp_name = "unit"
    path = training.save_checkpoint(str(tmp_path), 7, net, opt, ema, args)
    assert path.endswith("unit-7.pt")
    state = torch.load(path, weights_only=False)
    assert set(state) == {"it", "network", "optimizer", "ema", "args"} and state["it"] == 7
    sd = ema_state_dict(state)
    assert float(sd["a"]) == 3.0 and float(sd["b"]) == -0.25
