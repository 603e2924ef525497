"""The fused optimizer tail in the network and the trainer, at the reduced network shapes of tests/test_gpu_trainer.py: the
packed conv images follow a FusedAdamEMA.step (version counters), a fused trainer against the stock one over two iterations, resume
through checkpoints in every direction, and `python -m babe_amd.train --fused-tail` on one and two ranks.  Needs a MI355X."""
import json
import os
import sys

import pytest
import torch

from tests.test_gpu_optim import BARS, EPS
from tests.test_gpu_train_cli import child, env_dist, env_plain, setup, torchrun  # noqa: F401  (setup: the CLI tests' fixture)
from tests.test_gpu_trainer import FS, NS, L, RecordingEDM, small_sd, snapshot
from tests.train_fixtures import write_wavs

pytestmark = pytest.mark.gpu


def make_net(sd=None):
    from babe_amd.config import default_train_args
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    args = default_train_args(sample_rate=FS, audio_len=L, Ns=NS)
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(small_sd() if sd is None else sd, strict=True)
    return net, args


def make_trainer(wav_dir, model_dir, fused):
    """tests/test_gpu_trainer.py::make_trainer with the optimizer chosen."""
    from babe_amd.config import default_train_args
    from babe_amd.datasets import AudioFolderDataset
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    from babe_amd.optim import FusedAdamEMA
    from babe_amd.training import Trainer
    args = default_train_args(sample_rate=FS, audio_len=L, Ns=NS)
    args.exp.update(batch=2, num_workers=0, exp_name="small", model_dir=str(model_dir), lr=1e-3, lr_rampup_it=2, seed=42)
    args.dset.update(name="audiofolder", callable="datasets.audiofolder.AudioFolderDataset", path=str(wav_dir))
    args.logging.update(log_interval=1, save_interval=1000, freq_cqt_logging=2, num_sigma_bins=20)
    ds = AudioFolderDataset(args.dset, fs=FS, seg_len=L, seed=args.exp.seed)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, num_workers=0)
    net = Unet_CQT_oct_with_attention(args, "cuda")
    net.load_state_dict(small_sd(), strict=True)
    net.set_trainable(True)
    cls = FusedAdamEMA if fused else torch.optim.Adam
    opt = cls(net.parameters(), lr=args.exp.lr, betas=(0.9, 0.999), eps=1e-8)
    return Trainer(args, loader, net, opt, RecordingEDM(args), device="cuda")


@pytest.fixture(scope="module")
def wavs(tmp_path_factory):
    d = tmp_path_factory.mktemp("wavs")
    write_wavs(str(d), fs=FS, seconds=(6.0, 6.0, 6.0))
    return d


# ------------------------------------------------------------------------------------------------------------------- repack
def test_both_networks_repack_after_a_fused_step():
    """The kernel writes the parameters behind torch's back; the network decides from their version counters whether to repack
    its conv images.  After one step at a non-zero learning rate the next forward of the network and of the EMA network must be
    the forward of fresh networks loaded from their state_dict()s - which fails if the counters are not advanced."""
    from babe_amd.diff_params.edm import EDM
    from babe_amd.optim import FusedAdamEMA
    net, args = make_net()
    net.set_trainable(True)
    ema, _ = make_net()
    ema.eval().requires_grad_(False)
    g = torch.Generator().manual_seed(3)
    x = (0.1 * torch.randn(2, L, generator=g)).cuda()
    cn = torch.tensor([[-0.3], [0.4]], device="cuda")
    with torch.no_grad():
        y0, e0 = net(x, cn).clone(), ema(x, cn).clone()              # both engines have packed their weights now
    torch.manual_seed(11)
    EDM(args).loss_fn(net, x)[0].mean().backward()
    opt = FusedAdamEMA(net.parameters(), lr=1e-2, ema_pairs=zip(net.parameters(), ema.parameters()))
    opt.step(max_grad_norm=1.0, ema_s=0.5)
    with torch.no_grad():
        y1, e1 = net(x, cn).clone(), ema(x, cn).clone()
        yf, ef = make_net(net.state_dict())[0](x, cn), make_net(ema.state_dict())[0](x, cn)
    assert not torch.equal(y1, y0) and not torch.equal(e1, e0)
    assert torch.equal(y1, yf) and torch.equal(e1, ef)
    assert torch.isfinite(y1).all() and float(opt.last_grad_norm) > 0


# ------------------------------------------------------------------------------------------------------------------- trainer
@pytest.fixture(scope="module")
def pair(wavs, tmp_path_factory):
    """A fused and a stock trainer from the same seed, run side by side for two iterations; after each one the state of both
    and the stock trainer's .grad (clip_grad_norm_ has left the clipped gradient there)."""
    dirs = {k: tmp_path_factory.mktemp(k) for k in ("fused", "stock")}
    tr = {}
    for k in dirs:
        torch.manual_seed(5)
        tr[k] = make_trainer(wavs, dirs[k], fused=(k == "fused"))
    assert tr["fused"].fused_tail and not tr["stock"].fused_tail
    steps, norms = [], []
    for it in (0, 1):
        before = snapshot(tr["stock"])
        rng = torch.get_rng_state()
        for k in ("fused", "stock"):
            torch.set_rng_state(rng)                                 # the same sigma and noise draws for both
            tr[k].training_loop(total_its=it + 1)
        gclip = {k: p.grad.detach().clone() for k, p in tr["stock"].network.named_parameters() if p.grad is not None}
        norms.append(float(tr["fused"].optimizer.last_grad_norm))
        steps.append(dict(before=before, fused=snapshot(tr["fused"]), stock=snapshot(tr["stock"]), gclip=gclip))
    logs = {}
    for k, d in dirs.items():
        with open(os.path.join(str(d), "train_log.jsonl")) as f:
            logs[k] = [json.loads(ln) for ln in f]
    return dict(tr=tr, dirs=dirs, steps=steps, logs=logs, norms=norms)


def test_fused_trainer_against_the_stock_trainer(pair):
    """lr_rampup_it = 2: at iteration 0 the learning rate and the EMA decay are 0, so at iteration 1 the weights are still equal
    and both tails see bit-equal gradients.  p, m, v and the EMA agree within twice the bars of the kernel test (the second
    step's inputs already differ by the first's roundings); the logged loss is bit-equal.

    The moments come out bit-equal (the kernel forms them with the fused multiply-adds torch's own kernels are built with); p
    and the EMA differ by the roundings the kernel's double update leaves out.  Measured: iteration 0 all equal; iteration 1
    m 0, v 0, p 3.7, ema 4.4 eps x magnitude.  The gradient norms of this network (0.05, 0.02) are below exp.max_grad_norm = 1:
    both tails form the norm and multiply by exactly 1; clipping that bites is checked in tests/test_gpu_optim.py."""
    logs = pair["logs"]
    assert all(0 < n < 1 for n in pair["norms"])                      # the norm pass ran
    assert [ln["it"] for ln in logs["fused"]] == [0, 1]
    assert [ln["loss"] for ln in logs["fused"]] == [ln["loss"] for ln in logs["stock"]]
    assert [ln["lr"] for ln in logs["fused"]] == [ln["lr"] for ln in logs["stock"]] == [0.0, 5e-4]
    for it, st in enumerate(pair["steps"]):
        b, f, s, gc = st["before"], st["fused"], st["stock"], st["gclip"]
        assert set(f) == set(s) and any(k.startswith("m.") for k in f)
        worst = {"m": 0.0, "v": 0.0, "ema": 0.0, "p": 0.0}
        for name in gc:
            g = gc[name].double()
            m_old = b["m." + name].double() if "m." + name in b else torch.zeros_like(g)
            v_old = b["v." + name].double() if "v." + name in b else torch.zeros_like(g)
            p_old, p_new = b["net." + name].double(), s["net." + name].double()
            mags = {"m": ("m.", m_old.abs() + g.abs()), "v": ("v.", v_old + g * g),
                    "p": ("net.", p_old.abs() + (p_new - p_old).abs()), "ema": ("ema.", b["ema." + name].double().abs() + p_new.abs())}
            for q, (prefix, mag) in mags.items():
                err = (f[prefix + name].double() - s[prefix + name].double()).abs()
                ratio = torch.where(err == 0, torch.zeros_like(err), err / (EPS * mag))
                worst[q] = max(worst[q], float(ratio.max()))
        print(f"\niteration {it}: fused against stock trainer, in eps x magnitude: {worst}")
        for q in worst:
            assert worst[q] <= 2 * BARS[q], (it, q, worst[q])
        if it == 0:                                                  # lr = 0 and decay 0: the weights stay, the EMA is the weights
            assert all(torch.equal(f[k], b[k]) for k in f if k.startswith("net."))
            assert all(torch.equal(f["ema." + k[4:]], f[k]) for k in f if k.startswith("net."))
        else:
            assert sum(not torch.equal(f[k], b[k]) for k in f if k.startswith("net.")) > 100
    # parameters without a gradient (frozen ones) are averaged as update_ema averages them
    last = pair["steps"][1]
    frozen = [k for k, p in pair["tr"]["fused"].network.named_parameters() if p.grad is None]
    for k in frozen:
        mag = last["before"]["ema." + k].double().abs() + last["stock"]["net." + k].double().abs()
        err = (last["fused"]["ema." + k].double() - last["stock"]["ema." + k].double()).abs()
        assert bool((err <= 2 * BARS["ema"] * EPS * mag).all()), k
        assert torch.equal(last["fused"]["net." + k], last["before"]["net." + k])


def _opt_state(tr):
    return [(tr.optimizer.state[p]["step"].clone(), tr.optimizer.state[p]["exp_avg"].clone(), tr.optimizer.state[p]["exp_avg_sq"].clone())
            for p in tr.network.parameters() if p in tr.optimizer.state]


def test_resume_through_checkpoints_in_every_direction(pair, wavs, tmp_path_factory):
    """Fused 2 + 2 iterations through a checkpoint equals the uninterrupted 4 bit for bit; a checkpoint of the fused trainer
    resumes under torch.optim.Adam and one of the stock trainer under the fused tail, `step` and the moments bit-equal at the
    moment of loading, and each continues."""
    # the pair has run 2 iterations each: their checkpoints are the two starting points
    paths = {k: pair["tr"][k].save_checkpoint() for k in ("fused", "stock")}
    saved = {k: _opt_state(pair["tr"][k]) for k in paths}
    ck = {k: torch.load(paths[k], map_location="cpu", weights_only=False) for k in paths}
    assert set(ck["fused"]) == set(ck["stock"]) == {"it", "network", "optimizer", "ema", "args", "rng"}
    assert ck["fused"]["optimizer"]["param_groups"] == ck["stock"]["optimizer"]["param_groups"]
    assert set(ck["fused"]["optimizer"]["state"]) == set(ck["stock"]["optimizer"]["state"])
    # uninterrupted: the fused trainer of the pair goes on to 4
    pair["tr"]["fused"].training_loop(total_its=4)
    want = snapshot(pair["tr"]["fused"])
    for resumed_fused, source in ((True, "fused"), (False, "fused"), (True, "stock")):
        torch.manual_seed(999)
        tr = make_trainer(wavs, pair["dirs"][source], fused=resumed_fused)
        assert tr.resume_from_checkpoint(checkpoint_path=paths[source]) is True and tr.it == 2
        got = _opt_state(tr)
        assert len(got) == len(saved[source]) > 100
        for (s0, m0, v0), (s1, m1, v1) in zip(saved[source], got):
            assert float(s1) == float(s0) == 2.0 and s1.dtype == torch.float32
            assert s1.device.type == "cpu" or not resumed_fused          # FusedAdamEMA keeps `step` on the host
            assert torch.equal(m0, m1) and torch.equal(v0, v1)
        if resumed_fused and source == "fused":
            tr.training_loop(total_its=4)
            have = snapshot(tr)
            assert set(have) == set(want)
            bad = [k for k in want if not torch.equal(want[k], have[k])]
            assert not bad, bad[:5]
        else:
            tr.training_loop(total_its=3)
            assert all(float(s) == 3.0 for s, _, _ in _opt_state(tr))
            assert all(torch.isfinite(p).all() for p in tr.network.parameters())


# ------------------------------------------------------------------------------------------------------------------- command line
def test_command_line_fused_tail_one_and_two_ranks(setup):
    from babe_amd.config import default_args
    from babe_amd.io import load_checkpoint
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    d, cfg, sd = setup
    run = d / "fused1"
    child([sys.executable, "-m", "babe_amd.train", "--config", cfg, "--fused-tail", "--its", "3", f"exp.model_dir={run}"], env_plain())
    net = Unet_CQT_oct_with_attention(default_args(sample_rate=FS, audio_len=L, Ns=NS), "cuda")
    assert load_checkpoint(net, str(run / "cli-3.pt")) == 3
    state = torch.load(str(run / "cli-3.pt"), map_location="cpu", weights_only=False)
    assert set(state) == {"it", "network", "optimizer", "ema", "args", "rng"}
    assert sum(not torch.equal(state["network"][k], sd[k]) for k in sd) > 100          # it trained
    assert any(not torch.equal(state["ema"][k], state["network"][k]) for k in sd)       # and the EMA is an average of its own
    assert all(float(s["step"]) == 3.0 for s in state["optimizer"]["state"].values())
    # two ranks (gloo rendezvous, both on GPU 0) with the same data and noise: the ranks end with bit-equal weights
    common = ["--config", cfg, "--fused-tail", "--its", "2", "exp.seed_per_rank=False"]
    child(torchrun(2) + common + [f"exp.model_dir={d / 'fused2'}", "--dump-params", str(d / "fused2" / "w")], env_dist("gloo"))
    r0, r1 = torch.load(str(d / "fused2" / "w.rank0.pt")), torch.load(str(d / "fused2" / "w.rank1.pt"))
    assert set(r0) == set(r1) and sum(not torch.equal(r0[k], sd[k]) for k in sd) > 100
    bad = [k for k in r0 if not torch.equal(r0[k], r1[k])]
    assert not bad, bad[:5]
