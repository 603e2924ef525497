"""training.Trainer on the GPU at the reduced network shapes: the batch resampler against the resampler row by row, a resumed run
against the uninterrupted one bit for bit (parameters, EMA, Adam moments - which fails unless the generator and dataset states
travel in the checkpoint), and the contents of the log.  Needs a MI355X."""
import json
import os

import numpy as np
import pytest
import torch

from tests.train_fixtures import write_wavs

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
NS, L, FS = [8, 8, 8, 8, 16, 16, 16], 92092, 22050


# ---------------------------------------------------------------------------------------------------------------- resample_batch
def test_resample_batch_one_rate_and_mixed_rates_equal_resample_row_by_row():
    from babe_amd.resample import resample
    from babe_amd.utils.training_utils import resample_batch
    g = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(3, 6000, generator=g)).cuda()
    # 48000 -> 44100 is (160, 147): ceil(147 * 6000 / 160) = 5513 samples
    got = resample_batch(x, torch.tensor([48000, 48000, 48000]), 44100, 5500)
    assert got.shape == (3, 5500)
    for i in range(3):
        assert torch.equal(got[i], resample(x[i], 160, 147)[:5500])
    # 48000 -> 22050 is (320, 147): 2757 samples
    got = resample_batch(x, [48000, 48000, 48000], 22050, 2750)
    for i in range(3):
        assert torch.equal(got[i], resample(x[i], 320, 147)[:2750])
    # mixed: 44100 rows pass through, cropped
    got = resample_batch(x, torch.tensor([44100, 48000, 44100]), 44100, 5500)
    assert got.shape == (3, 5500)
    assert torch.equal(got[0], x[0, :5500]) and torch.equal(got[2], x[2, :5500])
    assert torch.equal(got[1], resample(x[1], 160, 147)[:5500])
    got = resample_batch(x, [44100, 48000, 44100], 22050, 2750)
    assert torch.equal(got[0], resample(x[0], 2, 1)[:2750]) and torch.equal(got[1], resample(x[1], 320, 147)[:2750])
    assert torch.equal(resample_batch(x, [44100] * 3, 16000, 2000), resample(x, 44100, 16000)[:, :2000])


def test_resample_batch_refuses_unlisted_rates_and_short_rows():
    from babe_amd.utils.training_utils import resample_batch
    x = torch.zeros(2, 6000, device="cuda")
    with pytest.raises(ValueError, match="32000"):
        resample_batch(x, [44100, 32000], 44100, 5000)
    with pytest.raises(ValueError, match="22050"):
        resample_batch(x, [22050, 22050], 22050, 5000)             # the 22050 table has no 22050 row, as in the reference
    with pytest.raises(ValueError, match="length_target"):
        resample_batch(x, [48000, 48000], 44100, 5600)             # 5513 samples come out
    with pytest.raises(ValueError, match="length_target"):
        resample_batch(x, [44100, 48000], 44100, 5600)


# ---------------------------------------------------------------------------------------------------------------- Trainer
def small_sd():
    u = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(G, "unet_small.npz")).items()}
    return {k[3:]: v for k, v in u.items() if k.startswith("sd.")}


class RecordingEDM:
    """EDM that keeps the sigma of every loss_fn call (built lazily: the import needs the library)."""

    def __new__(cls, args):
        from babe_amd.diff_params.edm import EDM

        class _Rec(EDM):
            def __init__(self, a):
                super().__init__(a)
                self.sigmas = []

            def loss_fn(self, net, x, return_residual=False):
                out = super().loss_fn(net, x, return_residual=return_residual)
                self.sigmas.append(out[1].detach().reshape(-1).cpu())
                return out
        return _Rec(args)


def make_trainer(wav_dir, model_dir):
    from babe_amd.config import default_train_args
    from babe_amd.datasets import AudioFolderDataset
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
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
    opt = torch.optim.Adam(net.parameters(), lr=args.exp.lr, betas=(0.9, 0.999), eps=1e-8)
    return Trainer(args, loader, net, opt, RecordingEDM(args), device="cuda")


def snapshot(tr):
    torch.cuda.synchronize()
    out = {"net." + k: p.detach().clone() for k, p in tr.network.named_parameters()}
    out.update({"ema." + k: p.detach().clone() for k, p in tr.ema.named_parameters()})
    for k, p in tr.network.named_parameters():
        st = tr.optimizer.state.get(p)
        if st:
            out["m." + k], out["v." + k] = st["exp_avg"].detach().clone(), st["exp_avg_sq"].detach().clone()
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The uninterrupted run (4 iterations) and the interrupted one (2, checkpoint, fresh objects, resume, 2 more), once."""
    wavs = tmp_path_factory.mktemp("wavs")
    write_wavs(str(wavs), fs=FS, seconds=(6.0, 6.0, 6.0))
    dir_a, dir_b = tmp_path_factory.mktemp("a"), tmp_path_factory.mktemp("b")
    torch.manual_seed(5)
    a = make_trainer(wavs, dir_a)
    start = snapshot(a)
    a.training_loop(total_its=4)
    torch.manual_seed(5)
    b1 = make_trainer(wavs, dir_b)
    b1.training_loop(total_its=2)
    path = b1.save_checkpoint()
    torch.manual_seed(999)                              # the resumed process has no reason to share the first one's generator
    b2 = make_trainer(wavs, dir_b)
    resumed = b2.resume_from_checkpoint()
    it_resumed = b2.it
    b2.training_loop(total_its=4)
    return dict(a=a, b2=b2, start=start, path=path, resumed=resumed, it_resumed=it_resumed, dir_a=dir_a, dir_b=dir_b)


def test_resumed_run_equals_the_uninterrupted_one_bit_for_bit(runs):
    assert runs["resumed"] is True and runs["it_resumed"] == 2 and runs["a"].it == runs["b2"].it == 4
    assert os.path.basename(runs["path"]) == "small-2.pt"
    ck = torch.load(runs["path"], map_location="cpu", weights_only=False)
    assert {"it", "network", "optimizer", "ema", "args", "rng"} == set(ck)
    assert ck["rng"]["dataset"][0]["pos"] == 4          # 2 iterations x 2 rows: in the middle of a group of eight crops
    sa, sb = snapshot(runs["a"]), snapshot(runs["b2"])
    assert set(sa) == set(sb) and any(k.startswith("m.") for k in sa)
    bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not bad, bad[:5]
    moved = [k for k in runs["start"] if k.startswith("net.") and not torch.equal(runs["start"][k], sa[k])]
    assert len(moved) > 100                             # the comparison is of a network that trained
    ema_moved = [k for k in runs["start"] if k.startswith("ema.") and not torch.equal(runs["start"][k], sa[k])]
    assert ema_moved


def test_checkpoint_loads_into_a_new_network(runs):
    from babe_amd.config import default_args
    from babe_amd.io import load_checkpoint
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    net = Unet_CQT_oct_with_attention(default_args(sample_rate=FS, audio_len=L, Ns=NS), "cuda")
    assert load_checkpoint(net, os.path.join(str(runs["dir_a"]), "small-4.pt")) == 4
    for (k, p), (_, q) in zip(net.named_parameters(), runs["a"].ema.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), k


def test_log_lines(runs):
    tr = runs["a"]
    with open(os.path.join(str(runs["dir_a"]), "train_log.jsonl")) as f:
        lines = [json.loads(ln) for ln in f]
    assert [ln["it"] for ln in lines] == [0, 1, 2, 3]
    edges = tr.sigma_bins
    assert len(edges) == 20 and len(tr.diff_params.sigmas) == 4
    for ln, sig in zip(lines, tr.diff_params.sigmas):
        assert np.isfinite(ln["loss"]) and ln["step_s"] > 0
        assert ln["lr"] == 1e-3 * min(ln["it"] / 2, 1)               # the ramp over lr_rampup_it = 2; the resumed run restores it
        # exactly the bins a row's sigma fell into: (previous edge, edge], float32 edges as on the device
        e32 = edges.astype(np.float32)
        want = {repr(float(edges[int(np.searchsorted(e32, np.float32(s), side="left"))])) for s in sig.tolist() if s <= e32[-1]}
        assert set(ln["error_sigma"]) == want and 1 <= len(want) <= 2
        assert all(np.isfinite(v) and v >= 0 for v in ln["error_sigma"].values())
        if ln["it"] % 2 == 0:
            assert len(ln["band_energy"]) == 7 * 64 and all(np.isfinite(v) and v >= 0 for v in ln["band_energy"])
            assert ("band_f" in ln) == (ln["it"] == 0)
        else:
            assert "band_energy" not in ln and "band_f" not in ln
    assert lines[0]["band_f"] == [float(f) for f in tr.network.CQTransform.design["f"]]
