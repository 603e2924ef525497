"""python -m babe_amd.train end to end on the one GPU a test box has, at the reduced network shapes: train, checkpoint, resume;
two ranks (gloo rendezvous, both on GPU 0) with the same data and noise against one process, bit for bit; one rank under
torch.distributed.run on RCCL.  Every child is a fresh process with its own time limit; after a child that faulted, aborted or
hung nothing further is started from this module.  Needs a MI355X."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.train_fixtures import write_wavs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
NS, L, FS = [8, 8, 8, 8, 16, 16, 16], 92092, 22050
_fault = []                                            # why no further child may start


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def child(cmd, env, timeout=600):
    """One fresh process; a fault, an abort or a time limit ends the module's GPU work."""
    if _fault:
        pytest.fail(f"not started: an earlier child run of this module {_fault[0]}")
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _fault.append(f"ran into its time limit ({' '.join(cmd[-6:])})")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stderr:
        _fault.append(f"ended with status {r.returncode}")
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return r


def env_plain():
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "BABE_DIST_BACKEND"):
        e.pop(k, None)
    return e


def env_dist(backend):
    e = env_plain()
    if backend:
        e["BABE_DIST_BACKEND"] = backend
    e["MASTER_ADDR"] = "127.0.0.1"
    e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return e


def torchrun(nproc):
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
            "--master-port", str(_free_port()), "-m", "babe_amd.train"]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli")
    write_wavs(str(d / "wavs"), fs=FS, seconds=(6.0, 6.0, 6.0))
    cfg = d / "small.yaml"
    cfg.write_text(
        f"exp:\n  exp_name: cli\n  sample_rate: {FS}\n  audio_len: {L}\n  batch: 2\n  num_workers: 0\n  lr: 1e-3\n"
        f"  lr_rampup_it: 1\n  resume: True\n  resume_checkpoint: {d / 'init.pt'}\n"
        f"network:\n  Ns: {NS}\n"
        f"dset:\n  name: audiofolder\n  callable: datasets.audiofolder.AudioFolderDataset\n  path: {d / 'wavs'}\n"
        "logging:\n  log_interval: 1\n  save_interval: 3\n  freq_cqt_logging: 2\n")
    u = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(G, "unet_small.npz")).items()}
    sd = {k[3:]: v for k, v in u.items() if k.startswith("sd.")}
    torch.save({"it": 0, "network": sd, "ema": sd}, str(d / "init.pt"))
    return d, str(cfg), sd


def log_its(run_dir):
    with open(os.path.join(str(run_dir), "train_log.jsonl")) as f:
        return [json.loads(ln) for ln in f]


def test_train_three_iterations_then_resume_to_five(setup):
    from babe_amd.config import default_args
    from babe_amd.io import load_checkpoint
    from babe_amd.networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    d, cfg, sd = setup
    run = d / "run1"
    r = child([sys.executable, "-m", "babe_amd.train", "--config", cfg, "--its", "3", f"exp.model_dir={run}"], env_plain())
    assert "Resuming from iteration 0" in r.stdout                              # the initial weights came from init.pt
    ck = run / "cli-3.pt"
    assert ck.is_file() and [ln["it"] for ln in log_its(run)] == [0, 1, 2]
    net = Unet_CQT_oct_with_attention(default_args(sample_rate=FS, audio_len=L, Ns=NS), "cuda")
    assert load_checkpoint(net, str(ck)) == 3
    state = torch.load(str(ck), map_location="cpu", weights_only=False)
    assert set(state) == {"it", "network", "optimizer", "ema", "args", "rng"}
    assert any(not torch.equal(state["network"][k], sd[k]) for k in sd)         # it trained
    for k, p in net.named_parameters():
        assert torch.equal(p.detach().cpu(), state["ema"][k]), k
    # second invocation: picks cli-3.pt up by itself and runs iterations 3 and 4
    r = child([sys.executable, "-m", "babe_amd.train", "--config", cfg, "--its", "5", f"exp.model_dir={run}", "exp.resume=True",
               "exp.resume_checkpoint=None"], env_plain())
    assert "Resuming from iteration 3" in r.stdout
    lines = log_its(run)
    assert [ln["it"] for ln in lines] == [0, 1, 2, 3, 4] and all(np.isfinite(ln["loss"]) for ln in lines)
    assert (run / "cli-5.pt").is_file()


def test_two_ranks_with_the_same_data_equal_one_process_bit_for_bit(setup):
    """exp.seed_per_rank=False: both ranks draw the same crops and the same noise, so their gradients are equal, g + g and
    * 0.5 are exact, and the averaged update is the single-process one.  logging.save_interval=1 puts a collective checkpoint
    (every rank's generator and dataset state, gathered by rank 0) inside the loop."""
    d, cfg, _ = setup
    common = ["--config", cfg, "--its", "2", "exp.seed_per_rank=False", "logging.save_interval=1"]
    child([sys.executable, "-m", "babe_amd.train"] + common + [f"exp.model_dir={d / 'one'}", "--dump-params", str(d / "one" / "w")],
          env_plain())
    child(torchrun(2) + common + [f"exp.model_dir={d / 'two'}", "--dump-params", str(d / "two" / "w")], env_dist("gloo"))
    one = torch.load(str(d / "one" / "w.rank0.pt"))
    r0, r1 = torch.load(str(d / "two" / "w.rank0.pt")), torch.load(str(d / "two" / "w.rank1.pt"))
    init = torch.load(str(d / "init.pt"))["network"]
    assert set(one) == set(r0) == set(r1)
    assert sum(not torch.equal(one[k], init[k]) for k in one) > 100              # the weights moved
    bad = [k for k in one if not (torch.equal(one[k], r0[k]) and torch.equal(one[k], r1[k]))]
    assert not bad, bad[:5]
    ck = torch.load(str(d / "two" / "cli-2.pt"), map_location="cpu", weights_only=False)
    assert len(ck["rng"]["torch"]) == 2 and len(ck["rng"]["dataset"]) == 2
    assert [ln["it"] for ln in log_its(d / "two")] == [0, 1]                     # rank 0 alone writes the log


def test_one_rank_under_torchrun_takes_the_rccl_branch(setup):
    d, cfg, _ = setup
    r = child(torchrun(1) + ["--config", cfg, "--its", "2", f"exp.model_dir={d / 'rccl'}"], env_dist(None))
    assert "world: 1" in r.stdout and "done: it = 2" in r.stdout
    lines = log_its(d / "rccl")
    assert [ln["it"] for ln in lines] == [0, 1] and all(np.isfinite(ln["loss"]) for ln in lines)
    assert (d / "rccl" / "cli-2.pt").is_file()
