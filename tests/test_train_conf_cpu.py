"""Training configuration and host logic without a GPU: config.default_train_args() against the reference's files (fixtures),
dotted overrides, which checkpoint a resume picks, and allreduce_grads in a gloo world of two CPU processes."""
import gzip
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import yaml

G = os.path.join(os.path.dirname(__file__), "golden")


def fixture(name):
    from babe_amd.config import to_attr
    with gzip.open(os.path.join(G, name)) as f:
        return to_attr(yaml.safe_load(f))                      # to_attr: load_yaml's float coercion ('2e-4' -> 2e-4)


def carried(ours, theirs, where):
    """Every key `ours` carries is in `theirs` with the same value, section by section; returns the number of leaves."""
    n = 0
    for k, v in ours.items():
        assert k in theirs, f"{where}.{k} is not in the reference's file"
        if isinstance(v, dict):
            n += carried(v, theirs[k], f"{where}.{k}")
        else:
            assert v == theirs[k] and type(v) is type(theirs[k]), (f"{where}.{k}", v, theirs[k])
            n += 1
    return n


def test_default_train_args_equal_the_reference_files_on_every_key_they_carry():
    from babe_amd.config import default_args, default_train_args
    a = default_train_args()
    exp = fixture("config_surface.yaml.gz").exp["maestro44k_8s"]
    assert carried(a.exp, exp, "exp") >= 30
    for k in ("optimizer", "lr", "lr_rampup_it", "batch", "num_accumulation_rounds", "ema_rate", "ema_rampup", "use_grad_clip",
              "max_grad_norm", "resume", "resume_checkpoint", "seed", "resample_factor", "exp_name", "model_dir",
              "scheduler_step_size", "scheduler_gamma", "use_fp16", "augmentations", "num_workers"):
        assert k in a.exp, k
    assert a.exp.optimizer == dict(type="adam", beta1=0.9, beta2=0.999, eps=1e-8) and a.exp.lr == 2e-4
    tc = fixture("train_conf.yaml.gz")
    assert carried(a.dset, tc.dset["maestro_allyears"], "dset") == 8
    assert set(a.logging) <= set(tc.logging_keys_read_by_trainer)
    assert dict(a.logging) == dict(log=True, log_interval=1, save_model=True, save_interval=50000, remove_last_checkpoint=False,
                                   num_sigma_bins=20, freq_cqt_logging=50)
    # everything default_args() has is still there, unchanged, and its arguments pass through
    base = default_args()
    for sec in ("network", "diff_params", "tester"):
        assert a[sec] == base[sec]
    assert all(a.exp[k] == v for k, v in base.exp.items())
    b = default_train_args(sample_rate=22050, audio_len=92092, Ns=[8] * 7)
    assert (b.exp.sample_rate, b.exp.audio_len, b.network.Ns, b.exp.batch) == (22050, 92092, [8] * 7, 4)


def test_dotted_overrides_parse_ints_floats_booleans_and_lists():
    from babe_amd.config import apply_overrides, default_train_args, parse_value
    a = default_train_args()
    apply_overrides(a, ["exp.batch=2", "exp.lr=1e-4", "exp.ema_rate=0.999", "exp.resume=False", "exp.use_grad_clip=true",
                        "dset.years=[2017, 2018]", "exp.model_dir=/tmp/run=1", "exp.resume_checkpoint=None",
                        "exp.optimizer.beta2=0.99", "logging.cqt.fmin=32.7", "network.attention_layers=[0,0,0,0,1,1,1,1]"])
    assert a.exp.batch == 2 and type(a.exp.batch) is int
    assert a.exp.lr == 1e-4 and type(a.exp.lr) is float and a.exp.ema_rate == 0.999
    assert a.exp.resume is False and a.exp.use_grad_clip is True
    assert a.dset.years == [2017, 2018] and a.network.attention_layers == [0, 0, 0, 0, 1, 1, 1, 1]
    assert a.exp.model_dir == "/tmp/run=1" and a.exp.resume_checkpoint == "None"
    assert a.exp.optimizer.beta2 == 0.99 and a.exp.optimizer.beta1 == 0.9
    assert a.logging.cqt.fmin == 32.7                          # a missing section is created
    assert parse_value("-3") == -3 and parse_value("2e4") == 2e4 and parse_value("abc") == "abc"
    with pytest.raises(ValueError):
        apply_overrides(a, ["exp.batch"])
    with pytest.raises(ValueError):
        apply_overrides(a, ["exp.batch.size=3"])


def test_command_line_configuration_merges_file_defaults_and_overrides(tmp_path):
    from babe_amd.train import load_config
    p = tmp_path / "c.yaml"
    p.write_text("exp:\n  lr: 1e-3\n  batch: 8\ndset:\n  name: folder\n  callable: datasets.audiofolder.AudioFolderDataset\n"
                 "model_dir: /somewhere\n")
    a = load_config(str(p), ["exp.batch=2"])
    assert a.exp.lr == 1e-3 and a.exp.batch == 2 and a.exp.ema_rampup == 10000
    assert a.dset.name == "folder" and a.dset.load_len == 405000 and a.exp.model_dir == "/somewhere"


def test_resume_picks_the_largest_checkpoint_id(tmp_path):
    from babe_amd.config import default_train_args
    from babe_amd.training import Trainer
    for n in (2, 10, 9):
        (tmp_path / f"x-{n}.pt").write_bytes(b"stub")
    (tmp_path / "x-11.pt.tmp").write_bytes(b"stub")
    (tmp_path / "xy-50.pt").write_bytes(b"stub")
    args = default_train_args()
    args.exp.update(exp_name="x", model_dir=str(tmp_path))
    t = Trainer.__new__(Trainer)                               # host logic only: no network, no GPU
    t.args, t.rank, t.it = args, 0, 0
    loaded = []
    t._load = lambda path: {"path": path}
    t._restore = lambda ck: (loaded.append(ck["path"]), setattr(t, "it", 10))
    assert t.resume_from_checkpoint() is True and loaded == [str(tmp_path / "x-10.pt")] and t.it == 10
    assert t.latest_checkpoint == str(tmp_path / "x-10.pt")
    assert t.resume_from_checkpoint(checkpoint_id=9) is True and loaded[-1] == str(tmp_path / "x-9.pt")
    assert t.resume_from_checkpoint(checkpoint_path="x-2.pt") is True and loaded[-1] == str(tmp_path / "x-2.pt")
    assert t.resume_from_checkpoint(checkpoint_path=str(tmp_path / "x-9.pt")) is True and loaded[-1] == str(tmp_path / "x-9.pt")
    # nothing to load: False, and the run starts at 0
    assert t.resume_from_checkpoint(checkpoint_path="missing.pt") is False and t.it == 0
    args.exp.exp_name = "none"
    t.it = 5
    assert t.resume_from_checkpoint() is False and t.it == 0
    # a loader that fails (a truncated file) is "nothing loaded" as well
    args.exp.exp_name = "x"

    def broken(path):
        raise RuntimeError("truncated")
    t._load = broken
    assert t.resume_from_checkpoint() is False and t.it == 0


# ---------------------------------------------------------------------------------------------------------------- allreduce_grads
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker_allreduce(rank, world, port, q):
    from babe_amd.training import allreduce_grads, train_step
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    shapes = [(3, 5), (7,), (2, 2, 2), (1,)]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    for i, p in enumerate(params):
        if i != 2:                                             # params[2] has no gradient, on every rank
            p.grad = (torch.arange(p.numel(), dtype=torch.float32).reshape(p.shape) + 1) * (3 * rank + 1) + 100 * i
    allreduce_grads(params, dist.group.WORLD)
    out = [None if p.grad is None else p.grad.clone() for p in params]

    # train_step with a group: the averaged gradient reaches the optimizer (SGD, lr 1: the step IS the gradient)
    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(4))

        def forward(self, x):
            return (self.w * x).sum(-1, keepdim=True)

    class DP:
        def loss_fn(self, net, x):
            return net(x), torch.ones(x.shape[0], 1)

    net = Net()
    opt = torch.optim.SGD(net.parameters(), lr=1.0)
    x = torch.tensor([[1.0, 2.0, 4.0, 8.0]]) * (rank + 1)
    train_step(net, opt, DP(), lambda: x, it=5, lr=1.0, lr_rampup_it=0, use_grad_clip=False, group=dist.group.WORLD)
    q.put((rank, [None if o is None else o.numpy().copy() for o in out], net.w.detach().numpy().copy()))
    dist.barrier()
    dist.destroy_process_group()


def test_allreduce_grads_world2_gloo_gives_every_rank_the_exact_mean():
    import numpy as np
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_allreduce, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    shapes = [(3, 5), (7,), (2, 2, 2), (1,)]
    for rank, grads, w in res:
        for i, (g, s) in enumerate(zip(grads, shapes)):
            if i == 2:
                assert g is None
                continue
            base = np.arange(int(np.prod(s)), dtype=np.float32).reshape(s) + 1
            want = ((base * 1 + 100 * i) + (base * 4 + 100 * i)) / 2              # ranks 0 and 1: factors 1 and 4
            assert g.shape == s and np.array_equal(g, want.astype(np.float32)), (rank, i)
        assert np.array_equal(w, -np.array([1.0, 2.0, 4.0, 8.0], dtype=np.float32) * 1.5)       # mean of x and 2x, one SGD step
