"""Command line: train the CQTDiff+ prior from audio files on the MI355X path.

    python -m babe_amd.train --config FILE [key.sub=value ...] [--precision f32|bf16] [--wgrad f32|bf16] [--its N]
                               [--dump-params PREFIX] [--fused-tail]

Follows the reference's train.py / utils/setup.py: load the configuration, build the dataset named by dset.callable
(`datasets.X` there is `babe_amd.datasets.X` here) behind a DataLoader (batch_size = exp.batch, num_workers = exp.num_workers;
0 keeps a run and its resume reproducible), the network, Adam (setup.py:70-73) and EDM, resume if exp.resume, run
training.Trainer.training_loop.  FILE is one YAML with the sections exp, network, diff_params, dset, logging (tester optional);
what it leaves out comes from config.default_train_args().  key.sub=value overrides are read as YAML scalars or flow lists.
--its N: stop when the iteration counter reaches N (a resumed run counts from its checkpoint) and write a last checkpoint;
without it the loop runs until interrupted.  A checkpoint loads with `python -m babe_amd.restore --ckpt`.
--fused-tail: gradient clipping, Adam and the EMA as the HIP kernels of optim.FusedAdamEMA instead of clip_grad_norm_,
torch.optim.Adam and update_ema; checkpoints are the same and resume under either.

Several GPUs: start it under torch.distributed.run (RANK, WORLD_SIZE, LOCAL_RANK); rank r trains on cuda:LOCAL_RANK with its
dataset seeded exp.seed + r, gradients are averaged over RCCL (BABE_DIST_BACKEND=gloo for tests that share one GPU), rank 0
keeps the EMA, the checkpoints and the log.  exp.seed_per_rank=False gives every rank the same data and noise - for tests only:
the averaged gradient is then the single-rank one.
"""
import argparse
import os

import numpy as np
import torch


def merge(base, over):
    """`over`'s values into `base`, section by section (in place)."""
    for k, v in over.items():
        if isinstance(v, dict) and isinstance(base.get(k), dict):
            merge(base[k], v)
        else:
            base[k] = v
    return base


def load_config(path, overrides=()):
    from .config import apply_overrides, default_train_args, load_yaml
    args = default_train_args()
    if path:
        merge(args, load_yaml(path))
    apply_overrides(args, overrides)
    if args.exp.get("model_dir", "None") in (None, "None") and args.get("model_dir", "None") not in (None, "None"):
        args.exp.model_dir = args.model_dir
    return args


def build_dataset(args, seed):
    """The dataset object of dset.callable, with the arguments utils/setup.py:10-34 passes: the _fs class gets the dset section
    alone, the others the file rate and length before exp.resample_factor."""
    from .datasets import resolve
    cls = resolve(args.dset.callable)
    overfit = bool(args.dset.get("overfit", False))
    if args.dset.name == "maestro_allyears":
        return cls(args.dset, overfit=overfit, seed=seed)
    rf = args.exp.resample_factor
    return cls(args.dset, fs=args.exp.sample_rate * rf, seg_len=args.exp.audio_len * rf, overfit=overfit, seed=seed)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", help="YAML with exp / network / diff_params / dset / logging sections")
    ap.add_argument("--precision", default="f32", choices=["f32", "bf16"], help="the network's conv arithmetic")
    ap.add_argument("--wgrad", default=None, choices=["f32", "bf16"], help="conv weight-gradient arithmetic")
    ap.add_argument("--its", type=int, default=None, help="stop when the iteration counter reaches N")
    ap.add_argument("--dump-params", default=None, metavar="PREFIX",
                    help="when the loop ends, every rank writes its network's state_dict to PREFIX.rank<r>.pt (to check that "
                         "the ranks hold the same weights)")
    ap.add_argument("--fused-tail", action="store_true",
                    help="gradient norm, clipping, Adam and the EMA in one HIP pass (optim.FusedAdamEMA)")
    ap.add_argument("overrides", nargs="*", help="key.sub=value")
    a = ap.parse_args(argv)
    args = load_config(a.config, a.overrides)

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    group = None
    distributed = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    dev_idx = local_rank % max(torch.cuda.device_count(), 1)
    if distributed:
        import torch.distributed as dist
        from .dist import pin_host_threads
        pin_host_threads(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", world)))       # before the first GPU call
        torch.cuda.set_device(dev_idx)
        backend = os.environ.get("BABE_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev_idx))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        group = dist.group.WORLD
    device = torch.device("cuda", dev_idx)
    torch.cuda.set_device(device)

    from .diff_params.edm import EDM
    from .networks.cqtdiff_plus import Unet_CQT_oct_with_attention
    from .training import Trainer
    seed = args.exp.seed + (rank if args.exp.get("seed_per_rank", True) else 0)
    # the reference's Trainer seeds torch with the first draw of the numpy generator its dataset seeded (trainer.py:55)
    torch.manual_seed(int(np.random.RandomState(seed).randint(1 << 31)))
    dataset = build_dataset(args, seed)
    loader = torch.utils.data.DataLoader(dataset, batch_size=args.exp.batch, num_workers=args.exp.num_workers)
    net = Unet_CQT_oct_with_attention(args, device, precision=a.precision)
    # a bf16 attention core (network.attention_precision=bf16) trains under its own opt-in and bars
    net.set_trainable(True, attention="bf16" if net.bf16_attention else net.has_attention, wgrad=a.wgrad)
    opt = args.exp.optimizer
    if opt.type != "adam":
        raise NotImplementedError(f"exp.optimizer.type={opt.type!r} (the reference implements 'adam' only)")
    if a.fused_tail:
        from .optim import FusedAdamEMA
        optimizer = FusedAdamEMA(net.parameters(), lr=args.exp.lr, betas=(opt.beta1, opt.beta2), eps=opt.eps)
    else:
        optimizer = torch.optim.Adam(net.parameters(), lr=args.exp.lr, betas=(opt.beta1, opt.beta2), eps=opt.eps)
    trainer = Trainer(args, loader, net, optimizer, EDM(args), device=device, group=group)
    if rank == 0:
        print(f"total_params: {trainer.total_params / 1e6:.3f} M, model_dir: {trainer.model_dir}, world: {world}" +
              (f" ({dist.get_backend()})" if distributed else ""), flush=True)
    if args.exp.resume:
        ck = args.exp.get("resume_checkpoint", "None")
        ok = trainer.resume_from_checkpoint(checkpoint_path=None if ck in (None, "None") else ck)
        if rank == 0:
            print(f"Resuming from iteration {trainer.it}" if ok else "training from scratch", flush=True)
    try:
        trainer.training_loop(total_its=a.its)
        if a.dump_params:
            torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()}, f"{a.dump_params}.rank{rank}.pt")
        if distributed:
            dist.barrier()
    finally:
        if distributed:
            dist.destroy_process_group()
    if rank == 0:
        print(f"done: it = {trainer.it}, last checkpoint: {trainer.latest_checkpoint}", flush=True)


if __name__ == "__main__":
    main()
