"""Training helpers for the CQTDiff+ prior (reference training/trainer.py: train_step :381-424, update_ema :426-439,
state_dict / save_checkpoint :275-293).  Python only: the network's forward and backward are the HIP paths of
networks/cqtdiff_plus.py (call net.set_trainable() first); data loading stays with the caller."""
import os

import numpy as np
import torch


def train_step(net, optimizer, diff_params, get_batch, it, *, lr, lr_rampup_it=0, num_accumulation_rounds=1,
               use_grad_clip=True, max_grad_norm=1.0):
    """One optimizer step: zero_grad, `num_accumulation_rounds` x (loss_fn on get_batch(), loss.mean().backward()), the linear
    learning-rate ramp-up while it <= lr_rampup_it, clip_grad_norm_, step.  Returns (loss of the last round, error, sigma)."""
    optimizer.zero_grad()
    for _ in range(num_accumulation_rounds):
        audio = get_batch()
        error, sigma = diff_params.loss_fn(net, audio)
        loss = error.mean()
        loss.backward()
    if it <= lr_rampup_it:
        for g in optimizer.param_groups:
            g["lr"] = lr * min(it / max(lr_rampup_it, 1e-8), 1)
    if use_grad_clip:
        torch.nn.utils.clip_grad_norm_(net.parameters(), max_grad_norm)
    optimizer.step()
    return loss.detach(), error.detach(), sigma


def update_ema(ema, net, it, batch, ema_rampup=10000, ema_rate=0.9999):
    """Exponential moving average of net's parameters into ema's (in place; the ema network repacks on its next forward)."""
    t = it * batch
    with torch.no_grad():
        s = np.clip(t / ema_rampup, 0.0, ema_rate) if t < ema_rampup else ema_rate
        for dst, src in zip(ema.parameters(), net.parameters()):
            dst.copy_(dst * s + src * (1 - s))


def state_dict(it, net, optimizer, ema, args):
    return {"it": it, "network": net.state_dict(), "optimizer": optimizer.state_dict(), "ema": ema.state_dict(), "args": args}


def save_checkpoint(path, it, net, optimizer, ema, args):
    """torch.save of {'it', 'network', 'optimizer', 'ema', 'args'} (what babe_amd.io.load_checkpoint reads).  `path` is a file
    name or a directory (then <dir>/<args.exp.exp_name>-<it>.pt, the reference's name).  Returns the file name."""
    if os.path.isdir(path):
        path = os.path.join(path, f"{args.exp.exp_name}-{it}.pt")
    torch.save(state_dict(it, net, optimizer, ema, args), path)
    return path
