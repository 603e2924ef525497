"""Training helpers for the CQTDiff+ prior (reference training/trainer.py: train_step :381-424, update_ema :426-439,
state_dict / save_checkpoint :275-293).  Python only: the network's forward and backward are the HIP paths of
networks/cqtdiff_plus.py (call net.set_trainable() first).  `Trainer` puts them into the reference's loop (:540-586) with its
resume (:209-270) and a JSON-lines log in place of wandb; datasets are babe_amd/datasets, the command line is babe_amd/train.py."""
import glob
import json
import os
import re
import time

import numpy as np
import torch


def train_step(net, optimizer, diff_params, get_batch, it, *, lr, lr_rampup_it=0, num_accumulation_rounds=1,
               use_grad_clip=True, max_grad_norm=1.0, group=None, ema_s=None):
    """One optimizer step: zero_grad, `num_accumulation_rounds` x (loss_fn on get_batch(), loss.mean().backward()), the linear
    learning-rate ramp-up while it <= lr_rampup_it, clip_grad_norm_, step.  Returns (loss of the last round, error, sigma).
    group: a torch.distributed process group; the gradients are averaged over its ranks (allreduce_grads) after the accumulation
    rounds, so the ramp, the clipping and the step see the same gradient on every rank.  None: nothing is added.
    An optimizer with the fused tail (optim.FusedAdamEMA) clips inside its step() and averages its attached EMA tensors there
    with the decay ema_s (None: no EMA); .grad then keeps the unclipped gradient."""
    optimizer.zero_grad()
    for _ in range(num_accumulation_rounds):
        audio = get_batch()
        error, sigma = diff_params.loss_fn(net, audio)
        loss = error.mean()
        loss.backward()
    if group is not None:
        allreduce_grads(net.parameters(), group)
    if it <= lr_rampup_it:
        for g in optimizer.param_groups:
            g["lr"] = lr * min(it / max(lr_rampup_it, 1e-8), 1)
    if getattr(optimizer, "fused_tail", False):
        optimizer.step(max_grad_norm=max_grad_norm if use_grad_clip else None, ema_s=ema_s)
        return loss.detach(), error.detach(), sigma
    if use_grad_clip:
        torch.nn.utils.clip_grad_norm_(net.parameters(), max_grad_norm)
    optimizer.step()
    return loss.detach(), error.detach(), sigma


def ema_decay(it, batch, ema_rampup=10000, ema_rate=0.9999):
    """The EMA's decay at iteration `it`: t / ema_rampup clipped to [0, ema_rate] while t = it * batch is below ema_rampup,
    ema_rate from there on (reference :426-439)."""
    t = it * batch
    return np.clip(t / ema_rampup, 0.0, ema_rate) if t < ema_rampup else ema_rate


def update_ema(ema, net, it, batch, ema_rampup=10000, ema_rate=0.9999):
    """Exponential moving average of net's parameters into ema's (in place; the ema network repacks on its next forward)."""
    s = ema_decay(it, batch, ema_rampup, ema_rate)
    with torch.no_grad():
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


def allreduce_grads(params, group):
    """Average the gradients over the ranks of `group`: the .grad of every parameter that has one is packed into ONE flat fp32
    buffer, summed with a single all_reduce, multiplied by 1 / world and copied back.  A parameter without a gradient is skipped -
    on every rank alike, or the buffers differ in length.  Under gloo a device buffer goes through host memory (gloo reduces
    there anyway; dist.gather_results does the same for its gather); RCCL reduces it where it is."""
    import torch.distributed as dist
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        return
    world = dist.get_world_size(group)
    flat = torch.cat([g.detach().reshape(-1).to(torch.float32) for g in grads])
    if flat.is_cuda and dist.get_backend(group) == "gloo":
        host = flat.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        flat = host.to(flat.device)
    else:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    flat.mul_(1.0 / world)
    o = 0
    with torch.no_grad():
        for g in grads:
            n = g.numel()
            g.copy_(flat[o:o + n].view_as(g))
            o += n


class _LossTap:
    """diff_params as train_step sees it, keeping the signed error of the last loss_fn call for the log."""

    def __init__(self, diff_params):
        self.diff_params, self.residual, self.want = diff_params, None, False

    def loss_fn(self, net, x):
        if not self.want:
            return self.diff_params.loss_fn(net, x)
        err2, sigma, self.residual = self.diff_params.loss_fn(net, x, return_residual=True)
        return err2, sigma


class Trainer:
    """The reference's Trainer (training/trainer.py:35-586) on this tree's step functions, without wandb, the profiler hook
    and the sampling demos.

    args: config.default_train_args() or a loaded YAML (exp, network, diff_params, dset, logging).  dset: a DataLoader (its
    .dataset's state_dict() goes into checkpoints when it has one) or any iterator of batches.  network: trainable
    (set_trainable) and on `device`; optimizer over its parameters; diff_params: diff_params.edm.EDM.
    group: a torch.distributed process group for data parallelism - every rank computes its own batch, the gradients are
    averaged (allreduce_grads) and every rank applies the same update; only rank 0 keeps the EMA, writes checkpoints and the
    log.  save_checkpoint() is collective there: every rank calls it (training_loop does) so that rank 0 can store every rank's
    generator and dataset state.

    `ema` is a second network built from the same args and loaded with network.state_dict(), requires_grad off (no deepcopy:
    the module owns library handles).

    Checkpoints hold the reference's five keys ('it', 'network', 'optimizer', 'ema', 'args') and one more, 'rng':
    {'torch': [per rank: the CPU generator state - loss_fn draws sigma and the noise there],
     'dataset': [per rank: dataset.state_dict() or None]}.  The reference saves neither, so its resumed run sees other data and
    other noise than the uninterrupted one; here it continues the same sequence (num_workers = 0).
    An in-loop checkpoint is written, as in the reference, BEFORE `it` is incremented: <exp_name>-<it>.pt holds the state after
    it + 1 steps and a run resumed from it repeats index `it` for the learning-rate and EMA ramps.  training_loop(total_its)
    also writes one after its last iteration, named for the number of steps done; resuming from that one is exact.

    Log: one JSON line per logged iteration in <model_dir>/train_log.jsonl - it, loss, lr, step_s, error_sigma {bin edge: mean
    error of the rows whose sigma fell in (previous edge, edge]} and, every logging.freq_cqt_logging iterations, band_energy
    (mean over the batch of CQT_nsgt.band_energy of the signed error; band_f, the bins' centre frequencies, with the first of
    them).  The reference reports, per sigma bin, the error of the bin's FIRST row only (:350-352); this is the mean over the
    bin's rows.  Binning runs on the GPU and everything a line needs comes to the host in one transfer."""

    def __init__(self, args, dset, network, optimizer, diff_params, device="cuda", group=None):
        self.args, self.network, self.optimizer, self.device, self.group = args, network, optimizer, device, group
        self.diff_params = diff_params
        self._tap = _LossTap(diff_params)
        self.rank, self.world = 0, 1
        if group is not None:
            import torch.distributed as dist
            self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        self._loader = dset
        self.dataset = getattr(dset, "dataset", None)
        self.dset = iter(dset)
        self.total_params = sum(p.numel() for p in network.parameters() if p.requires_grad)
        self.ema = type(network)(network.args, device, precision=network.precision,
                                 attention_precision=getattr(network, "attention_precision", None))
        self.ema.load_state_dict(network.state_dict())
        self.ema.eval().requires_grad_(False)
        # an optimizer with the fused tail (optim.FusedAdamEMA) averages the EMA in its step(): rank 0 attaches the pairs
        self.fused_tail = bool(getattr(optimizer, "fused_tail", False))
        if self.fused_tail and self.rank == 0:
            optimizer.attach_ema(zip(network.parameters(), self.ema.parameters()))
        self.it = 0
        self.latest_checkpoint = None
        self._saved_it = None                  # `it` of the last checkpoint written or loaded (the same on every rank)
        lg = args.logging
        self.sigma_bins = np.logspace(np.log10(args.diff_params.sigma_min), np.log10(args.diff_params.sigma_max),
                                      num=lg.num_sigma_bins, base=10)
        self._bins_dev = torch.tensor(self.sigma_bins, dtype=torch.float32, device=device)
        self._band_f_logged = False
        self.timers = {"get_batch": 0.0, "train_step": 0.0, "update_ema": 0.0, "log": 0.0, "save": 0.0, "its": 0}
        self.sync_timers = False               # tools: synchronise around every phase so that the timers add up to the wall time

    @property
    def model_dir(self):
        """exp.model_dir, else the reference's top-level model_dir, else the working directory ("None" is the files' unset)."""
        for d in (self.args.exp.get("model_dir", None), self.args.get("model_dir", None)):
            if d not in (None, "None"):
                return str(d)
        return "."

    # ---------------------------------------------------------------- data
    def get_batch(self):
        """The next batch on the device at exp.sample_rate (reference :362-380): maestro_allyears yields (audio, rates) and goes
        through resample_batch; any other set is resampled by exp.resample_factor when that is not 1."""
        from .resample import resample
        from .utils.training_utils import resample_batch
        t0 = time.perf_counter()
        ex = self.args.exp
        if self.args.dset.name == "maestro_allyears":
            audio, fs = next(self.dset)
            audio = resample_batch(audio.to(self.device).to(torch.float32), fs, ex.sample_rate, ex.audio_len)
        else:
            audio = next(self.dset).to(self.device).to(torch.float32)
            if ex.resample_factor != 1:
                audio = resample(audio, ex.resample_factor, 1)
        self.timers["get_batch"] += time.perf_counter() - t0
        return audio

    # ---------------------------------------------------------------- the step functions, with exp.* values
    def train_step(self):
        ex = self.args.exp
        ema_s = None
        if self.fused_tail and self.rank == 0:
            ema_s = ema_decay(self.it, ex.batch, ema_rampup=ex.ema_rampup, ema_rate=ex.ema_rate)
        return train_step(self.network, self.optimizer, self._tap, self.get_batch, self.it, lr=ex.lr,
                          lr_rampup_it=ex.lr_rampup_it, num_accumulation_rounds=ex.num_accumulation_rounds,
                          use_grad_clip=ex.use_grad_clip, max_grad_norm=ex.max_grad_norm, group=self.group, ema_s=ema_s)

    def update_ema(self):
        """Nothing with the fused tail: train_step has averaged already."""
        if self.fused_tail:
            return
        ex = self.args.exp
        update_ema(self.ema, self.network, self.it, ex.batch, ema_rampup=ex.ema_rampup, ema_rate=ex.ema_rate)

    def _rng_state(self):
        mine = (torch.get_rng_state(), self.dataset.state_dict() if hasattr(self.dataset, "state_dict") else None)
        if self.group is None:
            return {"torch": [mine[0]], "dataset": [mine[1]]}
        import torch.distributed as dist
        every = [None] * self.world
        dist.all_gather_object(every, mine, group=self.group)
        return {"torch": [e[0] for e in every], "dataset": [e[1] for e in every]}

    def save_checkpoint(self):
        """<model_dir>/<exp_name>-<it>.pt; removes the one before it under logging.remove_last_checkpoint.  Returns the file name
        (None on ranks other than 0, which only contribute their generator and dataset states)."""
        rng = self._rng_state()
        self._saved_it = self.it
        if self.rank != 0:
            return None
        os.makedirs(self.model_dir, exist_ok=True)
        state = state_dict(self.it, self.network, self.optimizer, self.ema, self.args)
        state["rng"] = rng
        path = os.path.join(self.model_dir, f"{self.args.exp.exp_name}-{self.it}.pt")
        torch.save(state, path)
        if self.args.logging.get("remove_last_checkpoint", False) and self.latest_checkpoint not in (None, path):
            try:
                os.remove(self.latest_checkpoint)
            except OSError:
                print("could not remove last checkpoint", self.latest_checkpoint)
        self.latest_checkpoint = path
        return path

    # ---------------------------------------------------------------- resume
    def _load(self, path):
        return torch.load(path, map_location=self.device, weights_only=False)

    def _restore(self, ck):
        """Load a checkpoint dict: this tree's and the reference's layout key by key, any older layout (io.ema_state_dict) into
        both networks with the optimizer left as it is."""
        from .io import ema_state_dict
        if isinstance(ck, dict) and "network" in ck and "ema" in ck:
            self.network.load_state_dict(ck["network"])
            self.ema.load_state_dict(ck["ema"])
            if "optimizer" in ck:
                self.optimizer.load_state_dict(ck["optimizer"])
        else:
            sd = ema_state_dict(ck, set(self.network.state_dict().keys()))
            self.network.load_state_dict(sd)
            self.ema.load_state_dict(sd)
        self.ema.requires_grad_(False)
        self.it = int(ck["it"]) if isinstance(ck, dict) and "it" in ck else 0
        rng = ck.get("rng") if isinstance(ck, dict) else None
        if rng:
            ds = rng["dataset"][self.rank] if self.rank < len(rng["dataset"]) else None
            if ds is not None and hasattr(self.dataset, "load_state_dict"):
                self.dataset.load_state_dict(ds)
            # a fresh iterator over the restored dataset; a DataLoader draws its base seed from the torch generator when its
            # iterator is made, so the generator's state is set after that
            self.dset = iter(self._loader)
            if self.rank < len(rng["torch"]):
                torch.set_rng_state(rng["torch"][self.rank].cpu())

    def resume_from_checkpoint(self, checkpoint_path=None, checkpoint_id=None):
        """Resume from an explicit file (as given, else under model_dir), from <exp_name>-<checkpoint_id>.pt, or from the
        largest id among model_dir's <exp_name>-*.pt (reference :209-270).  Every rank loads.  Returns True when something was
        loaded; otherwise False with it = 0.  A checkpoint without 'it' resumes at 0 (the reference puts an arbitrary large
        number there)."""
        ex = self.args.exp
        try:
            if checkpoint_path is not None:
                cands = [checkpoint_path, os.path.join(self.model_dir, checkpoint_path)]
                path = next((c for c in cands if os.path.isfile(c)), None)
                if path is None:
                    raise FileNotFoundError(f"{checkpoint_path} (also looked under {self.model_dir})")
            else:
                if checkpoint_id is None:
                    rx = re.compile(re.escape(ex.exp_name) + r"-(\d+)\.pt$")
                    ids = [int(m.group(1)) for m in map(rx.search, glob.glob(os.path.join(self.model_dir, f"{ex.exp_name}-*.pt")))
                           if m]
                    if not ids:
                        raise FileNotFoundError(f"no {ex.exp_name}-*.pt in {self.model_dir}")
                    checkpoint_id = max(ids)
                path = os.path.join(self.model_dir, f"{ex.exp_name}-{checkpoint_id}.pt")
            self._restore(self._load(path))
            self.latest_checkpoint, self._saved_it = path, self.it
            return True
        except Exception as e:                                                   # noqa: BLE001  (as the reference: report, start over)
            print("Could not resume from checkpoint:", e)
            self.it = 0
            return False

    # ---------------------------------------------------------------- log
    def _log_line(self, loss, error, sigma):
        """One dict for train_log.jsonl (the caller adds step_s); one device-to-host copy."""
        nb = len(self.sigma_bins)
        with torch.no_grad():
            rows = error.detach().mean(dim=-1).reshape(-1)                                   # [B]
            idx = torch.bucketize(sigma.detach().reshape(-1).to(torch.float32), self._bins_dev)   # edges[i-1] < s <= edges[i]
            hot = (idx[:, None] == torch.arange(nb, device=idx.device)[None, :]).to(torch.float32)   # sigma above the last edge: none
            parts = [loss.detach().reshape(1), rows @ hot, hot.sum(0)]
            band = self._tap.residual is not None and self._tap.want
            if band:
                parts.append(self.network.CQTransform.band_energy(self._tap.residual.contiguous()).mean(0))
            host = torch.cat(parts).cpu().tolist()
        line = {"it": self.it, "loss": host[0], "lr": self.optimizer.param_groups[0]["lr"]}
        sums, cnt = host[1:1 + nb], host[1 + nb:1 + 2 * nb]
        line["error_sigma"] = {repr(float(self.sigma_bins[i])): sums[i] / cnt[i] for i in range(nb) if cnt[i] > 0}
        if band:
            line["band_energy"] = host[1 + 2 * nb:]
            if not self._band_f_logged:
                line["band_f"] = [float(f) for f in self.network.CQTransform.design["f"]]
                self._band_f_logged = True
        return line

    def _tick(self, key, t0):
        if self.sync_timers:
            torch.cuda.synchronize()
        t = time.perf_counter()
        self.timers[key] += t - t0
        return t

    # ---------------------------------------------------------------- loop
    def training_loop(self, total_its=None):
        """Reference :540-586: train_step, update_ema (rank 0), the checkpoint every logging.save_interval, the log line every
        logging.log_interval, it += 1 - until `it` reaches total_its (None: without end).  With total_its a last checkpoint is
        written when the loop ends (logging.save_model)."""
        lg = self.args.logging
        log_on, save_on = lg.get("log", True), lg.get("save_model", True)
        log_f = None
        if log_on and self.rank == 0:
            os.makedirs(self.model_dir, exist_ok=True)
            log_f = open(os.path.join(self.model_dir, "train_log.jsonl"), "a")
        try:
            while total_its is None or self.it < total_its:
                logging_now = log_on and self.it % lg.log_interval == 0
                self._tap.want = bool(logging_now and self.rank == 0 and self.it % lg.freq_cqt_logging == 0)
                self._tap.residual = None
                if self.sync_timers:
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                gb0 = self.timers["get_batch"]
                loss, error, sigma = self.train_step()
                t1 = self._tick("train_step", t0)
                self.timers["train_step"] -= self.timers["get_batch"] - gb0
                if self.rank == 0:
                    self.update_ema()
                t2 = self._tick("update_ema", t1)
                if self.it > 0 and self.it % lg.save_interval == 0 and save_on:
                    self.save_checkpoint()
                t3 = self._tick("save", t2)
                if logging_now and log_f is not None:
                    line = self._log_line(loss, error, sigma)
                    line["step_s"] = time.perf_counter() - t0          # (after the line's host transfer: the step has finished)
                    log_f.write(json.dumps(line) + "\n")
                    log_f.flush()
                self._tick("log", t3)
                self.timers["its"] += 1
                self.it += 1
            if total_its is not None and save_on and self._saved_it != self.it:
                self.save_checkpoint()
        finally:
            if log_f is not None:
                log_f.close()
