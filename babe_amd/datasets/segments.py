"""What the three dataset classes share: the reference's draw sequence, a reader that touches only the crop, and a state that can
be saved in the middle of a group of crops.

The reference (datasets/audiofolder.py:58-97, datasets/maestro_dataset.py:59-101 and :140-181) picks a file with
random.randint(0, n-1), reads ALL of it with soundfile, and cuts eight crops at np.random.randint(0, len - seg_len) before it
picks the next file; the MAESTRO classes pass over a file with fewer than five whole segments without drawing a crop.  The same
sequence is drawn here from private random.Random(seed) / np.random.RandomState(seed) instances - bit for bit the sequences the
reference's global random.seed(seed) / np.random.seed(seed) give, but nobody else's draws can shift them and their state can be
saved.  Only the crop is read: a MAESTRO file is about 300 MB, a crop 1.6 MB, and a training step of this tree consumes four
crops every 170 ms.
"""
import random

import numpy as np
import torch

CROPS_PER_FILE = 8                       # "get 8 random batches to be a bit faster" (audiofolder.py:81, maestro_dataset.py:84,163)
WORKER_SEED_STRIDE = 1000003             # DataLoader worker w > 0 draws from seed + w * this (see SegmentStream.__iter__)


def open_wav(path):
    """(sample rate, samples) of a wav file with the samples memory-mapped where scipy can ([frames] or [frames, channels], the
    file's own sample type); a format scipy cannot map (24-bit PCM) is read whole."""
    from scipy.io import wavfile
    try:
        sr, x = wavfile.read(path, mmap=True)
    except ValueError:
        sr, x = wavfile.read(path)
    return int(sr), x


def to_mono_float(x):
    """babe_amd.io.read_audio_file's conversion of a block of samples: integers scaled by 1 / 2^(bits-1), unsigned bytes centred,
    then the channel mean, float32."""
    x = np.asarray(x)
    if x.dtype.kind == "i":
        x = x.astype(np.float32) / float(np.iinfo(x.dtype).max + 1)
    elif x.dtype.kind == "u":
        x = (x.astype(np.float32) - 128.0) / 128.0
    x = x.astype(np.float32)
    if x.ndim == 2:
        x = x.mean(axis=1)
    return x


class SegmentStream(torch.utils.data.IterableDataset):
    """Endless iterator over float32 crops [seg_len] (with_rate: (crop, sample rate)) of the files in `train_samples`.

    skip_short: pass over files with fewer than five whole segments (the MAESTRO classes; the folder class does not).
    overfit: crops start at 0 of samples 10 s .. 60 s of the first file, and nothing is drawn.
    state_dict() / load_state_dict(): both generators' states, the file of the current group and how many of its eight crops
    are out - a stream restored from it continues with the crop the saved one would have yielded next.  The state is the
    iterating process's: under a DataLoader it is meaningful with num_workers = 0 only.
    A DataLoader worker w > 0 reseeds with seed + w * WORKER_SEED_STRIDE so that workers do not all yield one sequence (the
    reference's workers do); worker 0 and num_workers = 0 keep the reference's sequence."""

    def __init__(self, train_samples, seg_len, overfit=False, seed=42, skip_short=False, with_rate=False, crop_reads=True):
        super().__init__()
        if len(train_samples) == 0:
            raise ValueError("error in dataloading: empty or nonexistent folder")
        self.train_samples = list(train_samples)
        self.seg_len = int(seg_len)
        self.overfit = bool(overfit)
        self.seed = seed
        self.skip_short, self.with_rate, self.crop_reads = skip_short, with_rate, crop_reads
        self._seed(seed)
        if self.overfit:
            sr, x = open_wav(self.train_samples[0])
            self.overfit_rate = sr
            self.overfit_sample = to_mono_float(x[10 * sr:60 * sr])                        # "use only 50s"
            if len(self.overfit_sample) < self.seg_len or (skip_short and len(self.overfit_sample) // self.seg_len <= 4):
                raise ValueError(f"{self.train_samples[0]}: samples 10 s .. 60 s hold {len(self.overfit_sample)} samples, too "
                                 f"few for segments of {self.seg_len}")

    def _seed(self, seed):
        self._py = random.Random(seed)
        self._np = np.random.RandomState(seed)
        self._file = None                  # index of the current group's file
        self._pos = 0                      # crops of the current group already yielded (0: the next item opens a group)

    # ---------------------------------------------------------------- state
    def state_dict(self):
        return {"py": self._py.getstate(), "np": self._np.get_state(), "file": self._file, "pos": self._pos}

    def load_state_dict(self, state):
        py = state["py"]
        self._py.setstate((py[0], tuple(py[1]), py[2]))
        self._np.set_state(state["np"])
        self._file, self._pos = state["file"], int(state["pos"])

    # ---------------------------------------------------------------- reads
    def _open(self, path):
        """(sample rate, samples, frames).  crop_reads=False is the reference's whole-file read (tools/loader_bench.py times both)."""
        sr, x = open_wav(path)
        if not self.crop_reads:
            x = to_mono_float(x)
        return sr, x, x.shape[0]

    def _next_group(self):
        """Draw files until one is usable; returns (file index, sample rate, samples, frames)."""
        skipped = 0
        while True:
            num = self._py.randint(0, len(self.train_samples) - 1)
            sr, x, n = self._open(self.train_samples[num])
            if n <= self.seg_len:
                raise ValueError(f"{self.train_samples[num]}: {n} samples, no longer than a segment of {self.seg_len}")
            if self.skip_short and n // self.seg_len <= 4:
                skipped += 1
                if skipped > 100 + 10 * len(self.train_samples):
                    raise ValueError(f"no file with five whole segments of {self.seg_len} samples among the last {skipped} drawn")
                continue
            return num, sr, x, n

    def __iter__(self):
        wi = torch.utils.data.get_worker_info()
        if wi is not None and wi.id > 0:
            self._seed(self.seed + wi.id * WORKER_SEED_STRIDE)
        cur = None                                      # (sample rate, samples, frames) of self._file, once opened here
        while True:
            if self.overfit:
                seg = self.overfit_sample[:self.seg_len]
                yield (seg, self.overfit_rate) if self.with_rate else seg
                continue
            if self._pos == 0 or self._file is None:
                self._file, *cur = self._next_group()
            elif cur is None:                           # restored in the middle of a group: same file, nothing drawn
                cur = self._open(self.train_samples[self._file])
            sr, x, n = cur
            idx = int(self._np.randint(0, n - self.seg_len))
            seg = to_mono_float(x[idx:idx + self.seg_len])
            self._pos = (self._pos + 1) % CROPS_PER_FILE
            self.last_draw = (self._file, idx)          # (for tests and logs)
            yield (seg, sr) if self.with_rate else seg
