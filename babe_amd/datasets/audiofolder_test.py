"""AudioFolderDatasetTest (reference datasets/audiofolder_test.py:30-76): one fixed crop from each of the first files of a folder,
for evaluation."""
import glob
import os

import numpy as np
import torch

from .segments import open_wav, to_mono_float


class AudioFolderDatasetTest(torch.utils.data.Dataset):
    """AudioFolderDatasetTest(dset_args, fs, seg_len, num_samples=4, seed=42): map-style; item i is (segment float32 numpy
    [seg_len], the file's sample rate, the file's name) for the i-th of the first `num_samples` files of dset_args.test.path.

    The file list is glob(path/*.wav) SORTED (the reference takes glob's order, which depends on the file system: AudioFolderDataset
    sorts for the same reason).  The crop start is drawn once, at construction, from a private numpy RandomState(seed) - the
    sequence the reference's np.random.seed(seed) gives; a file shorter than seg_len is tiled, as there.  Only the crop is read
    (datasets/segments.py).  Several channels are mixed down to one unless dset_args.test.stereo is set, which is refused: every
    consumer of this tree is mono (the reference's own mix-down averages over the wrong axis after its transpose)."""

    def __init__(self, dset_args, fs=44100, seg_len=131072, num_samples=4, seed=42):
        super().__init__()
        if dset_args.test.get("stereo", False):
            raise NotImplementedError("dset.test.stereo: the evaluation path is mono")
        files = sorted(glob.glob(os.path.join(dset_args.test.path, "*.wav")))
        if len(files) == 0:
            raise ValueError("error in dataloading: empty or nonexistent folder")
        rng = np.random.RandomState(seed)
        self.train_samples = files
        self.seg_len, self.fs = int(seg_len), fs
        self.test_samples, self.filenames, self._fs = [], [], []
        for path in files[:num_samples]:
            sr, x = open_wav(path)
            n = x.shape[0]
            if n > self.seg_len:
                idx = int(rng.randint(0, n - self.seg_len))
                seg = to_mono_float(x[idx:idx + self.seg_len])
            else:                                   # (n == seg_len: the reference's randint(0, 0) raises; the whole file is the crop)
                seg = np.tile(to_mono_float(x), self.seg_len // n + 1)[:self.seg_len]
            self.test_samples.append(seg)
            self.filenames.append(os.path.basename(path))
            self._fs.append(sr)

    def __getitem__(self, idx):
        return self.test_samples[idx], self._fs[idx], self.filenames[idx]

    def __len__(self):
        return len(self.test_samples)
