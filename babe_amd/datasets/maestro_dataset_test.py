"""MaestroDatasetTestChunks (reference datasets/maestro_dataset_test.py:30-74): one chunk from each of the first files of the
test split of MAESTRO v3, for evaluation."""
import os

import torch

from .maestro_dataset import maestro_files
from .segments import open_wav, to_mono_float


class MaestroDatasetTestChunks(torch.utils.data.Dataset):
    """MaestroDatasetTestChunks(dset_args, num_samples=4, seed=42): map-style; item i is (segment float32 numpy
    [dset_args.load_len], the file's sample rate, the file's name): the load_len samples that start 10 s into the i-th of the
    first `num_samples` files with split == "test" and year in dset_args.years.

    The csv is read like the training classes read it (datasets/maestro_dataset.py) and the list is SORTED, like
    AudioFolderDataset's and for the same reason: one order on every machine.  Only the chunk is read, mixed down to mono.
    A file that ends before 10 s + load_len raises ValueError (the reference would hand out a shorter segment).  Nothing is drawn:
    `seed` is accepted for the reference's signature."""

    def __init__(self, dset_args, num_samples=4, seed=42):
        super().__init__()
        self.seg_len = int(dset_args.load_len)
        self.filelist = sorted(maestro_files(dset_args.path, dset_args.years, "test"))
        if len(self.filelist) == 0:
            raise ValueError("error in dataloading: no file of the test split in the given years")
        self.test_samples, self.filenames, self.f_s = [], [], []
        for path in self.filelist[:num_samples]:
            sr, x = open_wav(path)
            if x.shape[0] < 10 * sr + self.seg_len:
                raise ValueError(f"{path}: {x.shape[0]} samples, fewer than 10 s + a segment of {self.seg_len}")
            self.test_samples.append(to_mono_float(x[10 * sr:10 * sr + self.seg_len]))
            self.filenames.append(os.path.basename(path))
            self.f_s.append(sr)

    def __getitem__(self, idx):
        return self.test_samples[idx], self.f_s[idx], self.filenames[idx]

    def __len__(self):
        return len(self.test_samples)
