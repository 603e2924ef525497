"""MaestroDataset and MaestroDataset_fs (reference datasets/maestro_dataset.py:31-181): random crops from the training split of
MAESTRO v3, chosen by year."""
import csv
import os

from .segments import SegmentStream


def maestro_files(path, years, split):
    """Paths of the rows of <path>/maestro-v3.0.0.csv with year in `years` and the given split, in the file's order."""
    years = {int(y) for y in years}
    with open(os.path.join(path, "maestro-v3.0.0.csv"), newline="") as f:
        return [os.path.join(path, r["audio_filename"]) for r in csv.DictReader(f)
                if int(r["year"]) in years and r["split"] == split and r["audio_filename"]]


def maestro_train_files(path, years):
    """The training split, in the file's order (maestro_dataset.py:44-54)."""
    return maestro_files(path, years, "train")


class MaestroDataset(SegmentStream):
    """MaestroDataset(dset_args, fs, seg_len, overfit=False, seed=42): float32 numpy segments [seg_len] from dset_args.path,
    years dset_args.years.  A file with fewer than five whole segments is passed over.  overfit=True asserts that the first
    file is at `fs`, like the reference; otherwise the rate is not checked (the reference's assert there is a tuple)."""

    def __init__(self, dset_args, fs=44100, seg_len=131072, overfit=False, seed=42):
        super().__init__(maestro_train_files(dset_args.path, dset_args.years), seg_len, overfit=overfit, seed=seed,
                         skip_short=True, with_rate=False)
        self.fs = fs
        if self.overfit and self.overfit_rate != fs:
            raise ValueError(f"wrong sampling rate: {self.train_samples[0]} is at {self.overfit_rate} Hz, not {fs}")


class MaestroDataset_fs(SegmentStream):
    """MaestroDataset_fs(dset_args, overfit=False, seed=42): (float32 segment [dset_args.load_len], sample rate) - the files keep
    their own rate (44.1 or 48 kHz) and the trainer resamples the batch (utils.training_utils.resample_batch).
    overfit=True: the reference reads self.overfit_sample, which this class never sets there (it would raise); here it follows
    the rule of the other two classes - samples 10 s .. 60 s of the first file, crop start 0."""

    def __init__(self, dset_args, overfit=False, seed=42):
        super().__init__(maestro_train_files(dset_args.path, dset_args.years), int(dset_args.load_len), overfit=overfit,
                         seed=seed, skip_short=True, with_rate=True)
