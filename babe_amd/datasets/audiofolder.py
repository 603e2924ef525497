"""AudioFolderDataset (reference datasets/audiofolder.py:30-97): random crops from the *.wav files of one folder."""
import glob
import os

from .segments import SegmentStream


class AudioFolderDataset(SegmentStream):
    """AudioFolderDataset(dset_args, fs, seg_len, overfit=False, seed=42): yields float32 numpy segments [seg_len] without end.

    dset_args.path: the folder.  The file list is glob(path/*.wav) SORTED - the reference uses glob's order as it comes, which
    depends on the file system, so neither its runs nor a resumed run of ours would be repeatable on another machine.
    No file is passed over for being short (the reference has that test commented out); one no longer than seg_len raises
    ValueError.  `fs` is kept but, as in the reference (whose assert on it is a tuple and never fires), not checked.
    Draw order, reads, overfit and the saved state: datasets/segments.py."""

    def __init__(self, dset_args, fs=44100, seg_len=131072, overfit=False, seed=42):
        files = sorted(glob.glob(os.path.join(dset_args.path, "*.wav")))
        super().__init__(files, seg_len, overfit=overfit, seed=seed, skip_short=False, with_rate=False)
        self.fs = fs
