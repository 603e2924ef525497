"""Training datasets (reference datasets/audiofolder.py, datasets/maestro_dataset.py): endless streams of random crops from
wav files.  `dset.callable` of a configuration names them as the reference does (datasets.audiofolder.AudioFolderDataset, ...);
babe_amd.train maps that onto this package.  Test-split datasets (datasets/audiofolder_test.py, datasets/maestro_dataset_test.py):
map-style, a fixed segment per file; `dset_test.callable` names them for babe_amd.evaluate (resolve)."""
import importlib

from .audiofolder import AudioFolderDataset  # noqa: F401
from .maestro_dataset import MaestroDataset, MaestroDataset_fs  # noqa: F401
from .audiofolder_test import AudioFolderDatasetTest  # noqa: F401
from .maestro_dataset_test import MaestroDatasetTestChunks  # noqa: F401


def resolve(name):
    """The class a configuration's `callable` names: the reference's `datasets.X.Y` is `babe_amd.datasets.X.Y` here."""
    if name.startswith("datasets."):
        name = "babe_amd." + name
    mod, cls = name.rsplit(".", 1)
    return getattr(importlib.import_module(mod), cls)
