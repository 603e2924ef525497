"""Training datasets (reference datasets/audiofolder.py, datasets/maestro_dataset.py): endless streams of random crops from
wav files.  `dset.callable` of a configuration names them as the reference does (datasets.audiofolder.AudioFolderDataset, ...);
babe_amd.train maps that onto this package."""
from .audiofolder import AudioFolderDataset  # noqa: F401
from .maestro_dataset import MaestroDataset, MaestroDataset_fs  # noqa: F401
