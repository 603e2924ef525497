"""babe_amd.datasets without a GPU: the reference's draw sequence restated with freshly seeded generators, crops against
whole-file reads, the MAESTRO file list, and a state saved in the middle of a group of eight crops."""
import os
import random

import numpy as np
import pytest

from tests.train_fixtures import write_wavs

FS, SEG = 8000, 4000


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = tmp_path_factory.mktemp("wavs")
    return str(d), write_wavs(str(d), fs=FS, seconds=(4.0, 3.5, 3.0))


def attr(**kw):
    from babe_amd.config import to_attr
    return to_attr(kw)


def whole(path):
    from babe_amd.io import read_audio_file
    x, sr = read_audio_file(path)
    return x.numpy(), sr


def expected_draws(lengths, n_items, seed=42, skip_short=False, seg=SEG):
    """The draw rule of datasets/audiofolder.py:61-87 (skip_short: maestro_dataset.py:81-84) with freshly seeded generators."""
    random.seed(seed)
    np.random.seed(seed)
    out = []
    while len(out) < n_items:
        num = random.randint(0, len(lengths) - 1)
        if skip_short and np.floor(lengths[num] / seg) <= 4:
            continue
        for _ in range(8):
            out.append((num, np.random.randint(0, lengths[num] - seg)))
    return out[:n_items]


def test_folder_draws_follow_the_reference_sequence_and_crops_equal_whole_reads(folder):
    from babe_amd.datasets import AudioFolderDataset
    d, paths = folder
    ds = AudioFolderDataset(attr(path=d), fs=FS, seg_len=SEG, seed=42)
    assert ds.train_samples == paths == sorted(paths)
    files = [whole(p)[0] for p in paths]
    assert [len(f) for f in files] == [32000, 28000, 24000] and all(f.ndim == 1 and f.dtype == np.float32 for f in files)
    want = expected_draws([len(f) for f in files], 24)
    assert len({w[0] for w in want}) > 1                              # the 24 items visit more than one file
    it = iter(ds)
    for num, idx in want:
        seg = next(it)
        assert ds.last_draw == (num, idx)
        assert seg.dtype == np.float32 and seg.shape == (SEG,)
        assert np.array_equal(seg, files[num][idx:idx + SEG])


def test_stereo_is_averaged_and_integers_are_scaled(folder):
    from scipy.io import wavfile
    from babe_amd.datasets.segments import open_wav, to_mono_float
    _, paths = folder
    sr, raw = wavfile.read(paths[1])
    assert raw.ndim == 2 and raw.dtype == np.int16
    sr2, x = open_wav(paths[1])
    assert sr2 == sr == FS and isinstance(x, np.memmap)             # only the crop is read
    got = to_mono_float(x[100:100 + SEG])
    want = ((raw[100:100 + SEG, 0].astype(np.float64) + raw[100:100 + SEG, 1]) / 2 / 32768).astype(np.float32)
    assert np.array_equal(got, want)


def test_file_no_longer_than_a_segment_raises(tmp_path):
    from scipy.io import wavfile
    from babe_amd.datasets import AudioFolderDataset
    wavfile.write(str(tmp_path / "short.wav"), FS, np.zeros(SEG, np.int16))
    with pytest.raises(ValueError, match="short.wav"):
        next(iter(AudioFolderDataset(attr(path=str(tmp_path)), fs=FS, seg_len=SEG)))
    with pytest.raises(ValueError, match="empty"):
        AudioFolderDataset(attr(path=str(tmp_path / "nothing")), fs=FS, seg_len=SEG)


def test_24_bit_pcm_falls_back_to_a_whole_read(tmp_path):
    """scipy cannot memory-map 3-byte samples; the file is then read whole (left-justified int32)."""
    import struct
    from babe_amd.datasets.segments import open_wav, to_mono_float
    n = 50
    vals = np.arange(-25, 25, dtype=np.int32) * 70001
    data = b"".join(struct.pack("<i", int(v))[:3] for v in vals)
    hdr = (b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, FS, FS * 3, 3, 24) +
           b"data" + struct.pack("<I", len(data)))
    p = tmp_path / "pcm24.wav"
    p.write_bytes(hdr + data)
    sr, x = open_wav(str(p))
    assert sr == FS and len(x) == n and not isinstance(x, np.memmap)
    assert np.allclose(to_mono_float(x), vals / 2.0 ** 23, atol=0, rtol=1e-7)


@pytest.fixture(scope="module")
def maestro(tmp_path_factory, folder):
    """A 4-row maestro-v3.0.0.csv over the folder's files: two usable rows, one of another year, one of another split."""
    d, paths = folder
    root = tmp_path_factory.mktemp("maestro")
    os.makedirs(os.path.join(str(root), "2017"))
    from scipy.io import wavfile
    rng = np.random.RandomState(1)
    names = ["2017/long_a.wav", "2017/long_b.wav", "2017/other_split.wav", "2017/other_year.wav"]
    for i, nme in enumerate(names):
        n = 6 * SEG + 100 * i if i != 1 else 4 * SEG + 10             # long_b has 4 whole segments: passed over
        wavfile.write(os.path.join(str(root), nme), FS if i != 0 else 2 * FS, (rng.randn(n, 2) * 2000).astype(np.int16))
    with open(os.path.join(str(root), "maestro-v3.0.0.csv"), "w") as f:
        f.write("canonical_composer,canonical_title,split,year,midi_filename,audio_filename,duration\n")
        f.write('"A, B",t,train,2017,x.midi,2017/long_a.wav,3.0\n')
        f.write("C,t,train,2017,x.midi,2017/long_b.wav,2.0\n")
        f.write("C,t,validation,2017,x.midi,2017/other_split.wav,3.0\n")
        f.write("C,t,train,2018,x.midi,2017/other_year.wav,3.0\n")
    return str(root)


def test_maestro_classes_filter_year_and_split_and_pass_over_short_files(maestro):
    from babe_amd.datasets import MaestroDataset, MaestroDataset_fs
    dargs = attr(path=maestro, years=[2004, 2017], load_len=SEG)
    ds = MaestroDataset(dargs, fs=FS, seg_len=SEG, seed=42)
    assert ds.train_samples == [os.path.join(maestro, "2017/long_a.wav"), os.path.join(maestro, "2017/long_b.wav")]
    assert MaestroDataset(attr(path=maestro, years=[2018]), fs=FS, seg_len=SEG).train_samples == [
        os.path.join(maestro, "2017/other_year.wav")]
    lengths = [6 * SEG, 4 * SEG + 10]
    want = expected_draws(lengths, 24, skip_short=True)
    assert {w[0] for w in want} == {0}
    files = [whole(p)[0] for p in ds.train_samples]
    it = iter(ds)
    for num, idx in want:
        seg = next(it)
        assert ds.last_draw == (num, idx) and np.array_equal(seg, files[num][idx:idx + SEG])
    fs_ds = MaestroDataset_fs(dargs, seed=42)
    assert fs_ds.seg_len == SEG
    it = iter(fs_ds)
    for num, idx in want[:10]:
        seg, sr = next(it)
        assert sr == 2 * FS and fs_ds.last_draw == (num, idx) and np.array_equal(seg, files[num][idx:idx + SEG])


def test_overfit_takes_the_first_file_from_second_10_with_crop_start_0(tmp_path):
    from scipy.io import wavfile
    from babe_amd.datasets import AudioFolderDataset, MaestroDataset, MaestroDataset_fs
    fs = 100
    x = (np.arange(70 * fs) % 30000).astype(np.int16)
    wavfile.write(str(tmp_path / "a.wav"), fs, x)
    with open(str(tmp_path / "maestro-v3.0.0.csv"), "w") as f:
        f.write("split,year,audio_filename\ntrain,2017,a.wav\n")
    want = (x[10 * fs:10 * fs + 500] / 32768.0).astype(np.float32)
    dargs = attr(path=str(tmp_path), years=[2017], load_len=500)
    for ds in (AudioFolderDataset(dargs, fs=fs, seg_len=500, overfit=True), MaestroDataset(dargs, fs=fs, seg_len=500, overfit=True)):
        it = iter(ds)
        assert len(ds.overfit_sample) == 50 * fs
        assert np.array_equal(next(it), want) and np.array_equal(next(it), want)
    seg, sr = next(iter(MaestroDataset_fs(dargs, overfit=True)))
    assert sr == fs and np.array_equal(seg, want)
    with pytest.raises(ValueError, match="wrong sampling rate"):
        MaestroDataset(dargs, fs=2 * fs, seg_len=500, overfit=True)


def test_state_saved_in_the_middle_of_a_group_continues_the_sequence(folder):
    import pickle
    from babe_amd.datasets import AudioFolderDataset
    d, _ = folder
    a = AudioFolderDataset(attr(path=d), fs=FS, seg_len=SEG, seed=7)
    it = iter(a)
    for _ in range(11):                                              # one whole group and three crops of the next
        next(it)
    state = pickle.loads(pickle.dumps(a.state_dict()))               # as it travels in a checkpoint
    assert state["pos"] == 3
    rest = [(next(it), a.last_draw) for _ in range(20)]
    b = AudioFolderDataset(attr(path=d), fs=FS, seg_len=SEG, seed=1234)
    b.load_state_dict(state)
    itb = iter(b)
    for seg, draw in rest:
        got = next(itb)
        assert b.last_draw == draw and np.array_equal(got, seg)
    assert len({draw[0] for _, draw in rest}) > 1                    # the 20 items cross into other groups and files


def test_collated_batches_keep_rates_per_row(maestro):
    import torch
    from babe_amd.datasets import MaestroDataset_fs
    ds = MaestroDataset_fs(attr(path=maestro, years=[2017], load_len=SEG))
    audio, fs = next(iter(torch.utils.data.DataLoader(ds, batch_size=3, num_workers=0)))
    assert audio.shape == (3, SEG) and audio.dtype == torch.float32 and fs.tolist() == [2 * FS] * 3
