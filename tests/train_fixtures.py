"""Synthetic audio files for the dataset, trainer and command-line tests: three short wavs written with scipy - 16-bit mono,
16-bit stereo and float32 mono - whose content is seeded noise over a few sines (any signal would do; it is never compared with
anything but itself)."""
import os

import numpy as np


def write_wavs(folder, fs=8000, seconds=(4.0, 3.5, 3.0), seed=0):
    """Write a_int16_mono.wav, b_int16_stereo.wav, c_float32_mono.wav into `folder`; returns their paths in sorted order."""
    from scipy.io import wavfile
    os.makedirs(folder, exist_ok=True)
    rng = np.random.RandomState(seed)

    def sig(n, ch=None):
        t = np.arange(n) / fs
        x = 0.05 * rng.randn(n, ch or 1)
        for f in (110.0, 440.0, 1760.0):
            x += 0.05 * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28))[:, None]
        return x if ch else x[:, 0]

    paths = []
    for name, sec, ch, dt in (("a_int16_mono", seconds[0], None, np.int16), ("b_int16_stereo", seconds[1], 2, np.int16),
                              ("c_float32_mono", seconds[2], None, np.float32)):
        x = sig(int(round(sec * fs)), ch)
        x = np.round(x * 32767).astype(np.int16) if dt == np.int16 else x.astype(np.float32)
        p = os.path.join(folder, name + ".wav")
        wavfile.write(p, fs, x)
        paths.append(p)
    return sorted(paths)
