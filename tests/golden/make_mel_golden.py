"""Writes tests/golden/mel_demo.npz: the int16 samples of the reference's demo wav
resource/demo/0.hifigan.light.705000.wav (24 kHz, 585 x 240 samples) and the mel behind it,
resource/test.mel.npy ([80, 585], stored as float32).  Run once against a checkout of the reference:

    python tests/golden/make_mel_golden.py /path/to/FastVocoder

The fixture is data only; no test reads the reference tree."""
import os
import sys

import numpy as np
import scipy.io.wavfile


def main(ref_root):
    sr, wav = scipy.io.wavfile.read(os.path.join(ref_root, "resource", "demo", "0.hifigan.light.705000.wav"))
    mel = np.load(os.path.join(ref_root, "resource", "test.mel.npy"))
    assert sr == 24000 and wav.dtype == np.int16 and wav.ndim == 1 and wav.shape[0] == mel.shape[1] * 240, \
        (sr, wav.dtype, wav.shape, mel.shape)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mel_demo.npz")
    np.savez_compressed(out, wav=wav, mel=mel.astype(np.float32), sample_rate=np.int32(sr))
    print(f"wrote {out}: wav {wav.shape} int16, mel {mel.shape} float32, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
