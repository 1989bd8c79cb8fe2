"""``MODE=preprocess``: the reference's dataset preparation (bin/preprocess.py) on the MI355X.
Same flags, same files (``<name>.mel.npy`` [80, T] float64 and ``<name>.npy``, the float32
waveform, under --save_path), the same printed ``min length of mel spectrogram is N.`` line and
the same shuffled train / valid / eval index files.  The wavs are processed one after another in
this process, each mel in one launch on the GPU (audio.melspectrogram), instead of the reference's
pool of cpu_count() // 2 librosa workers.

``--resample`` (off by default; not a flag of the reference, whose ``librosa.load`` always resamples): a wav at another
rate than ``hparams.sample_rate`` is converted on the GPU (audio.resample) instead of being reported and left out; the
resampled waveform stays on the device for the mel, and both come back to the host once.
"""
import argparse
import os
import random

import numpy as np
import torch

from .. import audio
from .. import hparams as hp


def preprocess(data_path_file, save_path, resample=False):
    """Mel and waveform files for every wav listed in ``data_path_file`` -> (audio_index, mel_index, lengths).
    A wav that fails is reported and left out of the indices (the reference's sequential path); without ``resample``
    that includes every wav at another rate than hparams.sample_rate."""
    os.makedirs(save_path, exist_ok=True)
    audio_index, mel_index, lengths = [], [], []
    with open(data_path_file, "r") as f:
        lines = [line.rstrip("\n") for line in f]
    for wav_filepath in lines:
        if not wav_filepath:
            continue
        try:
            wav_filename = wav_filepath.split("/")[-1]
            mel_filepath = os.path.join(save_path, f"{wav_filename}.mel.npy")
            new_wav_filepath = os.path.join(save_path, f"{wav_filename}.npy")
            y = audio.load_wav(wav_filepath, sample_rate=hp.sample_rate, encode=False, resample=resample,
                               keep_on_device=resample)
            if torch.is_tensor(y):      # resampled: the mel from the device tensor, then one copy of each to the host
                mel = audio.melspectrogram(y)[0].cpu().numpy()
                y = y.cpu().numpy()
            else:
                mel = audio.melspectrogram(y)
            np.save(mel_filepath, mel.astype(np.float64))
            np.save(new_wav_filepath, y)
            audio_index.append(new_wav_filepath)
            mel_index.append(mel_filepath)
            lengths.append(mel.shape[1])
        except Exception as e:
            print(f"ERROR: {wav_filepath}: {e}")
    if lengths:
        print(f"min length of mel spectrogram is {min(lengths)}.")
    return audio_index, mel_index, lengths


def write_file(audio_index, mel_index, index_list, file_name, audio_index_path, mel_index_path):
    with open(os.path.join(audio_index_path, file_name), "w", encoding="utf-8") as f:
        for index in index_list:
            f.write(audio_index[index] + "\n")
    with open(os.path.join(mel_index_path, file_name), "w", encoding="utf-8") as f:
        for index in index_list:
            f.write(mel_index[index] + "\n")


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--data_path', type=str, default=os.path.join("dataset", "ljspeech.txt"))
    parser.add_argument('--save_path', type=str, default=os.path.join("dataset", "processed"))
    parser.add_argument('--audio_index_path', type=str, default=os.path.join("dataset", "audio"))
    parser.add_argument('--mel_index_path', type=str, default=os.path.join("dataset", "mel"))
    parser.add_argument('--resample', action='store_true',
                        help="convert wavs at another rate than hparams.sample_rate on the GPU instead of skipping them")
    return parser


def run_preprocess(argv=None):
    args = build_parser().parse_args(argv)
    audio_index, mel_index, _ = preprocess(args.data_path, args.save_path, resample=args.resample)

    os.makedirs(args.audio_index_path, exist_ok=True)
    os.makedirs(args.mel_index_path, exist_ok=True)
    total = hp.train_size + hp.valid_size + hp.eval_size
    assert len(audio_index) >= total, \
        f"{len(audio_index)} utterances, hparams asks for train + valid + eval = {total}"
    index_list = list(range(total))
    random.shuffle(index_list)
    index_list_train = index_list[0:hp.train_size]
    index_list_valid = index_list[hp.train_size:hp.train_size + hp.valid_size]
    index_list_eval = index_list[hp.train_size + hp.valid_size:total]
    write_file(audio_index, mel_index, index_list_train, "train", args.audio_index_path, args.mel_index_path)
    write_file(audio_index, mel_index, index_list_valid, "valid", args.audio_index_path, args.mel_index_path)
    write_file(audio_index, mel_index, index_list_eval, "eval", args.audio_index_path, args.mel_index_path)


if __name__ == "__main__":
    run_preprocess()
