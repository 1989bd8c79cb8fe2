"""``MODE=evaluation``: the reference's bin/evaluation.py carried to the end.  It loads the eval utterances that
MODE=preprocess wrote (``<name>.npy`` waveforms and ``<name>.mel.npy`` mels, listed by the index files),
synthesizes each mel with the checkpoint, crops estimate and target to their common length and scores them with
the multi-resolution STFT distance of the reference's training loss (loss.MultiResolutionSTFTLoss, default
resolutions), one utterance at a time, on the GPU.  Output, one line per utterance, then the mean:

    eval <i> <audio path> samples=<n> sc=<spectral convergence> mag=<log-STFT-magnitude L1>
    eval mean utterances=<count> sc=<mean sc> mag=<mean mag>

(numbers printed with ``%.8e``; sc and mag are each averaged over the three resolutions).
"""
import argparse
import os

import numpy as np
import torch

from ..loss import MultiResolutionSTFTLoss
from .synthesize import Synthesizer


def parse_path_file(path):
    with open(path, "r") as f:
        return [line.rstrip("\n") for line in f if line.strip()]


def load_data(audio_index_path, mel_index_path, index_list):
    audio_index = parse_path_file(audio_index_path)
    mel_index = parse_path_file(mel_index_path)
    if max(index_list) >= min(len(audio_index), len(mel_index)):
        raise SystemExit(f"evaluation: asked for utterance {max(index_list)}, the index files list "
                         f"{len(audio_index)} waveforms and {len(mel_index)} mels")
    audio_list, mel_list = [], []
    for index in index_list:
        audio_list.append(np.load(audio_index[index]))
        mel_list.append(torch.from_numpy(np.load(mel_index[index])))
    return audio_list, mel_list, [audio_index[i] for i in index_list]


def score(synthesizer, loss, wav, mel):
    """(samples, sc, mag) of one utterance: synthesize mel [80, T], crop both to the common length."""
    est = synthesizer.synthesize(np.asarray(mel).T)[0]
    target = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).to(est.device)
    n = min(est.shape[0], target.shape[0])
    with torch.no_grad():
        sc, mag = loss.per_utterance(est[None, :n], target[None, :n])[0].tolist()
    return n, sc, mag


def run_evaluation(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--checkpoint_path', type=str)
    parser.add_argument('--audio_index_path', type=str, default=os.path.join("dataset", "audio", "eval"))
    parser.add_argument('--mel_index_path', type=str, default=os.path.join("dataset", "mel", "eval"))
    parser.add_argument('--config', type=str, help="path to model configuration file")
    parser.add_argument('--model_name', type=str, help="melgan, hifigan, multiband-hifigan and basis-melgan.")
    parser.add_argument('--num', type=int, default=6, help="score utterances 0..num-1 of the index (default 6)")
    args = parser.parse_args(argv)
    if args.num < 1:
        raise SystemExit("evaluation: --num must be at least 1")

    synthesizer = Synthesizer(args.checkpoint_path, args.config, args.model_name)
    audio_list, mel_list, names = load_data(args.audio_index_path, args.mel_index_path, list(range(args.num)))
    loss = MultiResolutionSTFTLoss().to(synthesizer.device)
    rows = []
    for i, (wav, mel, name) in enumerate(zip(audio_list, mel_list, names)):
        n, sc, mag = score(synthesizer, loss, wav, mel)
        rows.append((sc, mag))
        print(f"eval {i} {name} samples={n} sc={sc:.8e} mag={mag:.8e}")
    sc_mean, mag_mean = (float(np.mean(c)) for c in zip(*rows))
    print(f"eval mean utterances={len(rows)} sc={sc_mean:.8e} mag={mag_mean:.8e}")
    return rows


if __name__ == "__main__":
    run_evaluation()
