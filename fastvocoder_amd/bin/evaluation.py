"""``MODE=evaluation``: the reference's bin/evaluation.py carried to the end.  It loads the eval utterances that
MODE=preprocess wrote (``<name>.npy`` waveforms and ``<name>.mel.npy`` mels, listed by the index files),
synthesizes each mel with the checkpoint, crops estimate and target to their common length and scores them with
the multi-resolution STFT distance of the reference's training loss (loss.MultiResolutionSTFTLoss, default
resolutions), one utterance at a time, on the GPU.  Output, one line per utterance, then the mean:

    eval <i> <audio path> samples=<n> sc=<spectral convergence> mag=<log-STFT-magnitude L1>
    eval mean utterances=<count> sc=<mean sc> mag=<mean mag>

(numbers printed with ``%.8e``; sc and mag are each averaged over the three resolutions).

With ``--discriminator`` the checkpoint's ``'discriminator'`` entry (a training checkpoint of the reference holds it
beside ``'model'``, bin/train.py:235-247) is loaded into fastvocoder_amd.discriminator.Discriminator (with
``use_mpd=True`` when the entry carries ``mpd.`` keys: a checkpoint trained with the reference's multi-period
discriminator enabled, discriminator.py:11, 16), and every utterance is also scored with the adversarial / feature-map / discriminator terms of the reference's training loop
(loss.discriminator_terms), estimate against target:

    eval-d <i> adv=<adversarial> fm=<feature map> real=<real> fake=<fake> d=<real + fake>
    eval-d mean utterances=<count> adv=<mean adv> fm=<mean fm> d=<mean d>

each after the corresponding ``eval`` line.  Without the flag the output is unchanged.

With ``--griffin_lim`` every utterance's mel is also inverted by Griffin-Lim (audio.inv_mel_spectrogram, the initial
phase seeded with ``--gl_seed``, default 0) and scored against the same target with the same distance -- the floor to
read the vocoder's distances against:

    eval-gl <i> samples=<n> sc=<spectral convergence> mag=<log-STFT-magnitude L1>
    eval-gl mean utterances=<count> sc=<mean sc> mag=<mean mag>

each after the utterance's ``eval`` (and ``eval-d``) line.  Without the flag the output is unchanged.
"""
import argparse
import os

import numpy as np
import torch

from ..audio import inv_mel_spectrogram
from ..loss import MultiResolutionSTFTLoss, discriminator_terms
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


def score(synthesizer, loss, wav, mel, discriminator=None):
    """(samples, sc, mag) of one utterance: synthesize mel [80, T], crop both to the common length; with a
    discriminator also its five terms (a dict) as a fourth item."""
    est = synthesizer.synthesize(np.asarray(mel).T)[0]
    target = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).to(est.device)
    n = min(est.shape[0], target.shape[0])
    with torch.no_grad():
        sc, mag = loss.per_utterance(est[None, :n], target[None, :n])[0].tolist()
    if discriminator is None:
        return n, sc, mag
    return n, sc, mag, score_discriminator(discriminator, est[:n].contiguous(), target[:n].contiguous())


def score_griffin_lim(loss, wav, mel, device, seed):
    """(samples, sc, mag) of Griffin-Lim of mel [80, T] against the target, cropped to the common length."""
    est = inv_mel_spectrogram(torch.as_tensor(np.asarray(mel), dtype=torch.float32).to(device), seed=seed)
    target = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).to(device)
    n = min(est.shape[0], target.shape[0])
    with torch.no_grad():
        sc, mag = loss.per_utterance(est[None, :n].contiguous(), target[None, :n].contiguous())[0].tolist()
    return n, sc, mag


def discriminator_uses_mpd(state_dict):
    """Does a checkpoint's 'discriminator' entry hold the multi-period discriminator (``mpd.`` keys)?"""
    return any(k.startswith("mpd.") for k in state_dict)


def load_discriminator(synthesizer):
    """The checkpoint's discriminator on the synthesizer's device, or a clear exit when the checkpoint has none."""
    from ..discriminator import Discriminator
    sd = synthesizer.checkpoint.get("discriminator") if isinstance(synthesizer.checkpoint, dict) else None
    if sd is None:
        raise SystemExit("evaluation: --discriminator needs a checkpoint with a 'discriminator' entry (a training "
                         "checkpoint of the reference); this one has none")
    d = Discriminator(use_mpd=discriminator_uses_mpd(sd)).to(synthesizer.device)
    d.load_state_dict(sd)
    return d.eval()


def score_discriminator(discriminator, est, target):
    """The five discriminator terms of one (estimate, target) pair of [n] device waveforms, as floats."""
    with torch.no_grad():
        terms = discriminator_terms(discriminator(est[None, None]), discriminator(target[None, None]))
    return {k: float(v) for k, v in terms.items()}


def run_evaluation(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('--checkpoint_path', type=str)
    parser.add_argument('--audio_index_path', type=str, default=os.path.join("dataset", "audio", "eval"))
    parser.add_argument('--mel_index_path', type=str, default=os.path.join("dataset", "mel", "eval"))
    parser.add_argument('--config', type=str, help="path to model configuration file")
    parser.add_argument('--model_name', type=str, help="melgan, hifigan, multiband-hifigan and basis-melgan.")
    parser.add_argument('--num', type=int, default=6, help="score utterances 0..num-1 of the index (default 6)")
    parser.add_argument('--discriminator', action='store_true',
                        help="also print the adversarial / feature-map / discriminator scores of the checkpoint's "
                             "'discriminator'")
    parser.add_argument('--griffin_lim', action='store_true',
                        help="also score Griffin-Lim of each mel against the same target (eval-gl lines)")
    parser.add_argument('--gl_seed', type=int, default=0, help="seed of the Griffin-Lim initial phase (default 0)")
    args = parser.parse_args(argv)
    if args.num < 1:
        raise SystemExit("evaluation: --num must be at least 1")

    synthesizer = Synthesizer(args.checkpoint_path, args.config, args.model_name)
    audio_list, mel_list, names = load_data(args.audio_index_path, args.mel_index_path, list(range(args.num)))
    loss = MultiResolutionSTFTLoss().to(synthesizer.device)
    disc = load_discriminator(synthesizer) if args.discriminator else None
    rows, drows, grows = [], [], []
    for i, (wav, mel, name) in enumerate(zip(audio_list, mel_list, names)):
        n, sc, mag, *d = score(synthesizer, loss, wav, mel, disc)
        rows.append((sc, mag))
        print(f"eval {i} {name} samples={n} sc={sc:.8e} mag={mag:.8e}")
        if d:
            t = d[0]
            drows.append((t["adversarial"], t["feature_map"], t["discriminator"]))
            print(f"eval-d {i} adv={t['adversarial']:.8e} fm={t['feature_map']:.8e} real={t['real']:.8e} "
                  f"fake={t['fake']:.8e} d={t['discriminator']:.8e}")
        if args.griffin_lim:
            gn, gsc, gmag = score_griffin_lim(loss, wav, mel, synthesizer.device, args.gl_seed)
            grows.append((gsc, gmag))
            print(f"eval-gl {i} samples={gn} sc={gsc:.8e} mag={gmag:.8e}")
    sc_mean, mag_mean = (float(np.mean(c)) for c in zip(*rows))
    print(f"eval mean utterances={len(rows)} sc={sc_mean:.8e} mag={mag_mean:.8e}")
    if drows:
        adv, fm, d = (float(np.mean(c)) for c in zip(*drows))
        print(f"eval-d mean utterances={len(drows)} adv={adv:.8e} fm={fm:.8e} d={d:.8e}")
    if grows:
        gsc, gmag = (float(np.mean(c)) for c in zip(*grows))
        print(f"eval-gl mean utterances={len(grows)} sc={gsc:.8e} mag={gmag:.8e}")
    return rows


if __name__ == "__main__":
    run_evaluation()
