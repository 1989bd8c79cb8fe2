"""The training data path of the reference (data/dataset.py): the utterances ``MODE=preprocess`` wrote, held in memory,
and fixed-length random crops of them in shuffled batches.

``load_data_to_buffer(audio_index, mel_index)`` reads the ``<name>.npy`` / ``<name>.mel.npy`` pairs the two index
files list (dataset.py:19-53); the mel is stored ``[80, T]`` and kept ``[T, 80]``, as dataset.py:38 transposes it.
``BatchIterator`` gives the crop of ``BufferDataset.__getitem__`` (dataset.py:63-75) -- the first frame uniform in
``[0, frames - fixed_length - 1]`` (``random.randint``'s closed range), the waveform slice ``start * hop`` to
``end * hop`` -- and the epochs of ``DataLoader(shuffle=True, drop_last=True)``, from ONE seeded generator, so that a
seed fixes the whole run.  Differences, on purpose: utterances too short for a crop are left out and counted in one
printed line (the reference raises inside ``random.randint``); batches are collated in this process (no DataLoader
workers: the buffer is in memory and a crop is a slice); the ``features_*.bin`` pickle cache and the sorting into
``batch_expand_size`` sub-batches by length (all crops have one length) are not reproduced.

Basis-MelGAN (``WeightDataset``, dataset.py:77-116): with ``weight_dir`` the items also carry the pre-computed target
weights ``weight [F_total, C]``, loaded from ``<weight_dir>/<basename of the audio path>`` and transposed; a crop
slices its rows ``start * r : end * r`` with ``r = hop_size // (L // 2)`` weight frames per mel frame, and the
iterator yields ``(mel, wav, weight)``.
"""
import os

import numpy as np
import torch

from . import hparams as hp


class MissingWeightFile(FileNotFoundError):
    """A target-weight file of Basis-MelGAN's dataset does not exist; the message names the path."""


def parse_path_file(path):
    with open(path, "r", encoding="utf-8") as f:
        return [line.rstrip("\n") for line in f if line.strip()]


def load_data_to_buffer(audio_index_path_file, mel_index_path_file, size=None, weight_dir=None):
    """-> [{"mel": float32 [T, 80], "wav": float32 [n]}] for the first ``size`` (default hparams.test_size, 0 = all)
    utterances of the index files; with ``weight_dir`` also "weight": float32 [F_total, C].  A missing weight file
    raises MissingWeightFile (a FileNotFoundError) that names the path."""
    audio_index = parse_path_file(audio_index_path_file)
    mel_index = parse_path_file(mel_index_path_file)
    if len(audio_index) != len(mel_index):
        raise ValueError(f"{audio_index_path_file} lists {len(audio_index)} waveforms, {mel_index_path_file} "
                         f"{len(mel_index)} mels")
    n = len(audio_index)
    size = hp.test_size if size is None else size
    if size != 0 and size < n:
        n = size
    buffer = []
    for i in range(n):
        mel = torch.from_numpy(np.ascontiguousarray(np.load(mel_index[i]).T, dtype=np.float32))
        wav = torch.from_numpy(np.ascontiguousarray(np.load(audio_index[i]), dtype=np.float32))
        item = {"mel": mel, "wav": wav}
        if weight_dir is not None:
            path = os.path.join(weight_dir, audio_index[i].split("/")[-1])
            if not os.path.isfile(path):
                raise MissingWeightFile(f"the target weights {path} of {audio_index[i]} do not exist")
            item["weight"] = torch.from_numpy(np.ascontiguousarray(np.load(path).T, dtype=np.float32))
        buffer.append(item)
    return buffer


def croppable(item, fixed_length, hop, weight_rate=None):
    """Can a crop of ``fixed_length`` frames be cut from this utterance (at every start the reference may draw)?"""
    frames = item["mel"].shape[0]
    if "weight" in item and item["weight"].shape[0] < (frames - 1) * weight_rate:
        return False
    return frames - fixed_length - 1 >= 0 and item["wav"].shape[0] >= (frames - 1) * hop


def crop(item, start, fixed_length, hop, weight_rate=None):
    """BufferDataset.__getitem__ at a given first frame -> (mel [fixed_length, 80], wav [fixed_length * hop]); for an
    item with target weights, WeightDataset's: (mel, wav, weight [fixed_length * weight_rate, C])."""
    end = start + fixed_length
    if "weight" in item:
        return (item["mel"][start:end, :], item["wav"][start * hop:end * hop],
                item["weight"][start * weight_rate:end * weight_rate, :])
    return item["mel"][start:end, :], item["wav"][start * hop:end * hop]


class BatchIterator:
    """``for mel, wav in BatchIterator(...).epoch()``: mel [B, fixed_length, 80], wav [B, fixed_length * hop], CPU fp32
    tensors.  ``len()`` is the number of batches of an epoch (``drop_last``).  When the items carry target weights
    (``basis_L``: the basis length L, required then) it yields ``(mel, wav, weight [B, fixed_length * r, C])``,
    ``r = hop // (L // 2)``.

    Data-parallel training (``rank``, ``world_size``): ``batch_size`` is per rank.  Every rank draws the same
    permutation and the same crop starts from the same seeded stream, for a global batch of ``batch_size * world_size``
    rows, and rank r yields the rows ``[r * batch_size, (r + 1) * batch_size)`` of it: the ranks' batches concatenated
    in rank order are, bit for bit, the single-process iterator's at batch size ``batch_size * world_size`` with the
    same seed.  ``len()`` is ``items // (batch_size * world_size)``."""

    def __init__(self, buffer, batch_size, fixed_length=None, hop=None, seed=0, name="train", basis_L=None, rank=0,
                 world_size=1):
        self.fixed_length = hp.fixed_length if fixed_length is None else int(fixed_length)
        self.hop = hp.hop_size if hop is None else int(hop)
        self.batch_size = int(batch_size)
        if self.batch_size < 1 or self.fixed_length < 1 or self.hop < 1:
            raise ValueError(f"batch_size {batch_size}, fixed_length {fixed_length} and hop {hop} must be positive")
        self.rank, self.world_size = int(rank), int(world_size)
        if self.world_size < 1 or not 0 <= self.rank < self.world_size:
            raise ValueError(f"rank {rank} of world_size {world_size}")
        self.weight_rate = None
        with_weight = sum("weight" in it for it in buffer)
        if with_weight not in (0, len(buffer)):
            raise ValueError(f"{with_weight} of {len(buffer)} {name} utterances carry target weights: all of them or none "
                             "must")
        if with_weight:
            if basis_L is None or int(basis_L) < 2 or self.hop % (int(basis_L) // 2):
                raise ValueError(f"items with target weights need basis_L, the basis length, whose half divides the hop "
                                 f"{self.hop}, got {basis_L}")
            self.weight_rate = self.hop // (int(basis_L) // 2)
        self.items = [it for it in buffer if croppable(it, self.fixed_length, self.hop, self.weight_rate)]
        self.skipped = len(buffer) - len(self.items)
        if self.skipped:
            print(f"data: {self.skipped} of {len(buffer)} {name} utterances are too short for a crop of "
                  f"{self.fixed_length} frames and are left out")
        self.rng = np.random.RandomState(seed)

    def __len__(self):
        return len(self.items) // (self.batch_size * self.world_size)

    def epoch(self):
        order = self.rng.permutation(len(self.items))
        rows = self.batch_size * self.world_size                 # the global batch; every rank draws all its starts
        mine = range(self.rank * self.batch_size, (self.rank + 1) * self.batch_size)
        for b in range(len(self)):
            parts = []
            for row, idx in enumerate(order[b * rows:(b + 1) * rows]):
                item = self.items[idx]
                start = int(self.rng.randint(0, item["mel"].shape[0] - self.fixed_length))   # high is exclusive
                if row in mine:
                    parts.append(crop(item, start, self.fixed_length, self.hop, self.weight_rate))
            yield tuple(torch.stack(column) for column in zip(*parts))
