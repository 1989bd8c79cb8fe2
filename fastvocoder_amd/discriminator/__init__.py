"""The reference's discriminators (model/discriminator/), forward only, on the MI355X: ``MelGANDiscriminator`` and
``MelGANMultiScaleDiscriminator`` (msd.py), ``STFTDiscriminator`` and ``MultiResolutionSTFTDiscriminator`` (mfd.py),
and ``Discriminator`` (discriminator.py: MSD + MFD).  Same constructor arguments, ``state_dict`` keys and nested
feature-map lists as the reference; every layer runs as a HIP launch (csrc/disc.hip for the grouped downsamples,
the average pool and the bins-major STFT magnitude, fv_conv1d_fused for the dense convs).  There is no CPU path and
no autograd.  The scores of the reference's training loop are ``fastvocoder_amd.loss.discriminator_terms``."""
from .discriminator import Discriminator
from .mfd import MultiResolutionSTFTDiscriminator, STFTDiscriminator
from .msd import MelGANDiscriminator, MelGANMultiScaleDiscriminator

__all__ = ["Discriminator", "MelGANDiscriminator", "MelGANMultiScaleDiscriminator", "MultiResolutionSTFTDiscriminator",
           "STFTDiscriminator"]
