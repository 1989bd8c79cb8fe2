"""The reference's discriminators (model/discriminator/), forward only, on the MI355X: ``MelGANDiscriminator`` and
``MelGANMultiScaleDiscriminator`` (msd.py), ``STFTDiscriminator`` and ``MultiResolutionSTFTDiscriminator`` (mfd.py),
``DiscriminatorP`` and ``MultiPeriodDiscriminator`` (mpd.py), and ``Discriminator`` (discriminator.py: MSD + MFD,
with ``use_mpd=True`` MPD + MSD + MFD).  Same constructor arguments, ``state_dict`` keys and nested
feature-map lists as the reference; every layer runs as a HIP launch (csrc/disc.hip for the grouped downsamples,
the average pool and the bins-major STFT magnitude, csrc/mpd.hip for the strided period convs, fv_conv1d_fused for
the dense convs).  There is no CPU path and
no autograd.  The scores of the reference's training loop are ``fastvocoder_amd.loss.discriminator_terms``."""
from .discriminator import Discriminator
from .mfd import MultiResolutionSTFTDiscriminator, STFTDiscriminator
from .mpd import DiscriminatorP, MultiPeriodDiscriminator
from .msd import MelGANDiscriminator, MelGANMultiScaleDiscriminator

__all__ = ["Discriminator", "DiscriminatorP", "MelGANDiscriminator", "MelGANMultiScaleDiscriminator",
           "MultiPeriodDiscriminator", "MultiResolutionSTFTDiscriminator", "STFTDiscriminator"]
