"""The reference's Discriminator (model/discriminator/discriminator.py): MSD + MFD; the MPD stays out, as there."""
from ..generator.engine import NativeModule
from .common import check_length, device_input
from .mfd import MultiResolutionSTFTDiscriminator
from .msd import MelGANMultiScaleDiscriminator


class Discriminator(NativeModule):
    def __init__(self):
        super().__init__()
        self.msd = MelGANMultiScaleDiscriminator()
        self.mfd = MultiResolutionSTFTDiscriminator()

    def min_length(self):
        """Shortest input both discriminators accept (1680 samples with the default resolutions)."""
        return max(self.msd.min_length(), self.mfd.min_length())

    def forward(self, x):
        """x (B, 1, T) -> msd(x) + mfd(x): 6 lists of feature maps, the last map of each the score."""
        x = device_input(x, "x", 3)
        check_length(self, x.shape[-1])
        return self.msd(x) + self.mfd(x)
