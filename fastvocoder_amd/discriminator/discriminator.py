"""The reference's Discriminator (model/discriminator/discriminator.py): MSD + MFD, and with ``use_mpd=True`` the
MPD the reference keeps one commented line away (discriminator.py:11, 16), registered first as there."""
from ..generator.engine import NativeModule
from .common import NotDifferentiable, check_length, device_input
from .mfd import MultiResolutionSTFTDiscriminator
from .mpd import MultiPeriodDiscriminator
from .msd import MelGANMultiScaleDiscriminator


class Discriminator(NotDifferentiable, NativeModule):
    def __init__(self, use_mpd=False):
        super().__init__()
        self.use_mpd = bool(use_mpd)
        if self.use_mpd:
            self.mpd = MultiPeriodDiscriminator()
        self.msd = MelGANMultiScaleDiscriminator()
        self.mfd = MultiResolutionSTFTDiscriminator()

    def min_length(self):
        """Shortest input every discriminator accepts (1680 samples with the default resolutions)."""
        need = max(self.msd.min_length(), self.mfd.min_length())
        return max(need, self.mpd.min_length()) if self.use_mpd else need

    def forward(self, x):
        """x (B, 1, T) -> msd(x) + mfd(x): 6 lists of feature maps, the last map of each the score; with ``use_mpd``
        mpd(x) + msd(x) + mfd(x): 11 lists, 71 maps."""
        x = device_input(x, "x", 3)
        check_length(self, x.shape[-1])
        outs = self.msd(x) + self.mfd(x)
        return self.mpd(x) + outs if self.use_mpd else outs

    def _graph_forward(self, x):
        """``forward`` on the graph of x (loss.generator_adversarial_terms): msd then mfd, as ``forward``, with
        ``use_mpd`` mpd first.  Autograd adds the sub-discriminators' gradients into x in the reverse of that order
        (a node built later runs earlier): the MFD's resolutions from the last to the first, then the MSD's scales
        from the coarsest, each through its pools, to scale 0, then the MPD's periods from 11 down to 2 -- the same
        order, hence the same bits, on every call."""
        x = device_input(x, "x", 3, differentiable=True)
        check_length(self, x.shape[-1])
        mpd = self.mpd._graph_forward(x) if self.use_mpd else []
        return mpd + self.msd._graph_forward(x) + self.mfd._graph_forward(x)
