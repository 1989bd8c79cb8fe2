"""The reference's Discriminator (model/discriminator/discriminator.py): MSD + MFD, and with ``use_mpd=True`` the
MPD the reference keeps one commented line away (discriminator.py:11, 16), registered first as there."""
from .. import _native
from .common import DiscriminatorModule, NotDifferentiable, checked_input
from .mfd import MultiResolutionSTFTDiscriminator
from .mpd import MultiPeriodDiscriminator
from .msd import MelGANMultiScaleDiscriminator


class Discriminator(NotDifferentiable, DiscriminatorModule):
    def __init__(self, use_mpd=False):
        super().__init__()
        self.use_mpd = bool(use_mpd)
        if self.use_mpd:
            self.mpd = MultiPeriodDiscriminator()
        self.msd = MelGANMultiScaleDiscriminator()
        self.mfd = MultiResolutionSTFTDiscriminator()

    @property
    def grad_precision(self):
        """The arithmetic of the MPD's weight gradients (``self.mpd.grad_precision``); "f32" without the MPD.  The MSD
        and MFD weight gradients have fp32 kernels only."""
        return self.mpd.grad_precision if self.use_mpd else "f32"

    @grad_precision.setter
    def grad_precision(self, value):
        if value not in _native.GRAD_PRECISIONS:
            raise ValueError(f"{type(self).__name__}.grad_precision: {value!r} ('f32' or 'bf16')")
        if self.use_mpd:
            self.mpd.grad_precision = value
        elif value != "f32":
            raise NotImplementedError("Discriminator(use_mpd=False).grad_precision = 'bf16': the MSD / MFD weight "
                                      "gradients have no bf16 kernels (only the MPD's do)")

    def min_length(self):
        """Shortest input every discriminator accepts (1680 samples with the default resolutions)."""
        need = max(self.msd.min_length(), self.mfd.min_length())
        return max(need, self.mpd.min_length()) if self.use_mpd else need

    def _forward(self, x, graph):
        """x (B, 1, T) -> msd(x) + mfd(x): 6 lists of feature maps, the last map of each the score; with ``use_mpd``
        mpd(x) + msd(x) + mfd(x): 11 lists, 71 maps.  On the graph (loss.generator_adversarial_terms) the MPD's nodes
        are built first: autograd adds the sub-discriminators' gradients into x in the reverse of the build order (a
        node built later runs earlier), the MFD's resolutions from the last to the first, then the MSD's scales from
        the coarsest, each through its pools, to scale 0, then the MPD's periods from 11 down to 2 -- the same order,
        hence the same bits, on every call.  Off the graph the MPD launches last, as it always has; the children
        check the channel count."""
        x = checked_input(self, x, 3, graph, mono=False)
        mpd = self.mpd._forward(x, graph) if self.use_mpd and graph else []
        outs = self.msd._forward(x, graph) + self.mfd._forward(x, graph)
        if self.use_mpd and not graph:
            mpd = self.mpd._forward(x, graph)
        return mpd + outs

    def _param_forward(self, x):
        """``_forward`` with every sub-discriminator on its parameters' graph (loss.discriminator_step_terms with
        stft_grad=True, and period_grad=True with ``use_mpd``): the lists in the order of ``_forward``.  The launch
        order is fixed: forward, the MPD's periods in the order of PERIODS (with ``use_mpd``), then the MSD's scales
        from scale 0, each behind its pool, then the MFD's resolutions in the order of the list; backward, autograd
        runs the nodes in the reverse of the build order (a node built later runs earlier) -- the MFD's resolutions
        from the last to the first, the MSD's scales from the coarsest to scale 0, the MPD's periods from 11 down to
        2 -- and inside a node the layers from the score downwards, per layer the weight and bias gradient, the
        weight-norm adjoint, then the data gradient for the layer below.  No two nodes share a parameter, so every
        ``.grad`` is written by one node: the same order, hence the same bits, on every call."""
        x = checked_input(self, x, 3, False, mono=False)
        mpd = self.mpd._param_forward(x) if self.use_mpd else []
        return mpd + self.msd._param_forward(x) + self.mfd._param_forward(x)
