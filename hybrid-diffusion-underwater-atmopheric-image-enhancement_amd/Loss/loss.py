"""Drop-in for the reference's ``Loss/loss.py:269-283``: ``MSSSIMLoss``, which there wraps ``kornia.losses.MS_SSIMLoss()`` with its
defaults -- the MS-SSIM + L1 mix of Zhao et al., "Loss Functions for Image Restoration with Neural Networks".  Here the loss and
its gradient with respect to the prediction are hand-written gfx950 kernels (``csrc/msssim.hip`` through
``autograd.msssim_l1_loss``); kornia is never imported.

The definition is the one written out in ``autograd.msssim_l1_loss``.  ``layout="kornia"`` (default) applies the 15 window / channel
combinations that kornia's grouped convolution forms (output map ``o`` reads colour channel ``o // 5`` with
``sigmas[o // 3]``: red sees only the two finest scales, blue only the two coarsest); ``layout="per_channel"`` is the published
form, every channel at every scale.  The kornia layout was written from memory of kornia's source: agreement with kornia itself
is unpinned; what the tests pin is the definition.

Use with the trainer: ``GaussianDiffusionTrainer(model, beta_1, beta_T, T, msssim_loss=MSSSIMLoss())``.
"""
from __future__ import annotations

import torch.nn as nn

__all__ = ["MSSSIMLoss"]


class MSSSIMLoss(nn.Module):
    """forward(input, target) -> scalar; ``input`` (the prediction) is differentiated, ``target`` is not."""

    def __init__(self, id: int = None, *, layout: str = "kornia", sigmas=(0.5, 1.0, 2.0, 4.0, 8.0), data_range: float = 1.0,
                 K=(0.01, 0.03), alpha: float = 0.025, compensation: float = 200.0, reduction: str = "mean"):
        super().__init__()
        from ..autograd import msssim_config
        self._id = id
        self.layout, self.sigmas, self.data_range, self.K = layout, tuple(float(s) for s in sigmas), float(data_range), tuple(K)
        self.alpha, self.compensation, self.reduction = float(alpha), float(compensation), reduction
        self._cfg = msssim_config(layout=layout, sigmas=self.sigmas, data_range=data_range, K=K, alpha=alpha,
                                  compensation=compensation, reduction=reduction)       # raises on unsupported values

    @property
    def name(self):
        return self.__class__.__name__

    @property
    def id(self):
        return self._id

    def forward(self, input, target):
        from ..autograd import msssim_l1_loss
        return msssim_l1_loss(input, target, config=self._cfg)
