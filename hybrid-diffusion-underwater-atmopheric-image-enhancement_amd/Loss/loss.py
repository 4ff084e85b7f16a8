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

``PerceptualLoss_vgg`` (reference ``:159-241``) and ``CharbonnierLoss`` (``:286-300``) are here too, on ``hdiff_amd.perceptual``: the VGG
trunk's convs are the package's conv kernels, ReLU / pooling / the L1 mean / the Charbonnier map are ``csrc/perceptual.hip``.  No
pretrained weights ship and none are fetched: the caller hands ``PerceptualLoss_vgg`` a torchvision state dict (``weights=``); without
one the trunk is randomly initialised and says so.  Deliberate deviations: the target's features are taken under ``no_grad`` (the
target is a constant, as for ``MSSSIMLoss``); the ``*_bn``, ``squeeze`` and ``alex`` trunks are not provided.  The Charbonnier formula
``sqrt(d^2 + 1) - 1`` was written from memory of kornia's ``charbonnier_loss``: agreement with kornia itself is unpinned.  Pass either
to the trainer through ``extra_losses=[(name, weight, loss), ...]``.

``PerceptualLoss_dino`` (reference ``:244-266``) is the term the reference trains with: smooth-L1 over every hooked module output of a
frozen DINOv2 ViT, on ``hdiff_amd.dino`` (``csrc/dino.hip`` plus the package's dense-layer and attention kernels).  As for the VGG loss
no weights ship: ``weights=`` takes the hub checkpoint's state dict.  The tap list, the position-embedding rule and the
initialisation were written from memory of dinov2: agreement with the hub model is unpinned.  The trainer builds it itself with
``GaussianDiffusionTrainer(..., dino_loss="native", dino_weights=...)``.
"""
from __future__ import annotations

import warnings

import torch
import torch.nn as nn

__all__ = ["MSSSIMLoss", "PerceptualLoss_vgg", "PerceptualLoss_dino", "CharbonnierLoss"]

_UNSUPPORTED = ("Unsupported perceptual model type. Choose from ['vgg11', 'vgg11_bn', 'vgg13', 'vgg13_bn', 'vgg16', 'vgg16_bn', "
                "'vgg19', 'vgg19_bn', 'squeeze', 'alex']")
_NOT_PROVIDED = ("vgg11_bn", "vgg13_bn", "vgg16_bn", "vgg19_bn", "squeeze", "alex")


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


class PerceptualLoss_vgg(nn.Module):
    """forward(x, y) -> 0-dim tensor: the sum over the tapped layers of ``mean |feat(x) - feat(y)|`` (reference ``:217-233``; no input
    normalisation, it is commented out there).  ``x`` is differentiated; ``y``'s features are taken under ``no_grad``.

    ``weights``: a torchvision state dict of ``model`` (or the path of a file ``torch.load`` reads one from).  Without it the trunk
    keeps its random initialisation and one ``RuntimeWarning`` says so.  ``.perceptual`` is the ``hdiff_amd.perceptual.VGGFeatures``;
    move the loss to the device of the images (``.to(device)``) like any module."""

    def __init__(self, id: int = None, model='vgg16', layer_indices=None, *, weights=None):
        super().__init__()
        from ..perceptual import VGG_CFGS, VGGFeatures
        self._id = id
        if model in _NOT_PROVIDED:
            raise ValueError(f"perceptual model '{model}' is not provided: the HIP path has the plain VGG trunks {sorted(VGG_CFGS)} "
                             "(no batch norm, no SqueezeNet, no AlexNet)")
        if model not in VGG_CFGS:
            raise ValueError(_UNSUPPORTED)
        self.perceptual = VGGFeatures(model)
        self._model = model
        if weights is None:
            warnings.warn(f"PerceptualLoss_vgg: no weights were given; the {model} trunk is randomly initialised (pass weights=, a "
                          "torchvision state dict or its path)", RuntimeWarning, stacklevel=2)
        else:
            if not isinstance(weights, dict):
                weights = torch.load(weights, map_location="cpu")
            self.perceptual.load_torchvision(weights)
        self.layer_indices = {
            'squeeze':  [3, 7, 12],
            'vgg11':    [3, 8, 15, 22],
            'vgg11_bn': [3, 8, 15, 22],
            'vgg13':    [3, 8, 15, 22],
            'vgg13_bn': [3, 8, 15, 22],
            'vgg16':    [3, 8, 15, 22],
            'vgg16_bn': [3, 8, 15, 22],
            'vgg19':    [3, 8, 17, 26, 35],
            'vgg19_bn': [3, 8, 17, 26, 35],
            'alex':     [3, 6, 8, 10, 12],
        }
        if layer_indices is not None:
            self.layer_indices[model] = layer_indices

    @property
    def name(self):
        return self.__class__.__name__ + '_' + self._model

    @property
    def id(self):
        return self._id

    def extract_features(self, x):
        return self.perceptual(x, self.layer_indices[self._model])

    def forward(self, x, y):
        from ..perceptual import l1_mean
        x_features = self.extract_features(x)
        with torch.no_grad():
            y_features = self.extract_features(y)
        loss = None
        for xf, yf in zip(x_features, y_features):
            term = l1_mean(xf, yf).double()          # the handful of per-layer means are added in double and rounded once
            loss = term if loss is None else loss + term
        if loss is not None:
            loss = loss.float()
        if loss is None:
            raise RuntimeError(f"PerceptualLoss_vgg: none of the layer indices {self.layer_indices[self._model]} is a layer of "
                               f"{self._model}")
        return loss


class PerceptualLoss_dino(nn.Module):
    """forward(input, target) -> 0-dim fp32 tensor: the sum over the hooked modules of
    ``smooth_l1_loss(feature(input), feature(target), 'mean')`` (reference ``:244-266``; ``layers=None`` hooks every module, which is
    what the trainer constructs).  ``input`` is differentiated; ``target``'s features are taken without a graph.  The images go to the
    trunk as they are: no normalisation and no rescaling (the reference hands it ``y_0_pred / 255`` and a ``[-1, 1]`` target), 2
    pixels come off every edge, and ``H - 4`` / ``W - 4`` must be multiples of 14.

    ``weights``: the hub checkpoint's state dict of ``model`` (or the path of a file ``torch.load`` reads one from).  Without it the
    trunk keeps its random initialisation and one ``RuntimeWarning`` says so.  ``.perceptual`` is the ``hdiff_amd.dino.DinoV2Features``,
    ``.taps`` the ``(module names, tensor, multiplicity)`` list in use, ``.last_per_image`` the ``(B,)`` shares of the last call.  The
    attention probabilities (``attn.attn_drop``) are not hooked (``hdiff_amd.dino`` says why).  ``normalize_inputs=True`` is not
    provided; ``version='dino'``, ``dinov2_vitg14`` and the ``_reg`` models raise ``ValueError``.  ``dense``: ``"conv"`` (default) or
    ``"tokens"``, the trunk's dense-layer route (``hdiff_amd.dino.dense_route``); with ``trunk=`` the trunk's own choice stands and the
    two must not disagree."""

    def __init__(self, model="dinov2_vits14", version="dinov2", layers=None, normalize_inputs=False, *, weights=None, trunk=None,
                 dense=None):
        super().__init__()
        from ..dino import DinoV2Features, check_model_name, select_taps
        if normalize_inputs:
            raise NotImplementedError("PerceptualLoss_dino: normalize_inputs=True is not provided (the trainer never sets it; the "
                                      "images go to the trunk as they are)")
        if trunk is None:
            check_model_name(model, version)
            trunk = DinoV2Features(model, dense="conv" if dense is None else dense)
        elif not isinstance(trunk, DinoV2Features):
            raise TypeError("PerceptualLoss_dino: trunk= must be a hdiff_amd.dino.DinoV2Features")
        elif dense is not None and dense != trunk.dense:
            raise ValueError(f"PerceptualLoss_dino: dense={dense!r} but the trunk was built with dense={trunk.dense!r}")
        self.perceptual = trunk
        self._model, self.version, self.layers = model, version, layers
        self.taps = select_taps(trunk.depth, layers)
        self.last_per_image = None
        if weights is not None:
            if not isinstance(weights, dict):
                weights = torch.load(weights, map_location="cpu")
            self.perceptual.load_dinov2(weights)

    @property
    def name(self):
        return self.__class__.__name__ + '_' + str(self._model)

    def forward(self, input, target):
        from ..dino import dino_perceptual
        loss, self.last_per_image = dino_perceptual(self.perceptual, input, target, self.taps, return_per_image=True)
        return loss


class CharbonnierLoss(nn.Module):
    """forward(input, target) -> ``sqrt((input - target)^2 + 1) - 1`` (reference ``:286-300``, kornia's ``charbonnier_loss`` with its
    default ``reduction='none'``: an elementwise map); ``reduction='mean'`` / ``'sum'`` reduce it in a fixed order.  ``input`` is
    differentiated, ``target`` is not."""

    def __init__(self, id: int = None, *, reduction: str = 'none'):
        super().__init__()
        if reduction not in ("none", "mean", "sum"):
            raise ValueError(f"Invalid reduction mode: {reduction}. Expected one of 'none', 'mean', 'sum'.")
        self._id = id
        self.reduction = reduction

    @property
    def name(self):
        return self.__class__.__name__

    @property
    def id(self):
        return self._id

    def forward(self, input, target):
        from ..perceptual import charbonnier
        return charbonnier(input, target, self.reduction)
