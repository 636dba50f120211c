"""Masked soft Dice, Tversky, focal and Dice + CE losses over the fused kernels msk_region_loss_fwd / msk_region_loss_bwd
(medicalseg_amd/csrc/msk_loss_region.hip; tests/region_reference.py states the formulas).

Unlike ``DiceLoss`` (the reference's V-Net Dice, which sums p^2 over every voxel) all of them honour ``ignore_index`` in every
sum, so ``RandomPatchCrop3D(label_pad=255)`` really keeps the padding out of the loss.  Unlike ``CrossEntropyLoss`` the CE term
uses the logits as given and ones as class weights unless ``weight`` lists others.

With several ranks the batch-Dice sums (``batch_dice=True``) are those of each rank's own batch: no collective is added."""
import numpy as np

from ... import nn
from ...cvlibs import manager
from .fused import REGION_ACTIVATIONS, REGION_DICE, REGION_TVERSKY, RegionNode, Scalar, node_for, per_channel_dice
from .loss_utils import device_weights


def _check_gamma(gamma):
    gamma = float(gamma)
    if not (gamma == 0.0 or gamma >= 1.0):   # (1 - u)^(gamma - 1) in the derivative is inf * 0 at u -> 1 for gamma in (0, 1)
        raise ValueError("gamma must be 0 or >= 1, but it is {}".format(gamma))
    return gamma


class _RegionLoss(nn.Layer):
    """Settings, their checks and the node shared by the four losses."""

    def __init__(self, activation='softmax', batch_dice=True, do_bg=False, smooth=1e-5, squared_pred=False, ignore_index=255,
                 mode=REGION_DICE, alpha=0.0, beta=0.0, focal_on=False, gamma=0.0, weight=None):
        super().__init__()
        if activation not in REGION_ACTIVATIONS:
            raise ValueError("activation must be 'softmax' or 'sigmoid', but it is {!r}".format(activation))
        if float(smooth) < 0:
            raise ValueError("smooth must be >= 0, but it is {}".format(smooth))
        if mode == REGION_TVERSKY and squared_pred:
            raise ValueError("TverskyLoss does not take squared_pred=True")
        if mode == REGION_TVERSKY and (float(alpha) < 0 or float(beta) < 0):
            raise ValueError("alpha and beta must be >= 0, but they are {} and {}".format(alpha, beta))
        if focal_on and activation != 'softmax':
            raise ValueError("the focal / cross-entropy term needs activation='softmax'")
        self.activation, self.batch_dice, self.do_bg = activation, bool(batch_dice), bool(do_bg)
        self.smooth, self.squared_pred, self.ignore_index = float(smooth), bool(squared_pred), int(ignore_index)
        self.alpha, self.beta, self.gamma = float(alpha), float(beta), _check_gamma(gamma)
        self._mode, self._focal_on = mode, bool(focal_on)
        self.weight = None if weight is None else np.asarray(weight, dtype=np.float32).reshape(-1)
        self._weight_dev = None

    def _node(self, logits, labels):
        if not 1 <= logits.c <= 64:
            raise ValueError("the logits have %d classes; 1 .. 64 are supported" % logits.c)
        if self.activation == 'softmax' and logits.c == 1:
            raise ValueError("activation='softmax' needs at least 2 classes (use activation='sigmoid' for a one-channel head)")
        weight_ptr = None
        if self.weight is not None:
            if self.weight.size != logits.c:
                raise ValueError("%s weight has %d entries for %d classes" % (type(self).__name__, self.weight.size, logits.c))
            self._weight_dev = device_weights(logits.dev, self.weight, self._weight_dev)
            weight_ptr = self._weight_dev[1]
        settings = (self.ignore_index, REGION_ACTIVATIONS[self.activation], int(self.squared_pred), int(self.batch_dice),
                    int(self.do_bg), self._mode, self.smooth, self.alpha, self.beta, int(self._focal_on), self.gamma)
        return node_for(RegionNode, logits, labels, settings + (weight_ptr,))


@manager.LOSSES.add_component
class SoftDiceLoss(_RegionLoss):
    """nnU-Net's soft Dice (MemoryEfficientSoftDiceLoss) with MONAI's options, masked by ``ignore_index``:
    ``1 - mean((2 TP + smooth) / max(sum p^q + sum t + smooth, 1e-8))`` over the scored classes (and the samples unless
    ``batch_dice``), TP = sum p t, q = 2 with ``squared_pred``; ``do_bg=False`` leaves class 0 out when there is more than one
    class.  Returns ``(loss, per_channel_dice)``; the per-class Dice lists every class, the background included."""

    def __init__(self, activation='softmax', batch_dice=True, do_bg=False, smooth=1e-5, squared_pred=False, ignore_index=255):
        super().__init__(activation, batch_dice, do_bg, smooth, squared_pred, ignore_index)

    def forward(self, logits, labels):
        node = self._node(logits, labels)
        return Scalar([(1.0, node, "dice")]), per_channel_dice(node)


@manager.LOSSES.add_component
class TverskyLoss(_RegionLoss):
    """``1 - mean((TP + smooth) / (TP + alpha FP + beta FN + smooth))`` with FP = sum p - TP, FN = sum t - TP under the mask;
    alpha = beta = 0.5 is the soft Dice.  The other options are SoftDiceLoss's (``squared_pred`` must stay False).  Returns
    ``(loss, per_channel_dice)``; the second value is the Tversky index per class."""

    def __init__(self, alpha=0.3, beta=0.7, activation='softmax', batch_dice=True, do_bg=False, smooth=1e-5, squared_pred=False,
                 ignore_index=255):
        super().__init__(activation, batch_dice, do_bg, smooth, squared_pred, ignore_index, mode=REGION_TVERSKY, alpha=alpha,
                         beta=beta)

    def forward(self, logits, labels):
        node = self._node(logits, labels)
        return Scalar([(1.0, node, "dice")]), per_channel_dice(node)


@manager.LOSSES.add_component
class FocalLoss(_RegionLoss):
    """``sum w_y (1 - p_y)^gamma (-log p_y) / sum w_y`` over the voxels whose label is a class and not ``ignore_index``, p the
    softmax of the logits as given; ``weight`` is an optional list of per-class weights (default ones).  ``gamma=0`` is the
    plain (unweighted, unless ``weight``) cross entropy; gamma must be 0 or >= 1.  ``edge_label=True`` needs edge maps, which
    this package's datasets do not produce: ``loss_computation`` raises."""

    def __init__(self, gamma=2.0, weight=None, ignore_index=255, edge_label=False):
        super().__init__(ignore_index=ignore_index, focal_on=True, gamma=gamma, weight=weight)
        self.edge_label = edge_label

    def forward(self, logits, labels):
        return Scalar([(1.0, self._node(logits, labels), "ce")])


@manager.LOSSES.add_component
class DiceCELoss(_RegionLoss):
    """``lambda_dice * SoftDiceLoss + lambda_ce * FocalLoss(gamma, weight)`` (nnU-Net's DC_and_CE_loss at gamma = 0), both
    terms on ONE node: one statistics pass and one gradient pass over the logits.  Returns ``(loss, per_channel_dice)``."""

    def __init__(self, lambda_dice=1.0, lambda_ce=1.0, gamma=0.0, weight=None, activation='softmax', batch_dice=True,
                 do_bg=False, smooth=1e-5, squared_pred=False, ignore_index=255):
        super().__init__(activation, batch_dice, do_bg, smooth, squared_pred, ignore_index, focal_on=True, gamma=gamma,
                         weight=weight)
        self.lambda_dice, self.lambda_ce = float(lambda_dice), float(lambda_ce)

    def forward(self, logits, labels):
        node = self._node(logits, labels)
        return Scalar([(self.lambda_ce, node, "ce"), (self.lambda_dice, node, "dice")]), per_channel_dice(node)
