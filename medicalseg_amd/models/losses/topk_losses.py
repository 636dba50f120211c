"""Top-k cross entropy and Dice + top-k (nnU-Net's TopKLoss / DC_and_topk_loss, its nnUNetTrainerTopk10Loss and DiceTopK10
trainers) over msk_topk_ce_fwd / msk_topk_ce_bwd (medicalseg_amd/csrc/msk_loss_topk.hip; tests/topk_reference.py states the
formulas): cross entropy averaged over the hardest k per cent of the voxels.  The K-th largest per-voxel loss is found by an exact
radix select on the device; K, the threshold and the weight of the voxels tied at it are read there by the backward pass, so
nothing is downloaded and nothing synchronises.

Whenever no voxel is ignored this is ``torch.topk(cross_entropy(reduction='none').view(-1), int(V * k / 100)).mean()``.  With
ignored voxels nnU-Net counts them in V with loss 0; here, as in ``DiceCELoss``, every sum leaves them out: K is k per cent of the
voxels whose label is a class and not ``ignore_index``.  Voxels tied at the threshold share the remaining weight equally (a
subgradient that gives the same loss value and does not depend on the voxel order).

With several ranks the selection is rank-local, like the batch-Dice sums: no collective is added."""
import numpy as np

from ... import nn
from ...cvlibs import manager
from .fused import REGION_DICE, Scalar, TopKNode, node_for, per_channel_dice
from .loss_utils import device_weights
from .region_losses import _RegionLoss


class _TopKTerm:
    """k, the class weights and the node of the top-k term, shared by the two losses"""

    def _init_topk(self, k, weight, ignore_index):
        k = float(k)
        if not 0.0 < k <= 100.0:
            raise ValueError("k is the percentage of voxels that count and must be in (0, 100], but it is {}".format(k))
        self.k, self.topk_ignore_index = k, int(ignore_index)
        self.topk_weight = None if weight is None else np.asarray(weight, dtype=np.float32).reshape(-1)
        if self.topk_weight is not None and (self.topk_weight < 0).any():
            raise ValueError("the class weights must be >= 0, but they are {}".format(self.topk_weight.tolist()))
        self._topk_weight_dev = None

    def _topk_node(self, logits, labels):
        if not 2 <= logits.c <= 64:
            raise ValueError("the logits have %d classes; 2 .. 64 are supported" % logits.c)
        weight_ptr = None
        if self.topk_weight is not None:
            if self.topk_weight.size != logits.c:
                raise ValueError("%s weight has %d entries for %d classes" % (type(self).__name__, self.topk_weight.size, logits.c))
            self._topk_weight_dev = device_weights(logits.dev, self.topk_weight, self._topk_weight_dev)
            weight_ptr = self._topk_weight_dev[1]
        return node_for(TopKNode, logits, labels, (self.topk_ignore_index, self.k, weight_ptr))


@manager.LOSSES.add_component
class TopKLoss(nn.Layer, _TopKTerm):
    """``sum of the K largest w_y (-log softmax(z)_y) / K`` over the voxels whose label is a class and not ``ignore_index``,
    K = floor(k / 100 * their number), at least 1; ``weight`` is an optional list of per-class weights >= 0 (default ones).
    k = 100 is the plain (unweighted mean) cross entropy.  Returns a ``Scalar``."""

    def __init__(self, k=10, weight=None, ignore_index=255):
        super().__init__()
        self._init_topk(k, weight, ignore_index)
        self.ignore_index, self.weight = self.topk_ignore_index, self.topk_weight

    def forward(self, logits, labels):
        return Scalar([(1.0, self._topk_node(logits, labels), "topk")])


@manager.LOSSES.add_component
class DiceTopKLoss(_RegionLoss, _TopKTerm):
    """``lambda_dice * SoftDiceLoss + lambda_topk * TopKLoss(k, weight)`` (nnU-Net's DC_and_topk_loss).  The Dice term is a
    region node without the cross-entropy term, the top-k term a top-k node on the same logits: two forward passes, and in
    backward the first writes dL/dlogits and the second adds into it.  Returns ``(loss, per_channel_dice)``."""

    def __init__(self, lambda_dice=1.0, lambda_topk=1.0, k=10, weight=None, activation='softmax', batch_dice=True, do_bg=False,
                 smooth=1e-5, squared_pred=False, ignore_index=255):
        super().__init__(activation, batch_dice, do_bg, smooth, squared_pred, ignore_index, mode=REGION_DICE, focal_on=False)
        self._init_topk(k, weight, ignore_index)
        self.lambda_dice, self.lambda_topk = float(lambda_dice), float(lambda_topk)

    def forward(self, logits, labels):
        topk = self._topk_node(logits, labels)       # first: it refuses what the top-k kernels do not take (one class)
        dice = self._node(logits, labels)
        return Scalar([(self.lambda_dice, dice, "dice"), (self.lambda_topk, topk, "topk")]), per_channel_dice(dice)
