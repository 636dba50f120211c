import numpy as np

from ... import nn
from ...cvlibs import manager
from .fused import LossNode, Scalar, node_for, per_channel_dice
from .loss_utils import device_weights


@manager.LOSSES.add_component
class DiceLoss(nn.Layer):
    """V-Net dice with squared denominator (reference losses/dice_loss.py:24-102):
    per_channel = 2*w_c*sum(p*t)/clip(sum(p^2)+sum(t^2), 1e-6); loss = 1 - mean_c; p = sigmoid(logits)
    (sigmoid_norm=True, the shipped configs) or softmax over the classes (dice_loss.py:40-43); `weight` is the
    optional per-class factor on the intersection (dice_loss.py:68-69).  Returns (loss, per_channel_dice) like
    the reference (the second value is a lazily fetched host array)."""

    def __init__(self, sigmoid_norm=True, weight=None):
        super(DiceLoss, self).__init__()
        self.sigmoid_norm = bool(sigmoid_norm)
        self.weight = None if weight is None else np.asarray(weight, dtype=np.float32).reshape(-1)
        self._weight_dev = None
        self.eps = 1e-5

    def forward(self, logits, labels):
        node = node_for(LossNode, logits, labels)
        weight_ptr = None
        if self.weight is not None:
            if self.weight.size != logits.c:
                raise ValueError("DiceLoss weight has %d entries for %d classes" % (self.weight.size, logits.c))
            self._weight_dev = device_weights(logits.dev, self.weight, self._weight_dev)
            weight_ptr = self._weight_dev[1]
        node.set_dice(not self.sigmoid_norm, weight_ptr)
        loss = Scalar([(1.0, node, "dice")])
        return loss, per_channel_dice(node)
