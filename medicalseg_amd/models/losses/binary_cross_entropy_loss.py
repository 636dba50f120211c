from ... import nn
from ...cvlibs import manager
from .fused import BCENode, Scalar, node_for

_WEIGHT_MODES = {None: 0, 'dynamic': 1}
_POS_WEIGHT_NONE, _POS_WEIGHT_VALUE, _POS_WEIGHT_DYNAMIC = 0, 1, 2


@manager.LOSSES.add_component
class BCELoss(nn.Layer):
    """Binary cross entropy with logits, masked by ``ignore_index`` (reference
    losses/binary_cross_entropy_loss.py:22-172), evaluated by the fused kernels msk_bce_fwd / msk_bce_bwd.

    * target y: the label value itself when the logits have one channel; ``one_hot(label, C)`` otherwise, where a label
      outside [0, C) gives an all-zero row (ignore_index = 255 included).  [PADDLE] this is the behaviour of Paddle's GPU
      ``F.one_hot``, which MedicalSeg trains with;
    * mask = (label != ignore_index), one value per voxel, broadcast over the classes;
    * ``weight='dynamic'``: w = 2 neg / (pos + neg + 1e-10) y + 2 pos / (pos + neg + 1e-10) (1 - y), with pos = #(y == 1)
      and neg = #(y == 0) over the whole target, masked voxels included; ``pos_weight='dynamic'``: 2 neg / (pos + neg + 1e-10);
    * loss = mean(l * mask) / (mean(mask) + 1e-10) with l = binary_cross_entropy_with_logits(x, y, w, pos_weight).
    The weights carry no gradient.  Deliberate deviation: pos, neg and the mask sum are exact counts; the reference sums
    them in float32, which is inexact above 2^24 elements.

    ``weight`` is None or 'dynamic'.  Any other non-string ``weight`` raises TypeError with the reference's message.  The
    reference raises it for a Tensor only and lets other objects through to binary_cross_entropy_with_logits as
    per-element weights, which are not supported here.  ``pos_weight`` is None, a Python float or 'dynamic' (an int
    raises TypeError as in the reference).
    ``edge_label=True`` needs edge maps, which this port's datasets do not produce: ``loss_computation`` raises."""

    def __init__(self, weight=None, pos_weight=None, ignore_index=255, edge_label=False):
        super().__init__()
        self.weight = weight
        self.pos_weight = pos_weight
        self.ignore_index = ignore_index
        self.edge_label = edge_label
        self.EPS = 1e-10

        if self.weight is not None:
            if isinstance(self.weight, str):
                if self.weight != 'dynamic':
                    raise ValueError(
                        "if type of `weight` is str, it should equal to 'dynamic', but it is {}".format(self.weight))
            else:   # the reference: a Tensor only; per-element weights of any kind are not supported here
                raise TypeError(
                    'The type of `weight` is wrong, it should be Tensor or str, but it is {}'.format(type(self.weight)))

        self._pw_mode, self._pw_value = _POS_WEIGHT_NONE, 1.0
        if self.pos_weight is not None:
            if isinstance(self.pos_weight, str):
                if self.pos_weight != 'dynamic':
                    raise ValueError(
                        "if type of `pos_weight` is str, it should equal to 'dynamic', but it is {}".format(self.pos_weight))
                self._pw_mode = _POS_WEIGHT_DYNAMIC
            elif isinstance(self.pos_weight, float):
                self._pw_mode, self._pw_value = _POS_WEIGHT_VALUE, float(self.pos_weight)
            else:
                raise TypeError(
                    'The type of `pos_weight` is wrong, it should be float or str, but it is {}'.format(type(self.pos_weight)))

    def forward(self, logit, label):
        node = node_for(BCENode, logit, label, (int(self.ignore_index), _WEIGHT_MODES[self.weight], self._pw_mode, self._pw_value))
        return Scalar([(1.0, node, "bce")])
