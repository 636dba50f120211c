"""Lovasz-Softmax and Dice + Lovasz-Softmax (Berman, Triki, Blaschko, CVPR 2018; PaddleSeg's LovaszSoftmaxLoss) over
msk_lovasz_fwd / msk_lovasz_bwd (medicalseg_amd/csrc/msk_loss_lovasz.hip; tests/lovasz_reference.py states the formulas): the
convex surrogate of the Jaccard index, the one number of ``evaluate(hard_metrics=True)`` (``miou``, ``class_iou``) the other
losses do not optimise.  Per class the softmax errors ``|[y == c] - p_c|`` are sorted in descending order by an exact radix sort
on the device, ties in voxel order, and weighted by the gradient of the Jaccard index along that order; the sorted keys, the
permutation and dL/de stay on the device for the backward pass, so nothing is downloaded and nothing synchronises.

Whenever no voxel is ignored this is Berman's ``lovasz_softmax(softmax(logits), labels, classes, per_image)``.  Voxels whose label
is ``ignore_index`` or outside [0, C) are removed before anything else, as in ``DiceCELoss`` and ``TopKLoss``.

With several ranks the sort is rank-local, like the batch-Dice sums and the top-k selection: no collective is added."""
from ... import nn
from ...cvlibs import manager
from .fused import LOVASZ_ALL, LOVASZ_LIST, LOVASZ_PRESENT, REGION_DICE, LovaszNode, Scalar, node_for, per_channel_dice
from .region_losses import _RegionLoss


class _LovaszTerm:
    """classes, per_image and the node of the Lovasz term, shared by the two losses"""

    def _init_lovasz(self, classes, per_image, ignore_index):
        self.lovasz_mask = 0
        if isinstance(classes, str):
            if classes not in ("present", "all"):
                raise ValueError("classes must be 'present', 'all' or a list of class indices, but it is {!r}".format(classes))
            self.lovasz_mode = LOVASZ_PRESENT if classes == "present" else LOVASZ_ALL
        else:
            listed = [int(c) for c in classes]
            if not listed or any(c != f or not 0 <= c < 64 for c, f in zip(listed, classes)) or len(set(listed)) != len(listed):
                raise ValueError("classes must list distinct class indices in [0, 64), but it is {!r}".format(classes))
            self.lovasz_mode = LOVASZ_LIST
            for c in listed:
                self.lovasz_mask |= 1 << c
        self.classes, self.per_image, self.lovasz_ignore_index = classes, bool(per_image), int(ignore_index)

    def _lovasz_node(self, logits, labels):
        if not 2 <= logits.c <= 64:
            raise ValueError("the logits have %d classes; 2 .. 64 are supported" % logits.c)
        if self.lovasz_mask >> logits.c:
            raise ValueError("%s classes=%r names a class outside the %d of the logits" % (type(self).__name__, self.classes, logits.c))
        return node_for(LovaszNode, logits, labels, (self.lovasz_ignore_index, self.lovasz_mode, self.lovasz_mask, self.per_image))


@manager.LOSSES.add_component
class LovaszSoftmaxLoss(nn.Layer, _LovaszTerm):
    """The mean over the counted classes of ``sum_i e_(i) g_i``: e the errors ``|[y == c] - softmax(z)_c|`` of the voxels whose
    label is a class and not ``ignore_index`` in descending order, g the gradient of the Jaccard index along that order.
    ``classes``: 'present' counts the classes that occur in the labels, 'all' every class, a list those of its classes that
    occur.  ``per_image=True`` takes the loss per sample and averages.  Returns a ``Scalar``."""

    def __init__(self, classes='present', per_image=False, ignore_index=255):
        super().__init__()
        self._init_lovasz(classes, per_image, ignore_index)
        self.ignore_index = self.lovasz_ignore_index

    def forward(self, logits, labels):
        return Scalar([(1.0, self._lovasz_node(logits, labels), "lovasz")])


@manager.LOSSES.add_component
class DiceLovaszLoss(_RegionLoss, _LovaszTerm):
    """``lambda_dice * SoftDiceLoss + lambda_lovasz * LovaszSoftmaxLoss(classes, per_image)``.  The Dice term is a region node
    without the cross-entropy term, the Lovasz term a Lovasz node on the same logits: two forward passes, and in backward the
    first writes dL/dlogits and the second adds into it.  Returns ``(loss, per_channel_dice)``."""

    def __init__(self, lambda_dice=1.0, lambda_lovasz=1.0, classes='present', per_image=False, activation='softmax', batch_dice=True,
                 do_bg=False, smooth=1e-5, squared_pred=False, ignore_index=255):
        super().__init__(activation, batch_dice, do_bg, smooth, squared_pred, ignore_index, mode=REGION_DICE, focal_on=False)
        self._init_lovasz(classes, per_image, ignore_index)
        self.lambda_dice, self.lambda_lovasz = float(lambda_dice), float(lambda_lovasz)

    def forward(self, logits, labels):
        lovasz = self._lovasz_node(logits, labels)   # first: it refuses what the Lovasz kernels do not take (one class)
        dice = self._node(logits, labels)
        return Scalar([(self.lambda_dice, dice, "dice"), (self.lambda_lovasz, lovasz, "lovasz")]), per_channel_dice(dice)
