"""Boundary loss and Dice + boundary loss (Kervadec et al., "Boundary loss for highly unbalanced segmentation", MIDL 2019; the
BDLoss / DC_and_BD_loss of the nnU-Net loss collections) over msk_label_sdf and msk_boundary_loss_fwd / msk_boundary_loss_bwd
(medicalseg_amd/csrc/msk_loss_boundary.hip; tests/boundary_reference.py states the formulas): the softmax probability times the
signed distance map of the ground truth, averaged over the valid voxels and the classes of the set.  The maps are built on the
device from the label patch of every step by the exact distance transform of the surface metrics (msk_edt.hip), so random patch
crops need no precomputed maps: nothing is downloaded and nothing synchronises.

A voxel counts when its label is a class and not ``ignore_index``.  The map of a class treats every other value -- 255 and labels
beyond the class range included -- as outside the class.  With nothing ignored the loss is Kervadec's
``(probs[:, idc] * dist_maps[:, idc]).mean()``.  The loss is signed and unbounded below; it is meant to be mixed with a region
term (``DiceBoundaryLoss``), whose weight the caller may lower between iterations.

With several ranks the sums are rank-local, like the batch-Dice sums: no collective is added."""
from ... import nn
from ...cvlibs import manager
from ...utils.metric import _spacing_weights
from .fused import REGION_DICE, BoundaryNode, Scalar, node_for, per_channel_dice
from .region_losses import _RegionLoss


class _BoundaryTerm:
    """the class set, the spacing and the node of the boundary term, shared by the two losses"""

    def _init_boundary(self, classes, spacing, ignore_index):
        if classes is not None:
            classes = sorted({int(c) for c in classes})
            if not classes or classes[0] < 0 or classes[-1] > 63:
                raise ValueError("classes must list at least one class in 0 .. 63, but it is {}".format(classes))
        _, s = _spacing_weights(spacing)       # raises on anything msk_edt3d would refuse
        self.classes, self.boundary_ignore_index = classes, int(ignore_index)
        self.spacing = None if s is None else tuple(float(v) for v in s)

    def _boundary_node(self, logits, labels):
        if not 2 <= logits.c <= 64:
            raise ValueError("the logits have %d classes; 2 .. 64 are supported" % logits.c)
        classes = list(range(1, logits.c)) if self.classes is None else self.classes
        if classes[-1] >= logits.c:
            raise ValueError("%s classes %s name a class the %d-class logits do not have" % (type(self).__name__, classes, logits.c))
        mask = sum(1 << c for c in classes)
        return node_for(BoundaryNode, logits, labels, (self.boundary_ignore_index, mask, self.spacing))


@manager.LOSSES.add_component
class BoundaryLoss(nn.Layer, _BoundaryTerm):
    """``sum over the valid voxels and the classes of the set of softmax(z)_c * phi_c / (n_valid * |set|)``, phi_c the signed
    distance map of class c in the label: the distance to the class outside it, ``1 -`` the distance to its complement inside it,
    0 where the class is absent or fills the volume.  ``classes`` lists the set (default: every class but 0), ``spacing`` is
    (sz, sy, sx) or None for unit voxels.  Returns a ``Scalar``."""

    def __init__(self, classes=None, spacing=None, ignore_index=255):
        super().__init__()
        self._init_boundary(classes, spacing, ignore_index)
        self.ignore_index = self.boundary_ignore_index

    def forward(self, logits, labels):
        return Scalar([(1.0, self._boundary_node(logits, labels), "boundary")])


@manager.LOSSES.add_component
class DiceBoundaryLoss(_RegionLoss, _BoundaryTerm):
    """``lambda_dice * SoftDiceLoss + lambda_boundary * BoundaryLoss(classes, spacing)``.  The Dice term is a region node without
    the cross-entropy term, the boundary term a boundary node on the same logits: in backward the first writes dL/dlogits and the
    second adds into it.  ``lambda_boundary`` is read at every forward, so a caller can raise it between iterations (Kervadec's
    rebalancing); no scheduler is built in.  Returns ``(loss, per_channel_dice)``."""

    def __init__(self, lambda_dice=1.0, lambda_boundary=0.01, classes=None, spacing=None, activation='softmax', batch_dice=True,
                 do_bg=False, smooth=1e-5, squared_pred=False, ignore_index=255):
        if activation != 'softmax':
            raise ValueError("the boundary term needs activation='softmax', but it is {!r}".format(activation))
        super().__init__(activation, batch_dice, do_bg, smooth, squared_pred, ignore_index, mode=REGION_DICE, focal_on=False)
        self._init_boundary(classes, spacing, ignore_index)
        self.lambda_dice, self.lambda_boundary = float(lambda_dice), float(lambda_boundary)

    def forward(self, logits, labels):
        boundary = self._boundary_node(logits, labels)   # first: it refuses what the boundary kernels do not take (one class)
        dice = self._node(logits, labels)
        return Scalar([(float(self.lambda_dice), dice, "dice"), (float(self.lambda_boundary), boundary, "boundary")]), \
            per_channel_dice(dice)
