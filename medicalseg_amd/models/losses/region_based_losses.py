"""Region-based training (nnU-Net's ``regions`` / ``regions_class_order``): the network's channels are OVERLAPPING regions of
the label map -- whole tumour = {1, 2, 3}, tumour core = {2, 3}, enhancing = {3} -- each channel is a sigmoid, the loss is
nnU-Net's DC_and_BCE_loss, and the exported segmentation is rebuilt from the thresholded channels in a fixed order.  The fused
kernels are msk_mlabel_loss_fwd / msk_mlabel_loss_bwd / msk_regions_to_label (medicalseg_amd/csrc/msk_loss_mlabel.hip);
tests/mlabel_reference.py states the formulas.

The label stays the one int32 per voxel every transform, the label pyramid and the metrics carry: a table of 256 uint32 maps a
label value to the bit mask of the regions it belongs to.

With several ranks the batch-Dice sums (``batch_dice=True``) are those of each rank's own batch: no collective is added."""
import ctypes as C

import numpy as np

from ... import nn
from ...cvlibs import manager
from ...device import IntTensor
from .fused import MultiLabelNode, Scalar, node_for, per_channel_dice

MAX_REGIONS = 32
MAX_LABEL_VALUES = 256


class RegionSpec:
    """``regions``: a list whose entries are a label value or a list of label values (every value in [0, 256), no region
    empty, at most 32 regions).  ``class_order`` (optional, one label value per region): what ``to_label`` writes where a
    region's channel fires, regions taken in order so that the LAST region that fires wins (nnU-Net's loop over
    regions_class_order)."""

    def __init__(self, regions, class_order=None):
        if isinstance(regions, (int, np.integer)) or not len(regions):
            raise ValueError("regions must be a non-empty list of label values or lists of label values, got %r" % (regions,))
        if len(regions) > MAX_REGIONS:
            raise ValueError("at most %d regions are supported, got %d" % (MAX_REGIONS, len(regions)))
        self.regions = []
        for r in regions:
            values = [r] if isinstance(r, (int, np.integer)) and not isinstance(r, bool) else list(r)
            if not values:
                raise ValueError("a region is empty: %r" % (regions,))
            for v in values:
                if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= v < MAX_LABEL_VALUES:
                    raise ValueError("region label values must be integers in [0, %d), got %r" % (MAX_LABEL_VALUES, v))
            self.regions.append(tuple(int(v) for v in values))
        self.regions = tuple(self.regions)
        if class_order is not None:
            class_order = [int(v) for v in class_order]
            if len(class_order) != len(self.regions):
                raise ValueError("class_order has %d entries for %d regions" % (len(class_order), len(self.regions)))
            class_order = tuple(class_order)
        self.class_order = class_order
        self._dev_table = {}     # id(device) -> (device, pointer)

    @property
    def num_regions(self):
        return len(self.regions)

    def table(self):
        """uint32 [256]: bit r of table[v] is set when label value v belongs to region r"""
        t = np.zeros(MAX_LABEL_VALUES, dtype=np.uint32)
        for r, values in enumerate(self.regions):
            for v in values:
                t[v] |= np.uint32(1 << r)
        return t

    def device_table(self, dev):
        """(pointer, length) of the table on `dev`, uploaded once per device and kept for its lifetime"""
        held = self._dev_table.get(id(dev))
        if held is None or held[0] is not dev:
            t = self.table()
            ptr = dev.malloc(t.nbytes)
            dev.h2d(ptr, t)
            held = self._dev_table[id(dev)] = (dev, ptr)
        return held[1], MAX_LABEL_VALUES

    def to_label(self, logits):
        """IntTensor [N,1,D,H,W]: 0, then class_order[r] where channel r's LOGIT is above 0, r = 0 .. R-1 in order
        (msk_regions_to_label).  Lives in the activation arena, like inference()'s prediction."""
        if self.class_order is None:
            raise ValueError("RegionSpec.to_label needs class_order (one label value per region)")
        if logits.c != self.num_regions:
            raise ValueError("the logits have %d channels for %d regions" % (logits.c, self.num_regions))
        dev = logits.dev
        pred = IntTensor(dev, dev.arena.alloc(logits.voxels * 4), (logits.n, 1, logits.d, logits.h, logits.w), dev.arena.gen)
        order = (C.c_int32 * self.num_regions)(*self.class_order)
        dev.call("msk_regions_to_label", logits.msk(), order, C.c_void_p(pred.ptr))
        return pred


def as_region_spec(regions, class_order=None):
    """`regions` as a RegionSpec: one is passed through, a list builds one"""
    return regions if isinstance(regions, RegionSpec) else RegionSpec(regions, class_order)


@manager.LOSSES.add_component
class DiceBCERegionLoss(nn.Layer):
    """``lambda_dice * (1 - mean Dice) + lambda_bce * BCE`` over label regions, every channel a sigmoid (nnU-Net's
    DC_and_BCE_loss), both terms on ONE node: one statistics pass and one gradient pass over the logits.  The Dice is the masked
    soft Dice of SoftDiceLoss over ALL regions (``(2 TP + smooth) / max(sum p^q + sum t + smooth, 1e-8)``, per sample unless
    ``batch_dice``), the BCE term binary_cross_entropy_with_logits averaged over the valid voxels and the regions.  Returns
    ``(loss, per_channel_dice)``; ``region_spec`` is the RegionSpec that evaluate() and inference(regions=...) use.

    Two conventions differ from nnU-Net's: the Dice term is ``1 - dice`` (as SoftDiceLoss) where nnU-Net writes ``-dice``, and
    with an ignore label nnU-Net divides the BCE sum by the valid voxels only, not by R times that: ``lambda_bce = R``
    reproduces it."""

    def __init__(self, regions, class_order=None, lambda_dice=1.0, lambda_bce=1.0, batch_dice=True, smooth=1e-5,
                 squared_pred=False, ignore_index=255):
        super().__init__()
        if float(smooth) < 0:
            raise ValueError("smooth must be >= 0, but it is {}".format(smooth))
        self.region_spec = as_region_spec(regions, class_order)
        self.lambda_dice, self.lambda_bce = float(lambda_dice), float(lambda_bce)
        self.batch_dice, self.smooth, self.squared_pred = bool(batch_dice), float(smooth), bool(squared_pred)
        self.ignore_index = int(ignore_index)

    def forward(self, logits, labels):
        R = self.region_spec.num_regions
        if logits.c != R:
            raise ValueError("the logits have %d channels for %d regions" % (logits.c, R))
        ptr, length = self.region_spec.device_table(logits.dev)
        settings = (self.ignore_index, int(self.squared_pred), int(self.batch_dice), self.smooth, ptr, length)
        node = node_for(MultiLabelNode, logits, labels, settings)
        return Scalar([(self.lambda_bce, node, "bce"), (self.lambda_dice, node, "dice")]), per_channel_dice(node)
