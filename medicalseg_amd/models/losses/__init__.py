from .loss_utils import flatten, class_weights
from .cross_entropy_loss import CrossEntropyLoss
from .dice_loss import DiceLoss
from .mixes_losses import MixedLoss
from .binary_cross_entropy_loss import BCELoss
from .region_losses import DiceCELoss, FocalLoss, SoftDiceLoss, TverskyLoss
from .region_based_losses import DiceBCERegionLoss, RegionSpec
from .topk_losses import DiceTopKLoss, TopKLoss
from .boundary_losses import BoundaryLoss, DiceBoundaryLoss
from .lovasz_losses import DiceLovaszLoss, LovaszSoftmaxLoss
