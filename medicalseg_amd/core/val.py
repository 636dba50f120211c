"""Evaluation loop (reference medicalseg/core/val.py:29-187): eval-mode forward per
validation volume (batch 1), mDice = mean over volumes of the mean over classes of the
soft V-Net dice that DiceLoss returns as a side output."""
import os
import time

import numpy as np

from .. import nn
from ..datasets import DataLoader
from ..device import to_tensor
from ..utils import TimeAverager, logger, loss_computation, metric, save_array
from . import infer

np.set_printoptions(suppress=True)


def _load_dataset_json(eval_dataset):
    path = getattr(eval_dataset, "dataset_json_path", "")
    if path and os.path.exists(path):
        import json
        with open(path, encoding="utf-8") as f:
            return json.load(f)
    return None


_IDENTITY_GEOMETRY = {"spacing": (1.0, 1.0, 1.0), "direction": (1, 0, 0, 0, 1, 0, 0, 0, 1), "origin": (0.0, 0.0, 0.0),
                      "format": "xyz"}
_warned_geometry = [False]


def _image_info(dataset_json, idx):
    """spacing / direction / origin of one validation volume (reference core/val.py:96-97,149-154).  Identity geometry only
    when the dataset HAS no json (synthetic data); with a json, a volume or key that is missing raises KeyError as the
    reference's dictionary lookups do -- a NIfTI file with a silently wrong geometry is worse than no file."""
    if not dataset_json:
        if not _warned_geometry[0]:
            logger.warning("evaluate: the dataset has no dataset.json; predictions are saved with identity spacing / origin / direction.")
            _warned_geometry[0] = True
        return dict(_IDENTITY_GEOMETRY)
    name = str(idx[0]).split("/")[-1].split(".")[0]
    j = dataset_json["training"][name]
    return {"spacing": j["spacing_resample"], "direction": j["direction"], "origin": j["origin"], "format": "xyz"}


def evaluate(model, eval_dataset, losses, num_workers=0, print_detail=True, auc_roc=False, writer=None,
             save_dir=None, hard_metrics=False, pred_transform=None, auc_device=False, surface_metrics=False,
             surface_spacing=None, aug_eval=False, scales=1.0, flip_axes=(), sliding_window=None, sw_overlap=0.5,
             sw_mode='gaussian', sw_batch_size=1, sw_mirror_axes=(), regions=None):
    """regions (region-based training): a RegionSpec with class_order; by default ``losses['types'][0].region_spec`` when
    the loss has one (DiceBCERegionLoss), so validation during training and val.py need no option.  The model's channels are
    then sigmoid regions: the hard-label prediction is rebuilt from the thresholded logits (``inference(regions=...)`` /
    ``sliding_window_inference(regions=...)``), ``mdice`` is the per-region soft Dice of the loss, and ``hard_metrics`` adds
    region_dice (mean over the regions of the Dice pooled over the set), class_region_dice (per region) and
    region_dice_per_case (mean over volumes of the region-mean Dice), computed on the host in exact integers from the
    confusion counts already taken (utils.metric.region_areas_from_counts).  ``auc_roc`` and ``aug_eval`` need softmax
    probabilities: together with regions they raise ValueError.

    sliding_window: a roi (rd, rh, rw); the logits and the prediction of every volume come from
    ``infer.sliding_window_inference(roi_size=sliding_window, overlap=sw_overlap, mode=sw_mode, sw_batch_size=sw_batch_size,
    mirror_axes=sw_mirror_axes)`` -- the net on overlapping windows at the volume's own resolution, blended on the device -- in
    place of the one forward of ``infer.inference``; everything downstream (loss, mdice, hard and surface metrics, AUC, saved
    arrays) is unchanged.  sw_mirror_axes (0/1/2 = D/H/W): every window is also predicted mirrored along every subset of these
    axes and the mean of the logits is blended (nnU-Net's mirroring; sw_batch_size then counts passes); what comes back is
    still logits.  Without sliding_window a non-empty sw_mirror_axes raises ValueError.
    Together with aug_eval it raises ValueError: combining the two is out of scope here.  The call keeps its device buffers
    (one accumulator, patch batch and plan tables per geometry; volumes of another extent replace the accumulator) after the
    loop for the next evaluation; ``infer.sliding_release(device)`` frees them.

    aug_eval: the hard-label prediction (what pred_transform, hard_metrics, surface_metrics and the saved arrays see) and
    the AUC scores come from ``infer.aug_inference(scales=scales, flip_axes=flip_axes)``: the mean softmax over the mirrored
    (flip_axes: 0/1/2 = D/H/W, every subset) and rescaled passes and its argmax, in place of the single pass's.  ``mdice``
    and the loss stay those of the plain pass (its logits come back from the same call), so ``scales`` must contain 1.0.

    auc_device (with auc_roc): the softmax scores of every volume stay on the device as sortable keys
    (utils.metric.AucScores) and the AUC comes from exact pair counts taken there, downloaded once after the loop --
    the same float as the host path, without the download of the probabilities and the host sorts.

    hard_metrics: also score the hard-label prediction (the segmentation ``inference`` returns, passed through
    ``pred_transform`` first when given: any callable IntTensor -> IntTensor, e.g. TopkLargestConnectComponent(k=1))
    against the label on the device: confusion counts of every volume into one buffer (utils.metric.confusion_counts),
    downloaded once after the loop.  Adds miou, dice (both pooled over the set), dice_per_case (mean over volumes of the
    class-mean Dice), acc, kappa, class_iou, class_dice to the result.  ``mdice`` stays the soft V-Net Dice of the loss.

    surface_metrics: also score the boundary of the same hard-label prediction (after ``pred_transform``, as above) per
    volume and foreground class on the device (utils.metric.surface_metrics: exact distance transforms, only the surface
    voxels' distances are downloaded).  Adds hd95 and assd (nanmean over the volumes of the nanmean over the classes
    1 .. C-1), class_hd95 and class_assd (nanmean over the volumes) and surface_nan (the number of (volume, class) pairs
    whose class has no surface in the prediction or in the label: nan, left out of the means).  ``surface_spacing``:
    (s0, s1, s2) in the LABEL ARRAY's axis order, None = voxel units.  The dataset json's ``spacing_resample`` is not
    accepted as a source: it exists only for datasets prepared with a resample step, is keyed by the source file (a
    multi-volume file yields several arrays under other names), and neither the json nor the dataset records which
    array axis it belongs to after the remaining preparation steps -- the 'xyz' of the saved NIfTI files above is an
    assumption of this loop, not a recorded fact.  ignore_index gets no special treatment."""
    if regions is None:
        regions = getattr(losses['types'][0], 'region_spec', None)
    if regions is not None:
        if auc_roc or aug_eval:
            raise ValueError("evaluate: auc_roc=True and aug_eval=True score softmax probabilities and are not supported "
                             "together with regions")
        if getattr(regions, 'class_order', None) is None:
            raise ValueError("evaluate: regions needs a RegionSpec with class_order")
    if aug_eval and (1.0, 0) not in infer.tta_passes(scales, flip_axes):
        raise ValueError("evaluate(aug_eval=True): scales must contain 1.0 (mdice and the loss are the plain pass's), got %r"
                         % (scales,))
    if sliding_window is not None and aug_eval:
        raise ValueError("evaluate: sliding_window together with aug_eval=True is not supported")
    sw_mirror_axes = tuple(sw_mirror_axes)
    if sw_mirror_axes and sliding_window is None:
        raise ValueError("evaluate: sw_mirror_axes=%r needs sliding_window (aug_eval mirrors whole volumes)" % (sw_mirror_axes,))
    infer.tta_passes(1.0, sw_mirror_axes)            # a bad or duplicate axis raises here, before any work

    region_kw = {} if regions is None else {"regions": regions}      # without regions the calls are what they were
    # the chosen prediction path as one callable -> (pred, logits, mean_probs or None)
    if aug_eval:
        def predict(im, ori_shape):
            transforms = eval_dataset.transforms.transforms
            pred, mean_probs, logits = infer.aug_inference(model, im, ori_shape=ori_shape, transforms=transforms, scales=scales,
                                                           flip_axes=flip_axes, with_plain=True)
            if tuple(ori_shape) != tuple(logits.shape[2:]):      # as inference() does before the loss
                logits = infer.reverse_transform(logits, ori_shape, transforms, mode='bilinear')
            return pred, logits, mean_probs
    elif sliding_window is not None:
        def predict(im, ori_shape):
            return infer.sliding_window_inference(model, im, sliding_window, overlap=sw_overlap, mode=sw_mode,
                                                  sw_batch_size=sw_batch_size, ori_shape=ori_shape,
                                                  transforms=eval_dataset.transforms.transforms,
                                                  mirror_axes=sw_mirror_axes, **region_kw) + (None,)
    else:
        def predict(im, ori_shape):
            return infer.inference(model, im, ori_shape=ori_shape, transforms=eval_dataset.transforms.transforms,
                                   **region_kw) + (None,)
    new_loss = {'types': [losses['types'][0]], 'coef': [losses['coef'][0]]}
    if writer is not None:
        logger.warning("evaluate(writer=...): VisualDL logging is not built; the writer is ignored.")
    model.eval()
    dataset_json = _load_dataset_json(eval_dataset)
    from ..parallel import ParallelEnv
    env = ParallelEnv()
    local_rank = env.local_rank
    loader = DataLoader(eval_dataset, batch_size=1, shuffle=False, drop_last=False, num_workers=num_workers)
    total_iters = len(loader)
    if print_detail:
        logger.info("Start evaluating (total_samples: {}, total_iters: {})...".format(len(eval_dataset), total_iters))
    reader_cost_averager = TimeAverager()
    batch_cost_averager = TimeAverager()
    batch_start = time.time()
    mdice = 0.0
    channel_dice_array = np.array([])
    loss_all = 0.0
    counts = None                    # hard_metrics: [total_iters, K*K + 1] confusion counts on the device
    num_classes, ignore_index = eval_dataset.num_classes, getattr(eval_dataset, "ignore_index", 255)
    logits_all, label_all = [], []   # auc_roc: softmax scores and labels of the whole set on the host (core/val.py:121-131)
    auc_scores = None                # auc_roc with auc_device: the same scores as keys on the device
    surface_cases = []               # surface_metrics: one utils.metric.surface_metrics result per volume
    with nn.fused_inference():       # one scope for the whole set: BN is folded into the conv weights once
        for it, (im, label, idx) in enumerate(loader):
            reader_cost_averager.record(time.time() - batch_start)
            label_t = to_tensor(label.astype('int32'))
            pred, logits, mean_probs = predict(to_tensor(im), label.shape[-3:])
            loss, per_channel_dice = loss_computation(logits, label_t, new_loss)
            loss = sum(loss)
            if hard_metrics or surface_metrics:
                hard = pred_transform(pred) if pred_transform is not None else pred
                if isinstance(hard, tuple):     # the transform classes return (pred, label)
                    hard = hard[0]
            if hard_metrics:
                if counts is None:
                    counts = metric.ConfusionCounts(pred.dev, total_iters, num_classes, ignore_index, zero=True)
                metric.confusion_counts(hard, label_t, num_classes, ignore_index, out=counts.rows(it, len(label)))
            if surface_metrics:
                surface_cases.append(metric.surface_metrics(hard, label_t, num_classes, spacing=surface_spacing))
            if auc_roc:
                probs = mean_probs                                            # aug_eval: the mean softmax over the passes
                if probs is None:
                    probs = logits.empty_like()
                    logits.dev.call("msk_softmax_c", logits.msk(), probs.msk())   # F.softmax(logits, axis=1) on the device
                if auc_device:
                    if auc_scores is None:      # room for the whole set at the size of the first volume; grows otherwise
                        auc_scores = metric.AucScores(logits.dev, num_classes, total_iters * probs.voxels)
                    auc_scores.add(probs, label_t)
                else:
                    logits_all.append(probs.numpy())
                    label_all.append(np.asarray(label))
            loss_all += loss.numpy()
            pcd = np.asarray(per_channel_dice)
            mdice += np.mean(pcd)
            channel_dice_array = pcd.copy() if channel_dice_array.size == 0 else channel_dice_array + pcd
            if it < 5 and save_dir is not None:
                # reference core/val.py:137-153: npy + nii.gz with the volume's geometry from the dataset json
                info = _image_info(dataset_json, idx)
                save_array(save_path=os.path.join(save_dir, str(it)),
                           save_content={'pred': pred.numpy(), 'label': label, 'img': im},
                           form=('npy', 'nii.gz'), image_infor=info)
            batch_cost_averager.record(time.time() - batch_start, num_samples=len(label))
            reader_cost_averager.reset()
            batch_cost_averager.reset()
            batch_start = time.time()
    total_iters = max(total_iters, 1)
    mdice /= total_iters
    channel_dice_array = channel_dice_array / total_iters
    loss_all = loss_all / total_iters
    result_dict = {"mdice": float(mdice)}
    auc_infor = ""
    if auc_roc:
        if auc_device:
            if auc_scores is None:
                raise ValueError("evaluate(auc_roc=True, auc_device=True): the dataset is empty")
            try:
                auc = metric.auc_from_counts(auc_scores.counts(), eval_dataset.num_classes)
            finally:
                auc_scores.free()
        else:
            auc = metric.auc_roc(np.concatenate(logits_all), np.concatenate(label_all), num_classes=eval_dataset.num_classes)
        auc_infor = ' Auc_roc: {:.4f}'.format(auc)
        result_dict['auc_roc'] = auc
    hard_infor = None
    if hard_metrics and counts is not None:
        c = counts.numpy()
        counts.free()
        areas = metric.areas_from_counts(c, num_classes, ignore_index)
        class_iou, miou = metric.mean_iou(*areas)
        class_dice, hdice = metric.dice(*areas)
        _, acc = metric.accuracy(areas[0], areas[1])
        kappa = metric.kappa(*areas)
        dice_per_case = float(np.mean(metric.per_case(c, num_classes, ignore_index)["mdice"]))
        result_dict.update(miou=float(miou), dice=float(hdice), dice_per_case=dice_per_case, acc=float(acc),
                           kappa=float(kappa), class_iou=class_iou, class_dice=class_dice)
        hard_infor = ("[EVAL] Hard labels: mIoU: {:.4f}, Dice: {:.4f}, Dice per case: {:.4f}, Acc: {:.4f}, Kappa: {:.4f}".format(
            miou, hdice, dice_per_case, acc, kappa),
            "[EVAL] Class IoU: \n" + str(np.round(class_iou, 4)) + "\n[EVAL] Class hard dice: \n" + str(np.round(class_dice, 4)))
        if regions is not None:
            table, R = regions.table(), regions.num_regions
            class_region_dice, region_dice = metric.dice(*metric.region_areas_from_counts(c, num_classes, table, R))
            rows = metric.region_areas_from_counts(c, num_classes, table, R, per_volume=True)
            region_dice_per_case = float(np.mean([metric.dice(i, p, l)[1] for i, p, l in zip(*rows)]))
            result_dict.update(region_dice=float(region_dice), class_region_dice=class_region_dice,
                               region_dice_per_case=region_dice_per_case)
            hard_infor = (hard_infor[0] + ", Region Dice: {:.4f}, Region Dice per case: {:.4f}".format(
                region_dice, region_dice_per_case),
                hard_infor[1] + "\n[EVAL] Region hard dice: \n" + str(np.round(class_region_dice, 4)))
    surface_infor = None
    if surface_metrics and surface_cases:
        ss = metric.surface_summary(surface_cases)
        result_dict.update(ss)
        surface_infor = ("[EVAL] Surface ({}): HD95: {:.4f}, ASSD: {:.4f}, nan entries: {}".format(
            "voxels" if surface_spacing is None else "spacing {}".format(tuple(float(v) for v in surface_spacing)),
            ss["hd95"], ss["assd"], ss["surface_nan"]),
            "[EVAL] Class HD95: \n" + str(np.round(ss["class_hd95"], 4)) + "\n[EVAL] Class ASSD: \n" + str(np.round(ss["class_assd"], 4)))
    if print_detail and local_rank == 0:
        logger.info("[EVAL] #Images: {}, Dice: {:.4f}, Loss: {:6f}".format(len(eval_dataset), mdice,
                                                                           float(np.ravel(loss_all)[0])) + auc_infor)
        logger.info("[EVAL] Class dice: \n" + str(np.round(channel_dice_array, 4)))
        if hard_infor is not None:
            logger.info(hard_infor[0])
            logger.info(hard_infor[1])
        if surface_infor is not None:
            logger.info(surface_infor[0])
            logger.info(surface_infor[1])
    return result_dict
