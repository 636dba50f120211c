#!/usr/bin/env python
"""Evaluation entry point with the reference's command line (val.py:25-126)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Model evaluation')
    p.add_argument("--config", dest="cfg", help="The config file.", default=None, type=str)
    p.add_argument('--model_path', dest='model_path', help='The path of model for evaluation', type=str, default=None)
    p.add_argument('--save_dir', dest='save_dir', help='The path to save result', type=str, default="saved_model/val")
    p.add_argument('--num_workers', dest='num_workers', help='Num workers for data loader', type=int, default=0)
    p.add_argument('--print_detail', dest='print_detail', type=bool, default=True)
    p.add_argument('--auc_roc', dest='auc_roc', help='Whether to use auc_roc metric', type=bool, default=False)
    p.add_argument('--auc_device', dest='auc_device', type=bool, default=False,
                   help='With --auc_roc: keep the scores on the GPU and compute the AUC there (same value)')
    p.add_argument('--hard_metrics', dest='hard_metrics', type=bool, default=False,
                   help='Whether to report the hard-label metrics (mIoU, Dice, accuracy, kappa) of the prediction')
    p.add_argument('--surface_metrics', dest='surface_metrics', type=bool, default=False,
                   help='Whether to report the boundary metrics (HD95, ASSD; in voxels) of the hard-label prediction')
    p.add_argument('--aug_eval', dest='aug_eval', type=bool, default=False,
                   help='Whether to average the softmax over mirrored / rescaled passes (test-time augmentation)')
    p.add_argument('--scales', dest='scales', nargs='+', type=float, default=1.0,
                   help='With --aug_eval: scales of the passes; must contain 1.0')
    p.add_argument('--flip_axes', dest='flip_axes', nargs='*', type=int, default=(),
                   help='With --aug_eval: axes to mirror, 0 1 2 = D H W; every subset is one pass')
    p.add_argument('--sliding_window', dest='sliding_window', nargs=3, type=int, default=None, metavar=('D', 'H', 'W'),
                   help='Predict window by window at native resolution with this roi and blend the logits')
    p.add_argument('--sw_overlap', dest='sw_overlap', type=float, default=0.5,
                   help='With --sliding_window: overlap of neighbouring windows, 0 <= overlap < 1')
    p.add_argument('--sw_mode', dest='sw_mode', type=str, default='gaussian', choices=('gaussian', 'constant'),
                   help='With --sliding_window: window weight')
    p.add_argument('--sw_batch_size', dest='sw_batch_size', type=int, default=1,
                   help='With --sliding_window: windows per forward (passes per forward with --sw_mirror_axes)')
    p.add_argument('--sw_mirror_axes', dest='sw_mirror_axes', nargs='*', type=int, default=[],
                   help='With --sliding_window: axes to mirror every window along, 0 1 2 = D H W; every subset is one pass')
    return p.parse_args(argv)


def main(args):
    from medicalseg_amd.core import evaluate
    from medicalseg_amd.cvlibs import Config
    from medicalseg_amd.utils import load_entire_model, logger
    if not args.cfg:
        raise RuntimeError('No configuration file specified.')
    cfg = Config(args.cfg)
    val_dataset = cfg.val_dataset
    if val_dataset is None:
        raise RuntimeError('The verification dataset is not specified in the configuration file.')
    model = cfg.model
    if args.model_path:
        load_entire_model(model, args.model_path)
        logger.info('Loaded trained params of model successfully')
    print(evaluate(model, val_dataset, cfg.loss, num_workers=args.num_workers, print_detail=args.print_detail,
                   auc_roc=args.auc_roc, save_dir=args.save_dir, hard_metrics=args.hard_metrics, auc_device=args.auc_device,
                   surface_metrics=args.surface_metrics, aug_eval=args.aug_eval, scales=args.scales,
                   flip_axes=args.flip_axes, sliding_window=args.sliding_window, sw_overlap=args.sw_overlap,
                   sw_mode=args.sw_mode, sw_batch_size=args.sw_batch_size, sw_mirror_axes=args.sw_mirror_axes))


if __name__ == '__main__':
    main(parse_args())
