"""CLI: `python3 -m dnncancerannotator_amd {train,evaluate,predict} ...` (also reachable as `python3 -m annotator ...`).

Flag surface of the reference (README.md:16-120; runs/train.py:21-54, runs/evaluate.py:21-64), re-stated with argparse
because dsargparse (requirements.txt:11) is not available."""

import argparse
import logging
import sys

from .tta import MODES as TTA_MODES


def _at_least_one(text):
    n = int(text)
    if n < 1:
        raise argparse.ArgumentTypeError('must be at least 1, got %d' % n)
    return n


def _detection_arguments(p):
    """the candidate extraction shared by `evaluate --detection` and `predict --detection_map`; absent unless given"""
    p.add_argument('--detection_min_confidence', type=float, default=argparse.SUPPRESS,
                   help='the weakest peak that still starts a candidate, [0.001, 1] (default: 0.1)')
    p.add_argument('--detection_factor', type=float, default=argparse.SUPPRESS,
                   help='a candidate is the region around its peak above this fraction of the peak, [0.01, 1] (default: 0.4)')
    p.add_argument('--detection_max_candidates', type=int, default=argparse.SUPPRESS, help='candidates per slice, 1..64 (default: 5)')
    p.add_argument('--detection_min_area', type=int, default=argparse.SUPPRESS,
                   help='smallest region kept as a candidate, in pixels (default: 10)')
    p.add_argument('--detection_rounds', type=int, default=argparse.SUPPRESS,
                   help='peaks tried per slice, kept or dropped, max_candidates..256 (default: 16)')
    p.add_argument('--detection_link_min_overlap', type=int, default=argparse.SUPPRESS,
                   help='common pixels that join two candidates of neighbouring slices (default: 1)')
    p.add_argument('--detection_max_lesions', type=int, default=argparse.SUPPRESS,
                   help='rows per slice and plane of the table read from the map (default: 256)')


def _refine_arguments(p, what):
    """the mask refinement shared by `predict` and `evaluate`; absent unless given"""
    p.add_argument('--refine_hysteresis', type=float, default=argparse.SUPPRESS, metavar='LOW',
                   help='outline %s at LOW, in (0, 1) and below the threshold: the regions at LOW that hold a pixel at the '
                        'threshold (default: off)' % what)
    p.add_argument('--refine_closing', type=int, default=argparse.SUPPRESS, metavar='K',
                   help='close gaps below K pixels in %s after the opening: K x K closing, K odd, 3..15 (default: off)' % what)
    p.add_argument('--refine_fill_holes', action='store_true', default=argparse.SUPPRESS,
                   help='fill the holes of %s: background that does not reach the border of the slice' % what)


def build_parser(prog='python3 -m annotator'):
    parser = argparse.ArgumentParser(prog=prog, description='DNNAnnotator: DNN model to predict cancer segmentation (MI355X engine)')
    sub = parser.add_subparsers(dest='command', help='command')
    t = sub.add_parser('train', help='Train a model with specified configs.')
    t.add_argument('--config', nargs='+', required=True, help='configuration file path(s); later files overlay the first')
    t.add_argument('--save_path', required=True, help='where to save weights/configs/results')
    t.add_argument('--data_path', nargs='+', required=True, help='path to the data root dir')
    t.add_argument('--max_steps', type=int, required=True, help='max training steps')
    t.add_argument('--early_stop_steps', type=int, default=None, help='steps to train without improvements')
    t.add_argument('--save_freq', type=int, default=500, help='interval of checkpoints (default: 500 steps)')
    t.add_argument('--validate', action='store_true', help='also validate the model on the validation dataset')
    t.add_argument('--val_data_path', nargs='+', default=None, help='path to the validation dataset')
    t.add_argument('--visualize', action='store_true', help='should visualize results')
    t.add_argument('--profile', action='store_true', help='enable profiling')
    e = sub.add_parser('evaluate', help='Evaluate a model with specified configs for every checkpoints available.')
    e.add_argument('--save_path', required=True)
    e.add_argument('--data_path', nargs='+', required=True)
    e.add_argument('--tag', required=True, help='save tag')
    e.add_argument('--config', nargs='+', default=None)
    e.add_argument('--avoid_overwrite', action='store_true')
    e.add_argument('--export_path', default=None)
    e.add_argument('--export_images', action='store_true')
    e.add_argument('--export_csv', action='store_true')
    e.add_argument('--visualize_sensitivity', action='store_true')
    e.add_argument('--min_interval', type=int, default=1)
    e.add_argument('--step_range', type=int, nargs=2, default=None, help='"--step_range start end"')
    e.add_argument('--overlay', action='store_true')
    e.add_argument('--skip_visualization', action='store_true')
    e.add_argument('--export_casewise_metrics', action='store_true')
    # absent unless given (the defaults are those of runs.evaluate.evaluate)
    e.add_argument('--exam_lesions', action='store_true', default=argparse.SUPPRESS,
                   help='score the lesions linked through the slices of an exam against the labelled ones: also write '
                        'exam_lesion_results.csv, exam_lesion_cases.csv and exam_lesion_matches.csv')
    e.add_argument('--exam_threshold', type=float, nargs='+', default=argparse.SUPPRESS, metavar='T',
                   help='probability threshold(s) of --exam_lesions (default: 0.5)')
    e.add_argument('--exam_iou', type=float, default=argparse.SUPPRESS, help='3-D IoU at which two tumours hit (default: 0.30)')
    e.add_argument('--exam_min_area', type=int, default=argparse.SUPPRESS, help='smallest predicted lesion kept per slice (default: 0)')
    e.add_argument('--exam_filter_size', type=int, default=argparse.SUPPRESS, help='opening of the prediction, 1..15 (default: 5)')
    e.add_argument('--exam_resize_factor', type=float, default=argparse.SUPPRESS,
                   help='analyse probabilities and labels resized by this factor (default: 1.0)')
    e.add_argument('--exam_max_lesions', type=_at_least_one, default=argparse.SUPPRESS, help='lesions per slice and plane (default: 256)')
    e.add_argument('--exam_link_min_overlap', type=_at_least_one, default=argparse.SUPPRESS,
                   help='common pixels that join two lesions of neighbouring slices (default: 1)')
    e.add_argument('--surface_distances', action='store_true', default=argparse.SUPPRESS,
                   help='measure the predicted outline against the labelled one (Hausdorff, its percentile, ASSD, Dice): also write '
                        'surface_results.csv, surface_cases.csv and surface_slices.csv')
    e.add_argument('--surface_threshold', type=float, nargs='+', default=argparse.SUPPRESS, metavar='T',
                   help='probability threshold(s) of --surface_distances (default: 0.5)')
    e.add_argument('--surface_percentile', type=float, default=argparse.SUPPRESS, help='percentile of the distances reported beside '
                   'the largest (default: 95)')
    e.add_argument('--surface_min_area', type=int, default=argparse.SUPPRESS, help='smallest predicted lesion kept per slice (default: 0)')
    e.add_argument('--surface_filter_size', type=int, default=argparse.SUPPRESS, help='opening of the prediction, 1..15 (default: 5)')
    e.add_argument('--surface_resize_factor', type=float, default=argparse.SUPPRESS,
                   help='analyse probabilities and labels resized by this factor (default: 1.0)')
    e.add_argument('--surface_max_samples', type=_at_least_one, default=argparse.SUPPRESS,
                   help='boundary pixels per slice and side; a slice with more reports no distance (default: 65536)')
    e.add_argument('--tta', choices=TTA_MODES, default=argparse.SUPPRESS,
                   help='test-time augmentation: every probability read is the mean over the flip views (flips) or over all eight '
                        'flip / transpose views (d4, square slices only); default: none')
    e.add_argument('--uncertainty', action='store_true', default=argparse.SUPPRESS,
                   help='with --tta flips / d4 (or --ensemble): how much the views disagree (their standard deviation per pixel) on '
                        'wrong and on right pixels: also write uncertainty_results.csv and uncertainty_slices.csv')
    e.add_argument('--uncertainty_threshold', type=float, nargs='+', default=argparse.SUPPRESS, metavar='T',
                   help='probability threshold(s) of --uncertainty (default: 0.5)')
    e.add_argument('--calibration', action='store_true', default=argparse.SUPPRESS,
                   help='can the probability be believed: reliability table, ECE, MCE, Brier score, NLL and the temperature that '
                        'minimises the NLL: also write calibration_results.csv, calibration_bins.csv and calibration_slices.csv')
    e.add_argument('--calibration_bins', type=_at_least_one, default=argparse.SUPPRESS,
                   help='equal-width probability bins of --calibration, at most 256 (default: 15)')
    e.add_argument('--calibration_temperatures', type=float, nargs='+', default=argparse.SUPPRESS, metavar='T',
                   help='temperature grid of --calibration, each in [0.05, 20], at most 64 with T = 1, which is always added '
                        '(default: 41 points from 0.25 to 4)')
    e.add_argument('--temperature', type=float, default=argparse.SUPPRESS, metavar='T',
                   help='temperature scaling: every probability read is sigmoid(logit(p) / T), T in [0.05, 20]; --calibration then '
                        'measures the scaled probabilities (default: 1, no scaling)')
    e.add_argument('--visualize_attribution', action='store_true', default=argparse.SUPPRESS,
                   help='with --export_csv / --export_images: integrated-gradients attribution of every slice -- which modality, and '
                        'where in it, the prediction rests on: also write step_<step>_attribution.csv / .png per slice and '
                        'attribution_results.csv')
    e.add_argument('--attribution_steps', type=int, default=argparse.SUPPRESS, metavar='M',
                   help='path points of --visualize_attribution, 1..256; costs M + 2 forwards and M backward passes per batch (default: 32)')
    e.add_argument('--attribution_baseline', choices=('black', 'mean'), default=argparse.SUPPRESS,
                   help='where the path of --visualize_attribution starts: a zero image or the mean of each slice and modality '
                        '(default: black)')
    e.add_argument('--weights', choices=('raw', 'ema'), default=argparse.SUPPRESS,
                   help='which weights of each checkpoint to evaluate: the raw ones or their exponential moving average '
                        '(deploy_options.ema at training time; a checkpoint without one is an error); default: raw')
    e.add_argument('--detection', action='store_true', default=argparse.SUPPRESS,
                   help='lesion detection without a fixed threshold: ranked candidates from the detection map, lesion-level average '
                        'precision and FROC, exam-level AUROC: also write detection_results.csv, detection_froc.csv, '
                        'detection_cases.csv and detection_candidates.csv')
    _detection_arguments(e)
    e.add_argument('--detection_iou', type=float, default=argparse.SUPPRESS,
                   help='voxel IoU at which a candidate of --detection hits a tumour (default: 0.10)')
    e.add_argument('--bootstrap', type=int, default=argparse.SUPPRESS, metavar='R',
                   help='with --detection / --exam_lesions: resample the exams R times (100..1048576) on the GPU and also write '
                        'detection_bootstrap.csv, detection_bootstrap_replicates.csv and exam_lesion_bootstrap.csv: every figure with '
                        'the mean, deviation and interval of its replicates')
    e.add_argument('--bootstrap_seed', type=int, default=argparse.SUPPRESS,
                   help='seed of --bootstrap, 0..2^64-1; the same seed over the same data set resamples identically (default: 0)')
    e.add_argument('--bootstrap_level', type=float, default=argparse.SUPPRESS,
                   help='coverage of the intervals of --bootstrap, strictly between 0.5 and 1 (default: 0.95)')
    e.add_argument('--bootstrap_stratified', action='store_true', default=argparse.SUPPRESS,
                   help='--bootstrap with --detection: draw the exams with and without a labelled tumour separately')
    e.add_argument('--ensemble', nargs='+', default=argparse.SUPPRESS, metavar='MEMBER',
                   help='average further models on the GPU: MEMBER = RUN_DIR[:STEP], at most 15 (cross-validation folds, or snapshots '
                        'of one run: --ensemble RUN:800 RUN:900).  Every probability read is the mean over the checkpoint of '
                        '--save_path (member 0) and each member\'s checkpoint of the step being evaluated, or of its pinned STEP; '
                        '`loss` stays the loss of member 0\'s untransformed view.  Allows --uncertainty without --tta (the spread '
                        'between the members) and then also writes ensemble_uncertainty_results.csv')
    _refine_arguments(e, 'the predicted masks of --exam_lesions / --surface_distances')
    p = sub.add_parser('predict', help='Annotate slices that have no label: lesion tables and masks of one checkpoint.')
    p.add_argument('--save_path', required=True, help='the directory `train` wrote (options.yaml, checkpoints/)')
    p.add_argument('--data_path', nargs='+', required=True)
    p.add_argument('--output', required=True, help='where lesions.csv, slices.csv and the masks go')
    p.add_argument('--config', nargs='+', default=None)
    p.add_argument('--step', type=int, default=None, help='checkpoint step (default: the latest)')
    p.add_argument('--threshold', type=float, default=0.5, help='probability threshold (default: 0.5)')
    p.add_argument('--min_area', type=int, default=0, help='smallest lesion kept, in pixels of the analysed plane')
    p.add_argument('--filter_size', type=int, default=5, help='morphological opening, 1..15 (1: none; default: 5)')
    p.add_argument('--resize_factor', type=float, default=1.0, help='analyse the probabilities resized by this factor')
    p.add_argument('--max_lesions', type=int, default=256, help='lesions per slice in lesions.csv (default: 256)')
    p.add_argument('--export_images', action='store_true', help='also write <exam>/<slice>/mask.png')
    # absent unless given (the defaults are those of runs.predict.predict)
    p.add_argument('--link_slices', action='store_true', default=argparse.SUPPRESS,
                   help='join the lesions of neighbouring slices of an exam: also write exam_lesions.csv and exam_lesion_parts.csv')
    p.add_argument('--link_min_overlap', type=_at_least_one, default=argparse.SUPPRESS,
                   help='common pixels that join two lesions of neighbouring slices (default: 1)')
    p.add_argument('--tta', choices=TTA_MODES, default=argparse.SUPPRESS,
                   help='test-time augmentation: the lesions of the mean probability over the flip views (flips) or over all eight '
                        'flip / transpose views (d4, square slices only); default: none')
    p.add_argument('--uncertainty', action='store_true', default=argparse.SUPPRESS,
                   help='with --tta flips / d4: how much the views disagree (their standard deviation per pixel) per lesion and slice: '
                        'also write lesion_uncertainty.csv, slice_uncertainty.csv and, with --export_images, uncertainty.png')
    p.add_argument('--temperature', type=float, default=argparse.SUPPRESS, metavar='T',
                   help='temperature scaling: the tables and masks of sigmoid(logit(p) / T), T in [0.05, 20], e.g. the temperature '
                        '`evaluate --calibration` fitted (default: 1, no scaling)')
    p.add_argument('--lesion_features', action='store_true', default=argparse.SUPPRESS,
                   help='what every lesion looks like in the input modalities: also write lesion_features.csv (outline, axes, and per '
                        'modality mean, deviation, extrema, percentiles and the contrast against the tissue around the lesion) and, '
                        'with --link_slices, exam_lesion_features.csv')
    p.add_argument('--feature_bins', type=int, default=argparse.SUPPRESS, metavar='N',
                   help='histogram bins behind the percentiles of --lesion_features, 0..256 (0: no percentiles; default: 32)')
    p.add_argument('--feature_ring', type=int, default=argparse.SUPPRESS, metavar='R',
                   help='the tissue around a lesion of --lesion_features: background pixels within R pixels, 0..8 (0: none; default: 3)')
    p.add_argument('--weights', choices=('raw', 'ema'), default=argparse.SUPPRESS,
                   help='which weights of the checkpoint to annotate with: the raw ones or their exponential moving average '
                        '(deploy_options.ema at training time; a checkpoint without one is an error); default: raw')
    p.add_argument('--detection_map', action='store_true', default=argparse.SUPPRESS,
                   help='ranked lesion candidates without a fixed threshold: also write candidates.csv, slice_candidates.csv, with '
                        '--link_slices exam_candidates.csv and with --export_images detection.png (the map a detection challenge asks for)')
    _detection_arguments(p)
    p.add_argument('--ensemble', nargs='+', default=argparse.SUPPRESS, metavar='MEMBER',
                   help='average further models on the GPU: MEMBER = RUN_DIR[:STEP], at most 15 (cross-validation folds, or snapshots '
                        'of one run).  The tables and masks are those of the mean probability over the checkpoint of --save_path '
                        '(member 0) and each member\'s checkpoint: its pinned STEP, else --step, else its run\'s latest.  Allows '
                        '--uncertainty without --tta (the spread between the members) and then also writes '
                        'slice_ensemble_uncertainty.csv')
    _refine_arguments(p, 'the mask every table and mask.png reads')
    return parser


def main(argv=None, prog='python3 -m annotator'):
    logging.basicConfig(level=logging.INFO, format='%(levelname)s %(message)s')
    parser = build_parser(prog)
    args = vars(parser.parse_args(argv))
    command = args.pop('command')
    if command == 'train':
        from .runs.train import train
        train(**args)
    elif command == 'evaluate':
        from .runs.evaluate import evaluate
        rows = evaluate(**args)
        for step, r in (rows or {}).items():
            print(step, dict(r))
    elif command == 'predict':
        from .runs.predict import predict
        print(predict(**args))
    else:
        parser.print_help()
        return 2
    return 0


if __name__ == '__main__':
    sys.exit(main(prog='python3 -m dnncancerannotator_amd'))
