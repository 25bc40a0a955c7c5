"""`annotator predict` -- the reference left annotator/runs/predict.py empty: annotate slices that have no label with a trained
checkpoint (lesions.csv, slices.csv and, with --export_images, one mask.png per slice; with --link_slices also exam_lesions.csv and
exam_lesion_parts.csv: the lesions joined through the slices of an exam; with --tta MODE --uncertainty also lesion_uncertainty.csv,
slice_uncertainty.csv and uncertainty.png: how much the views disagree; with --temperature T every table reads the probabilities
scaled by T; with --lesion_features also lesion_features.csv and, with --link_slices, exam_lesion_features.csv: outline, axes and
per modality the intensities in and around every lesion; with --detection_map also candidates.csv, slice_candidates.csv, with
--link_slices exam_candidates.csv and with --export_images detection.png: ranked lesion candidates without a fixed threshold; with
--ensemble MEMBER ... every table reads the mean probability over the members' checkpoints, and with --uncertainty also
slice_ensemble_uncertainty.csv is written; with --refine_hysteresis LOW, --refine_closing K and --refine_fill_holes every table and
mask.png reads the refined mask; engine.TFKerasModel.annotate)."""

import os

from .. import casewise, engine, load
from .train import make_dataset


def predict(save_path, data_path, output, config=None, step=None, threshold=0.5, min_area=0, filter_size=5, resize_factor=1.0,
            max_lesions=256, export_images=False, link_slices=False, link_min_overlap=1, tta='none', uncertainty=False,
            temperature=None, lesion_features=False, feature_bins=None, feature_ring=None, weights='raw', detection_map=False,
            detection_min_confidence=None, detection_factor=None, detection_max_candidates=None, detection_min_area=None,
            detection_rounds=None, detection_link_min_overlap=None, detection_max_lesions=None, ensemble=None, refine_hysteresis=None,
            refine_closing=None, refine_fill_holes=False):
    engine.check_uncertainty(uncertainty, tta, ensemble)       # before anything is read
    refine = engine.check_refine(refine_hysteresis, refine_closing, refine_fill_holes, [threshold])      # likewise
    detection_values = dict(detection_min_confidence=detection_min_confidence, detection_factor=detection_factor,
                            detection_max_candidates=detection_max_candidates, detection_min_area=detection_min_area,
                            detection_rounds=detection_rounds, detection_link_min_overlap=detection_link_min_overlap,
                            detection_max_lesions=detection_max_lesions)
    engine.check_detection(detection_map, detection_min_confidence, detection_factor, detection_max_candidates, detection_min_area,
                           detection_rounds, None, detection_link_min_overlap, detection_max_lesions, flag='--detection_map')      # likewise
    if engine.check_weights(weights) == 'ema':       # likewise: the index of the checkpoint that will be read
        ckpts = engine.list_ckpts(os.path.join(save_path, 'checkpoints'))
        if ckpts and (step is None or step in ckpts):          # (a missing checkpoint is annotate's error, as without the flag)
            engine.check_ema_checkpoints([ckpts[max(ckpts) if step is None else step]])
    if ensemble:                         # likewise: every member's checkpoint (a missing one of save_path is annotate's error)
        ensemble = [engine.parse_member(m) for m in ensemble]
        engine.check_ensemble(save_path, ensemble, [step], weights)
    casewise.check_features(lesion_features, feature_bins, feature_ring)      # likewise
    scaled = engine.check_temperature(temperature)   # likewise; None without the flag and with --temperature 1
    if link_min_overlap < 1:
        raise ValueError('link_min_overlap must be at least 1, got %d' % link_min_overlap)
    saved_config = load.load_config(os.path.join(save_path, 'options.yaml'))['config']
    config = load._apply_config(saved_config, load.load_config(config)) if config else saved_config
    ds = make_dataset(data_path, config.get('data_options', {}).get('eval', {}), training=False, include_meta=True, labels=False)
    # the keyword of --tta goes to model.annotate only with a mode (tta.mask_of refuses d4 on non-square slices there, before any
    # checkpoint is read)
    more = dict(tta=tta) if tta != 'none' else {}
    if uncertainty:                      # likewise only with the flag
        more['uncertainty'] = True
    if scaled is not None:               # and the keyword of --temperature only with a temperature other than 1
        more['temperature'] = scaled
    if lesion_features:                  # and the keywords of --lesion_features only with the flag
        more.update(lesion_features=True, feature_bins=feature_bins, feature_ring=feature_ring)
    if weights == 'ema':                 # and the keyword of --weights only with the averaged weights
        more['weights'] = 'ema'
    if ensemble:                         # and that of --ensemble only with members
        more['ensemble'] = ensemble
    if detection_map:                    # and those of --detection_map only with the flag
        more.update(detection_map=True, **detection_values)
    if refine:                           # and those of --refine_* only when they ask for something
        more.update(refine_hysteresis=refine_hysteresis, refine_closing=refine_closing, refine_fill_holes=refine_fill_holes)
    model = engine.TFKerasModel(config)
    return model.annotate(ds, save_path=save_path, output=output, step=step, threshold=threshold, min_area=min_area,
                          filter_size=filter_size, resize_factor=resize_factor, max_lesions=max_lesions,
                          export_images=export_images, link_slices=link_slices, link_min_overlap=link_min_overlap, **more)
