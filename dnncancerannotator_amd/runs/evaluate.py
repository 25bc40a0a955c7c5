"""`annotator evaluate` -- annotator/runs/evaluate.py:21-91: evaluate every checkpoint under save_path/checkpoints."""

import os

from .. import engine, load
from .train import make_dataset


def evaluate(save_path, data_path, tag, config=None, avoid_overwrite=False, export_path=None, export_images=False,
             export_csv=False, visualize_sensitivity=False, min_interval=1, step_range=None, overlay=False,
             skip_visualization=False, export_casewise_metrics=False, exam_lesions=False, exam_threshold=(0.5,), exam_iou=0.30,
             exam_min_area=0, exam_filter_size=5, exam_resize_factor=1.0, exam_max_lesions=256, exam_link_min_overlap=1,
             surface_distances=False, surface_threshold=(0.5,), surface_percentile=95.0, surface_min_area=0, surface_filter_size=5,
             surface_resize_factor=1.0, surface_max_samples=65536, tta='none', uncertainty=False, uncertainty_threshold=(0.5,),
             calibration=False, calibration_bins=15, calibration_temperatures=None, temperature=None, visualize_attribution=False,
             attribution_steps=None, attribution_baseline=None, weights='raw', detection=False, detection_min_confidence=None,
             detection_factor=None, detection_max_candidates=None, detection_min_area=None, detection_rounds=None, detection_iou=None,
             detection_link_min_overlap=None, detection_max_lesions=None, bootstrap=None, bootstrap_seed=None, bootstrap_level=None,
             bootstrap_stratified=False, ensemble=None, refine_hysteresis=None, refine_closing=None, refine_fill_holes=False):
    engine.check_uncertainty(uncertainty, tta, ensemble)       # before anything is read
    refine = engine.check_refine(refine_hysteresis, refine_closing, refine_fill_holes,      # likewise: below every threshold in use
                                 list(exam_threshold if exam_lesions else ()) + list(surface_threshold if surface_distances else ()),
                                 consumers=bool(exam_lesions or surface_distances))
    resampling = engine.check_bootstrap(bootstrap, bootstrap_seed, bootstrap_level, bootstrap_stratified, detection, exam_lesions)
    detection_values = dict(detection_min_confidence=detection_min_confidence, detection_factor=detection_factor,
                            detection_max_candidates=detection_max_candidates, detection_min_area=detection_min_area,
                            detection_rounds=detection_rounds, detection_iou=detection_iou,
                            detection_link_min_overlap=detection_link_min_overlap, detection_max_lesions=detection_max_lesions)
    engine.check_detection(detection, *detection_values.values())      # likewise, the --detection_* flags without --detection included
    if engine.check_weights(weights) == 'ema':       # likewise: the index of every checkpoint that will be evaluated
        engine.check_ema_checkpoints(engine.select_ckpts(engine.list_ckpts(os.path.join(save_path, 'checkpoints')), min_interval,
                                                         step_range).values())
    if ensemble:                         # likewise: every member's checkpoint for every step that will be evaluated
        ensemble = [engine.parse_member(m) for m in ensemble]
        visited = engine.select_ckpts(engine.list_ckpts(os.path.join(save_path, 'checkpoints')), min_interval, step_range)
        engine.check_ensemble(save_path, ensemble, list(visited), weights)
    attribution = engine.check_attribution(visualize_attribution, attribution_steps, attribution_baseline, export_csv, export_images)
    scaled = engine.check_temperature(temperature)   # likewise; None without the flag and with --temperature 1
    if calibration:
        engine.check_calibration(calibration_bins, calibration_temperatures)
    saved_config = load.load_config(os.path.join(save_path, 'options.yaml'))['config']
    if config:
        config = load._apply_config(saved_config, load.load_config(config))
    else:
        config = saved_config
    ds = make_dataset(data_path, config.get('data_options', {}).get('eval', {}), training=False)
    # the Visualizer's data set (runs/evaluate.py:72-73 of the reference): the same slices with their exam path and sliceID
    viz_ds = None if skip_visualization else make_dataset(data_path, config.get('data_options', {}).get('eval', {}), training=False,
                                                          include_meta=True)
    # --exam_lesions, --surface_distances, --uncertainty and --calibration read a data set of their own (the slices with their labels, exam path and sliceID;
    # --skip_visualization does not touch it): one is built and shared when several are given
    meta_ds = make_dataset(data_path, config.get('data_options', {}).get('eval', {}), training=False, include_meta=True) \
        if exam_lesions or surface_distances or uncertainty or calibration or detection else None
    exam_ds = meta_ds if exam_lesions else None
    # the keywords of --surface_distances go to model.eval only with the flag
    surface = dict(surface_ds=meta_ds, surface_distances=surface_distances, surface_threshold=surface_threshold,
                   surface_percentile=surface_percentile, surface_min_area=surface_min_area, surface_filter_size=surface_filter_size,
                   surface_resize_factor=surface_resize_factor, surface_max_samples=surface_max_samples) if surface_distances else {}
    more = dict(tta=tta) if tta != 'none' else {}      # the keyword of --tta goes to model.eval only with a mode
    if uncertainty:                      # likewise the keywords of --uncertainty only with the flag
        more.update(uncertainty_ds=meta_ds, uncertainty=True, uncertainty_thresholds=tuple(uncertainty_threshold))
    if calibration:                      # and those of --calibration
        more.update(calibration_ds=meta_ds, calibration=True, calibration_bins=int(calibration_bins),
                    calibration_temperatures=None if calibration_temperatures is None else tuple(calibration_temperatures))
    if scaled is not None:               # the keyword of --temperature only with a temperature other than 1
        more['temperature'] = scaled
    if attribution:                      # and those of --visualize_attribution only with the flag
        more.update(visualize_attribution=True, attribution_steps=attribution[0], attribution_baseline=attribution[1])
    if weights == 'ema':                 # and the keyword of --weights only with the averaged weights
        more['weights'] = 'ema'
    if detection:                        # and those of --detection only with the flag
        more.update(detection_ds=meta_ds, detection=True, **detection_values)
    if ensemble:                         # and that of --ensemble only with members
        more['ensemble'] = ensemble
    if refine:                           # and those of --refine_* only when they ask for something
        more.update(refine_hysteresis=refine_hysteresis, refine_closing=refine_closing, refine_fill_holes=refine_fill_holes)
    if resampling:                       # and those of --bootstrap
        more.update(bootstrap=resampling['replicates'], bootstrap_seed=resampling['seed'], bootstrap_level=resampling['level'],
                    bootstrap_stratified=resampling['stratified'])
    model = engine.TFKerasModel(config)
    return model.eval(ds, viz_ds=viz_ds, tag=tag, save_path=os.path.join(save_path), avoid_overwrite=avoid_overwrite,
                      export_path=export_path, export_images=export_images, export_csv=export_csv,
                      visualize_sensitivity=visualize_sensitivity, min_interval=min_interval, step_range=step_range,
                      overlay=overlay, export_casewise_metrics=export_casewise_metrics, exam_ds=exam_ds, exam_lesions=exam_lesions,
                      exam_threshold=exam_threshold, exam_iou=exam_iou, exam_min_area=exam_min_area, exam_filter_size=exam_filter_size,
                      exam_resize_factor=exam_resize_factor, exam_max_lesions=exam_max_lesions,
                      exam_link_min_overlap=exam_link_min_overlap, **surface, **more)
