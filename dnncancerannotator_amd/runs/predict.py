"""`annotator predict` -- the reference left annotator/runs/predict.py empty: annotate slices that have no label with a trained
checkpoint (lesions.csv, slices.csv and, with --export_images, one mask.png per slice; engine.TFKerasModel.annotate)."""

import os

from .. import engine, load
from .train import make_dataset


def predict(save_path, data_path, output, config=None, step=None, threshold=0.5, min_area=0, filter_size=5, resize_factor=1.0,
            max_lesions=256, export_images=False):
    saved_config = load.load_config(os.path.join(save_path, 'options.yaml'))['config']
    config = load._apply_config(saved_config, load.load_config(config)) if config else saved_config
    ds = make_dataset(data_path, config.get('data_options', {}).get('eval', {}), training=False, include_meta=True, labels=False)
    model = engine.TFKerasModel(config)
    return model.annotate(ds, save_path=save_path, output=output, step=step, threshold=threshold, min_area=min_area,
                          filter_size=filter_size, resize_factor=resize_factor, max_lesions=max_lesions,
                          export_images=export_images)
