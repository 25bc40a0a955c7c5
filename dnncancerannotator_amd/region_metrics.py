"""Region-based (lesion-level) metrics (annotator/utils/metrics.py:80-510; the region/* entries of configs/additionals/metrics.yaml).

The counts -- label components detected (tp_label) or missed (fn), prediction components that match a lesion (tp_pred) or not (fp),
IoU > IoU_threshold after a k x k morphological opening of the prediction -- are computed on the GPU (kernels_region.hip; include/
dnnca.h dnnca_region_confusion*, dnnca_eval_region_*).  This module holds the seven metric classes, which turn the counts into the
reference's float32 results, and the spec grouping: metrics that differ only in class or name (metrics.yaml's seven region entries)
share one device spec.  Turned on by `deploy_options.region_metrics: device` (engine.TFKerasModel.from_config)."""

from collections import OrderedDict

import numpy as np

MAX_THRESHOLDS = 64      # include/dnnca.h: 1..64 thresholds per spec


def _f32(v):
    return np.float32(v)


class _RegionBasedMetric:
    """metrics.py:80-104 _RegionBasedMetric: thresholds (>= 0), IoU_threshold, epsilon, resize_factor, morph_filter_size."""

    def __init__(self, thresholds, IoU_threshold=0.30, epsilon=1e-07, resize_factor=1.0, morph_filter_size=5, name=None, **kw):
        thr = np.atleast_1d(np.asarray(thresholds, np.float32)).ravel()
        if not 1 <= thr.size <= MAX_THRESHOLDS:
            raise ValueError('region metrics take 1..%d thresholds, got %d' % (MAX_THRESHOLDS, thr.size))
        if not np.all(thr >= 0):                    # metrics.py:96 tf.debugging.assert_non_negative (NaN fails too)
            raise ValueError('region metric thresholds must be >= 0: %s' % thr)
        iou = float(IoU_threshold)
        if not 0.0 <= iou < 1.0:
            raise ValueError('IoU_threshold must lie in [0, 1), got %r' % IoU_threshold)
        if not float(resize_factor) > 0:
            raise ValueError('resize_factor must be > 0, got %r' % resize_factor)
        if not 1 <= int(morph_filter_size) <= 15:
            raise ValueError('morph_filter_size must lie in 1..15, got %r' % morph_filter_size)
        self.thresholds = thr
        self.IoU_threshold, self.epsilon = iou, float(epsilon)
        self.resize_factor, self.morph_filter_size = float(resize_factor), int(morph_filter_size)
        self.name = name or type(self).__name__
        self.reset_state()

    @property
    def spec(self):
        """the device spec (thresholds, IoU threshold, resize factor, filter size): equal for metrics that share their counts"""
        return (tuple(float(t) for t in self.thresholds), float(_f32(self.IoU_threshold)), float(_f32(self.resize_factor)),
                self.morph_filter_size)

    def reset_state(self):
        self.counts = np.zeros((len(self.thresholds), 4), np.int64)      # tp_label, fn, tp_pred, fp

    def add_counts(self, counts):
        self.counts += np.asarray(counts, np.int64).reshape(self.counts.shape)

    def update_state(self, device_model, y):
        """counts of the probabilities of the model's last forward / eval step against y [B, H, W]"""
        self.add_counts(device_model.region_confusion(y, self.spec))

    def merge(self, reduce_fn):
        self.counts = np.rint(np.asarray(reduce_fn(self.counts.astype(np.float64)))).astype(np.int64).reshape(self.counts.shape)

    # float32 formulas of the reference (tf.cast(count, float32) / (tf.cast(sum, float32) + epsilon)); squeezed when T = 1
    def _recall(self):
        tp, fn = self.counts[:, 0], self.counts[:, 1]
        return tp.astype(np.float32) / ((tp + fn).astype(np.float32) + _f32(self.epsilon))

    def _precision(self, tp_col=2):
        tp, fp = self.counts[:, tp_col], self.counts[:, 3]
        return tp.astype(np.float32) / ((tp + fp).astype(np.float32) + _f32(self.epsilon))

    @staticmethod
    def _squeeze(r):
        r = np.asarray(r)
        if r.size == 1:
            return r.reshape(()).item()
        return [v.item() for v in r]


class RegionBasedRecall(_RegionBasedMetric):
    """metrics.py:345-369: tp_label / (tp_label + fn + eps)"""

    def result(self):
        return self._squeeze(self._recall())


class RegionBasedPrecision(_RegionBasedMetric):
    """metrics.py:372-396: prediction-side tp / (tp + fp + eps) (get_tp_fp, :237-254)"""

    def result(self):
        return self._squeeze(self._precision())


class RegionBasedTruePositives(_RegionBasedMetric):
    """metrics.py:399-419: label components detected"""

    def result(self):
        return self._squeeze(self.counts[:, 0])


class RegionBasedFalsePositives(_RegionBasedMetric):
    """metrics.py:422-442: prediction components that match no label component"""

    def result(self):
        return self._squeeze(self.counts[:, 3])


class RegionBasedFalseNegatives(_RegionBasedMetric):
    """metrics.py:445-465: label components missed"""

    def result(self):
        return self._squeeze(self.counts[:, 1])


class RegionBasedFBetaScore(_RegionBasedMetric):
    """metrics.py:313-343 on FBetaScore (:37-77): (1 + b^2) P R / (b^2 P + R + eps) of the region precision and recall.  The
    reference builds its precision / recall without morph_filter_size: the default 5."""

    def __init__(self, beta, thresholds, IoU_threshold=0.30, epsilon=1e-07, resize_factor=1.0, name=None, **kw):
        assert beta > 0
        kw.pop('morph_filter_size', None)
        super().__init__(thresholds, IoU_threshold, epsilon, resize_factor, 5, name=name)
        self.beta = float(beta)

    def result(self):
        p, r = self._precision(), self._recall()
        b2 = self.beta ** 2
        s = _f32(1 + b2) * p * r / (_f32(b2) * p + r + _f32(self.epsilon))
        return self._squeeze(s)


class RegionBasedConfusionMatrix(_RegionBasedMetric):
    """metrics.py:468-510: result() is NaN; result_dict() has the three counts and recall / precision from the LABEL-side tp."""

    def result(self):
        return float('nan')

    def result_dict(self):
        tp, fn, fp = self.counts[:, 0], self.counts[:, 1], self.counts[:, 3]
        eps = _f32(self.epsilon)
        return {
            'true_positive_counts': self._squeeze(tp),
            'false_positive_counts': self._squeeze(fp),
            'false_negative_counts': self._squeeze(fn),
            'recall': self._squeeze(tp.astype(np.float32) / ((tp + fn).astype(np.float32) + eps)),
            'precision': self._squeeze(tp.astype(np.float32) / ((tp + fp).astype(np.float32) + eps)),
        }


_REGISTRY = {c.__name__: c for c in (RegionBasedRecall, RegionBasedPrecision, RegionBasedTruePositives, RegionBasedFalsePositives,
                                     RegionBasedFalseNegatives, RegionBasedFBetaScore, RegionBasedConfusionMatrix)}


def is_region_spec(metric_spec):
    name = metric_spec if isinstance(metric_spec, str) else (list(metric_spec)[0] if isinstance(metric_spec, dict) and
                                                             len(metric_spec) == 1 else '')
    return name.startswith('RegionBased')


def solve_region_metric(metric_spec):
    """{ClassName: {kwargs}} -> region metric instance; None for a metric that is not region-based"""
    if not is_region_spec(metric_spec):
        return None
    if isinstance(metric_spec, str):
        metric_spec = {metric_spec: {}}
    name, options = list(metric_spec.items())[0]
    if name not in _REGISTRY:
        raise ValueError(f'Unknown metric: {name}')
    return _REGISTRY[name](**dict(options or {}))


def group_by_spec(metrics):
    """[(device spec, [metrics sharing it])] in first-appearance order: one device computation per distinct spec"""
    groups = OrderedDict()
    for m in metrics:
        groups.setdefault(m.spec, []).append(m)
    return list(groups.items())
