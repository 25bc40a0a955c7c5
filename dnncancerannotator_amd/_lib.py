"""ctypes binding of libdnnca.so (include/dnnca.h).  The only bridge between the Python host and the HIP engine.

There is no CPU fallback: if the library is missing or no GPU is present, the calls fail loudly."""

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DNNCA_LIB') or os.path.join(HERE, 'libdnnca.so')      # DNNCA_LIB: A/B of two builds (development aid)

OK = 0
ARCH_UNET, ARCH_MULMO, ARCH_MULTIRES = 0, 1, 2
PAD_VALID, PAD_SAME = 0, 1
F32, BF16 = 0, 1
UNIQUE_ID_BYTES = 128
FLAG_GENERIC = 1


class DnncaError(RuntimeError):
    def __init__(self, code, message):
        super().__init__('libdnnca error %d: %s' % (code, message))
        self.code = code


class ModelDesc(C.Structure):
    _fields_ = [
        ('arch', C.c_int32), ('in_channels', C.c_int32), ('height', C.c_int32), ('width', C.c_int32),
        ('max_batch', C.c_int32), ('n_filters_first', C.c_int32), ('n_downsample', C.c_int32), ('rate', C.c_int32),
        ('kernel_size', C.c_int32), ('conv_stride', C.c_int32), ('bn', C.c_int32), ('padding', C.c_int32),
        ('reference_index', C.c_int32), ('n_conv', C.c_int32), ('leaky_alpha', C.c_float), ('l2', C.c_float),
        ('dtype', C.c_int32), ('flags', C.c_int32),
    ]


class LossCfg(C.Structure):
    _fields_ = [('has_weight', C.c_int32), ('weight', C.c_float), ('weight_add', C.c_float), ('weight_mul', C.c_float),
                ('label_smoothing', C.c_int32), ('label_smoothing_filter_size', C.c_int32), ('label_smoothing_sigma', C.c_float)]


class RegionLoss(C.Structure):                     # dnnca_region_loss
    _fields_ = [('region_weight', C.c_float), ('crossentropy_weight', C.c_float), ('alpha', C.c_float), ('beta', C.c_float),
                ('smooth', C.c_float)]


class LesionRefine(C.Structure):                   # dnnca_lesion_refine
    _fields_ = [('hysteresis_low', C.c_float), ('closing_size', C.c_int32), ('fill_holes', C.c_int32)]


class OptimizerCfg(C.Structure):                   # dnnca_optimizer_cfg
    _fields_ = [('kind', C.c_int32), ('beta1', C.c_float), ('beta2', C.c_float), ('epsilon', C.c_float), ('momentum', C.c_float),
                ('nesterov', C.c_int32), ('weight_decay', C.c_float), ('clipvalue', C.c_float), ('clipnorm', C.c_float),
                ('global_clipnorm', C.c_float)]


OPT_ADAM, OPT_ADAMW, OPT_SGD = 0, 1, 2


class StepOut(C.Structure):
    _fields_ = [('loss', C.c_float), ('positive_rate', C.c_float), ('weight', C.c_float),
                ('label_min', C.c_float), ('label_max', C.c_float)]


INTENSITY_WORDS = 32                               # uint32 words of a random_intensity record (include/dnnca.h)


class AugParam(C.Structure):                       # dnnca_aug_param
    _fields_ = [('dy', C.c_int32), ('dx', C.c_int32), ('flip', C.c_int32), ('contrast', C.c_float)]


class Confusion(C.Structure):
    _fields_ = [('tp', C.c_double), ('fp', C.c_double), ('fn', C.c_double), ('tn', C.c_double)]


class RegionSpec(C.Structure):                     # dnnca_region_spec
    _fields_ = [('thresholds', C.POINTER(C.c_float)), ('n_thresholds', C.c_int32), ('iou_threshold', C.c_float),
                ('resize_factor', C.c_float), ('morph_filter_size', C.c_int32)]


class RegionCounts(C.Structure):                   # dnnca_region_counts
    _fields_ = [('tp_label', C.c_int64), ('fn', C.c_int64), ('tp_pred', C.c_int64), ('fp', C.c_int64)]


class LesionRow(C.Structure):                      # dnnca_lesion_row (56 bytes, no padding)
    _fields_ = [('slice', C.c_int32), ('row', C.c_int32), ('area', C.c_int32), ('x0', C.c_int32), ('y0', C.c_int32),
                ('x1', C.c_int32), ('y1', C.c_int32), ('max_prob', C.c_float), ('sum_x', C.c_uint64), ('sum_y', C.c_uint64),
                ('sum_prob_q24', C.c_uint64)]


# the same record as a numpy dtype: DeviceModel.lesion_table returns its rows as a structured array
LESION_ROW_DTYPE = np.dtype([('slice', '<i4'), ('row', '<i4'), ('area', '<i4'), ('x0', '<i4'), ('y0', '<i4'), ('x1', '<i4'),
                             ('y1', '<i4'), ('max_prob', '<f4'), ('sum_x', '<u8'), ('sum_y', '<u8'), ('sum_prob_q24', '<u8')])


class LesionLink(C.Structure):                     # dnnca_lesion_link (16 bytes)
    _fields_ = [('slice', C.c_int32), ('row_prev', C.c_int32), ('row', C.c_int32), ('overlap', C.c_int32)]


# DeviceModel.lesion_table_linked returns its links as a structured array of this dtype
LESION_LINK_DTYPE = np.dtype([('slice', '<i4'), ('row_prev', '<i4'), ('row', '<i4'), ('overlap', '<i4')])



class LesionPair(C.Structure):                     # dnnca_lesion_pair (16 bytes)
    _fields_ = [('slice', C.c_int32), ('row_true', C.c_int32), ('row', C.c_int32), ('overlap', C.c_int32)]


# DeviceModel.lesion_table_matched returns its pairs as a structured array of this dtype
LESION_PAIR_DTYPE = np.dtype([('slice', '<i4'), ('row_true', '<i4'), ('row', '<i4'), ('overlap', '<i4')])


class SurfaceSample(C.Structure):                  # dnnca_surface_sample (16 bytes)
    _fields_ = [('slice', C.c_int32), ('side', C.c_int32), ('pixel', C.c_int32), ('d2', C.c_int32)]


# DeviceModel.surface_distances returns its samples as a structured array of this dtype
SURFACE_SAMPLE_DTYPE = np.dtype([('slice', '<i4'), ('side', '<i4'), ('pixel', '<i4'), ('d2', '<i4')])


class LesionSpread(C.Structure):                   # dnnca_lesion_spread (24 bytes, no padding)
    _fields_ = [('slice', C.c_int32), ('row', C.c_int32), ('area', C.c_int32), ('max_spread', C.c_float), ('sum_spread_q24', C.c_uint64)]


class SliceSpread(C.Structure):                    # dnnca_slice_spread (16 bytes, no padding)
    _fields_ = [('pixels', C.c_int32), ('max_spread', C.c_float), ('sum_spread_q24', C.c_uint64)]


class LesionShape(C.Structure):                    # dnnca_lesion_shape (48 bytes, no padding)
    _fields_ = [('slice', C.c_int32), ('row', C.c_int32), ('area', C.c_int32), ('boundary', C.c_int32), ('edges', C.c_int32),
                ('reserved', C.c_int32), ('sum_xx', C.c_uint64), ('sum_yy', C.c_uint64), ('sum_xy', C.c_uint64)]


class LesionIntensity(C.Structure):                # dnnca_lesion_intensity (40 bytes, no padding): a body or a ring record
    _fields_ = [('slice', C.c_int32), ('row', C.c_int32), ('channel', C.c_int32), ('n', C.c_int32), ('min', C.c_float),
                ('max', C.c_float), ('sum_q16', C.c_uint64), ('sum_sq_q16', C.c_uint64)]


class SpreadOutcome(C.Structure):                  # dnnca_spread_outcome (64 bytes): classes TN, FP, FN, TP
    _fields_ = [('n', C.c_uint64 * 4), ('sum_q24', C.c_uint64 * 4)]


class CalibBin(C.Structure):                       # dnnca_calib_bin (32 bytes): classes 0 (y <= 0.5) and 1
    _fields_ = [('n', C.c_uint64 * 2), ('sum_q24', C.c_uint64 * 2)]


class CalibTotal(C.Structure):                     # dnnca_calib_total (64 bytes): sum q^2 = sq_hi * 2^32 + sq_lo
    _fields_ = [('n', C.c_uint64 * 2), ('sum_q24', C.c_uint64 * 2), ('sq_lo', C.c_uint64 * 2), ('sq_hi', C.c_uint64 * 2)]


# DeviceModel.calibration returns structured arrays of these dtypes
CALIB_BIN_DTYPE = np.dtype([('n', '<u8', (2,)), ('sum_q24', '<u8', (2,))])
CALIB_TOTAL_DTYPE = np.dtype([('n', '<u8', (2,)), ('sum_q24', '<u8', (2,)), ('sq_lo', '<u8', (2,)), ('sq_hi', '<u8', (2,))])
CALIB_MAX_BINS, CALIB_MAX_TEMPERATURES = 256, 64
CALIB_MIN_T, CALIB_MAX_T = 0.05, 20.0              # the temperatures the library accepts


class DetectionCfg(C.Structure):                   # dnnca_detection_cfg
    _fields_ = [('min_confidence', C.c_float), ('factor', C.c_float), ('max_candidates', C.c_int32), ('min_area', C.c_int32),
                ('rounds', C.c_int32)]


class DetectionRow(C.Structure):                   # dnnca_detection_row (20 bytes)
    _fields_ = [('slice', C.c_int32), ('number', C.c_int32), ('seed', C.c_int32), ('area', C.c_int32), ('confidence', C.c_float)]


class DetectionSlice(C.Structure):                 # dnnca_detection_slice (16 bytes)
    _fields_ = [('candidates', C.c_int32), ('rounds', C.c_int32), ('dropped', C.c_int32), ('exhausted', C.c_int32)]


# DeviceModel.detection_map / detection_map_of return structured arrays of these dtypes
DETECTION_ROW_DTYPE = np.dtype([('slice', '<i4'), ('number', '<i4'), ('seed', '<i4'), ('area', '<i4'), ('confidence', '<f4')])
DETECTION_SLICE_DTYPE = np.dtype([('candidates', '<i4'), ('rounds', '<i4'), ('dropped', '<i4'), ('exhausted', '<i4')])


class BootstrapExam(C.Structure):                  # dnnca_bootstrap_exam (8 bytes)
    _fields_ = [('tumours', C.c_int32), ('score_rank', C.c_int32)]


class BootstrapCandidate(C.Structure):             # dnnca_bootstrap_candidate (12 bytes)
    _fields_ = [('exam', C.c_int32), ('hit', C.c_int32), ('level', C.c_int32)]


class BootstrapDetectionRow(C.Structure):          # dnnca_bootstrap_detection_row (120 bytes)
    _fields_ = [('positive_exams', C.c_int64), ('tumours', C.c_int64), ('candidates', C.c_int64), ('tp', C.c_int64), ('fp', C.c_int64),
                ('auroc_pairs', C.c_int64), ('auroc_twice', C.c_int64), ('tp_at', C.c_int64 * 7), ('ap', C.c_double)]


# DeviceModel.bootstrap_detection takes and returns structured arrays of these dtypes
BOOTSTRAP_EXAM_DTYPE = np.dtype([('tumours', '<i4'), ('score_rank', '<i4')])
BOOTSTRAP_CANDIDATE_DTYPE = np.dtype([('exam', '<i4'), ('hit', '<i4'), ('level', '<i4')])
BOOTSTRAP_DETECTION_ROW_DTYPE = np.dtype([('positive_exams', '<i8'), ('tumours', '<i8'), ('candidates', '<i8'), ('tp', '<i8'),
                                          ('fp', '<i8'), ('auroc_pairs', '<i8'), ('auroc_twice', '<i8'), ('tp_at', '<i8', (7,)),
                                          ('ap', '<f8')])
BOOTSTRAP_TILE = 1024                              # DNNCA_BOOTSTRAP_TILE: candidates per step of the detection kernel
BOOTSTRAP_MAX_EXAMS, BOOTSTRAP_MAX_CANDIDATES, BOOTSTRAP_MAX_REPLICATES = 16384, 1 << 22, 1 << 20
BOOTSTRAP_MAX_COLUMNS, BOOTSTRAP_MAX_STRATA = 64, 8


# DeviceModel.lesion_table_spread / spread_by_outcome return structured arrays of these dtypes
LESION_SPREAD_DTYPE = np.dtype([('slice', '<i4'), ('row', '<i4'), ('area', '<i4'), ('max_spread', '<f4'), ('sum_spread_q24', '<u8')])
SLICE_SPREAD_DTYPE = np.dtype([('pixels', '<i4'), ('max_spread', '<f4'), ('sum_spread_q24', '<u8')])
SPREAD_OUTCOME_DTYPE = np.dtype([('n', '<u8', (4,)), ('sum_q24', '<u8', (4,))])
# DeviceModel.lesion_table_features returns structured arrays of these dtypes
LESION_SHAPE_DTYPE = np.dtype([('slice', '<i4'), ('row', '<i4'), ('area', '<i4'), ('boundary', '<i4'), ('edges', '<i4'),
                               ('reserved', '<i4'), ('sum_xx', '<u8'), ('sum_yy', '<u8'), ('sum_xy', '<u8')])
LESION_INTENSITY_DTYPE = np.dtype([('slice', '<i4'), ('row', '<i4'), ('channel', '<i4'), ('n', '<i4'), ('min', '<f4'), ('max', '<f4'),
                                   ('sum_q16', '<u8'), ('sum_sq_q16', '<u8')])
FEATURE_MAX_BINS, FEATURE_MAX_RING, FEATURE_MAX_CHANNELS = 256, 8, 16


class LesionPlaneOut(C.Structure):                 # dnnca_lesion_plane_out: buffers and capacities in, counts out
    _fields_ = [('rows', C.POINTER(LesionRow)), ('rows_capacity', C.c_int64), ('n_rows', C.c_int64), ('totals', C.POINTER(C.c_int32)),
                ('links', C.POINTER(LesionLink)), ('links_capacity', C.c_int64), ('n_links', C.c_int64)]


class LesionPairsOut(C.Structure):                 # dnnca_lesion_pairs_out
    _fields_ = [('pairs', C.POINTER(LesionPair)), ('capacity', C.c_int64), ('n_pairs', C.c_int64)]


_FP = C.POINTER(C.c_float)
_VP = C.c_void_p

# name -> (restype, argtypes); mirrors include/dnnca.h one to one
SIGNATURES = {
    'dnnca_version': (C.c_char_p, []),
    'dnnca_last_error': (C.c_char_p, []),
    'dnnca_device_count': (C.c_int, [C.POINTER(C.c_int)]),
    'dnnca_init': (C.c_int, [C.c_int]),
    'dnnca_model_create': (C.c_int, [C.POINTER(ModelDesc), C.POINTER(_VP)]),
    'dnnca_model_destroy': (C.c_int, [_VP]),
    'dnnca_param_count': (C.c_int, [_VP, C.POINTER(C.c_int)]),
    'dnnca_param_info': (C.c_int, [_VP, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    'dnnca_num_trainable': (C.c_int, [_VP, C.POINTER(C.c_int64)]),
    'dnnca_num_state': (C.c_int, [_VP, C.POINTER(C.c_int64)]),
    'dnnca_set_params': (C.c_int, [_VP, _FP, C.c_int64]),
    'dnnca_get_params': (C.c_int, [_VP, _FP, C.c_int64]),
    'dnnca_set_state': (C.c_int, [_VP, _FP, C.c_int64]),
    'dnnca_get_state': (C.c_int, [_VP, _FP, C.c_int64]),
    'dnnca_get_grads': (C.c_int, [_VP, _FP, C.c_int64]),
    'dnnca_set_opt_state': (C.c_int, [_VP, _FP, _FP, C.c_int64, C.c_int64]),
    'dnnca_get_opt_state': (C.c_int, [_VP, _FP, _FP, C.c_int64, C.POINTER(C.c_int64)]),
    'dnnca_set_adam': (C.c_int, [_VP, C.c_float, C.c_float, C.c_float]),
    'dnnca_model_set_optimizer': (C.c_int, [_VP, C.POINTER(OptimizerCfg), C.POINTER(C.c_uint8), C.c_int]),
    'dnnca_last_grad_norm': (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]),
    'dnnca_apply_gradients': (C.c_int, [_VP, _FP, C.c_int64, C.c_float]),
    'dnnca_model_set_accumulation': (C.c_int, [_VP, C.c_int]),
    'dnnca_get_accumulation': (C.c_int, [_VP, _FP, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'dnnca_grad_accumulate_of': (C.c_int, [_VP, _FP, _FP, C.c_int64, C.c_int, _FP]),
    'dnnca_model_set_ema': (C.c_int, [_VP, C.c_float, C.c_int]),
    'dnnca_get_ema': (C.c_int, [_VP, _FP, C.c_int64, C.POINTER(C.c_int64)]),
    'dnnca_set_ema_state': (C.c_int, [_VP, _FP, C.c_int64, C.c_int64]),
    'dnnca_ema_exchange': (C.c_int, [_VP]),
    'dnnca_forward': (C.c_int, [_VP, _FP, C.c_int, C.c_int, _FP, _FP]),
    'dnnca_forward_tta': (C.c_int, [_VP, _FP, C.c_int, C.c_uint, _FP]),
    'dnnca_tta_view_of': (C.c_int, [_VP, _FP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _FP]),
    'dnnca_tta_mean_of': (C.c_int, [_VP, _FP, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, _FP]),
    'dnnca_forward_tta_spread': (C.c_int, [_VP, _FP, C.c_int, C.c_uint, _FP, _FP]),
    'dnnca_tta_spread_of': (C.c_int, [_VP, _FP, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, _FP, _FP]),
    'dnnca_get_tta_spread': (C.c_int, [_VP, C.c_int, _FP]),
    'dnnca_model_set_members': (C.c_int, [_VP, C.c_int]),
    'dnnca_member_store': (C.c_int, [_VP, C.c_int, _FP, C.c_int64, _FP, C.c_int64]),
    'dnnca_member_get': (C.c_int, [_VP, C.c_int, _FP, _FP]),
    'dnnca_forward_ensemble': (C.c_int, [_VP, _FP, C.c_int, C.c_uint, C.c_int, _FP]),
    'dnnca_get_ensemble_spread': (C.c_int, [_VP, C.c_int, _FP, _FP]),
    'dnnca_ensemble_of': (C.c_int, [_VP, _FP, _FP, C.c_int, C.c_int, C.c_int, C.c_int, _FP, _FP, _FP, _FP]),
    'dnnca_train_step': (C.c_int, [_VP, _FP, _FP, C.c_int, C.c_float, C.POINTER(LossCfg), C.POINTER(StepOut)]),
    'dnnca_eval_step': (C.c_int, [_VP, _FP, _FP, C.c_int, C.POINTER(LossCfg), C.POINTER(StepOut), _FP]),
    'dnnca_dev_alloc': (C.c_int, [C.POINTER(_VP), C.c_size_t]),
    'dnnca_dev_free': (C.c_int, [_VP]),
    'dnnca_memcpy_h2d': (C.c_int, [_VP, _VP, C.c_size_t]),
    'dnnca_warp_f32': (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 _VP, _VP]),
    'dnnca_warp_groups_f32': (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int,
                                        C.POINTER(C.c_double), C.POINTER(C.c_double), _VP, _VP]),
    'dnnca_affine_f32': (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), _VP, _VP]),
    'dnnca_intensity_f32': (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), _VP]),
    'dnnca_augment_u8': (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.POINTER(AugParam), C.c_int, C.c_int,
                                   _VP, _VP]),
    'dnnca_memcpy_d2h': (C.c_int, [_VP, _VP, C.c_size_t]),
    'dnnca_train_step_dev': (C.c_int, [_VP, _VP, _VP, C.c_int, C.c_float, C.POINTER(LossCfg), C.POINTER(StepOut)]),
    'dnnca_forward_dev': (C.c_int, [_VP, _VP, C.c_int, C.c_int]),
    'dnnca_last_step_out': (C.c_int, [_VP, C.POINTER(StepOut)]),
    'dnnca_sync': (C.c_int, [_VP]),
    'dnnca_crc32c': (C.c_int, [_VP, C.c_size_t, C.POINTER(C.c_uint32)]),
    'dnnca_stage_init': (C.c_int, [_VP, C.c_int, C.c_size_t]),
    'dnnca_stage_upload': (C.c_int, [_VP, C.c_int, _VP, C.c_size_t, _VP, C.c_size_t, C.POINTER(_VP), C.POINTER(_VP)]),
    'dnnca_stage_uploaded': (C.c_int, [_VP, C.c_int]),
    'dnnca_stage_wait': (C.c_int, [_VP, C.c_int]),
    'dnnca_train_step_staged': (C.c_int, [_VP, C.c_int, _VP, _VP, C.c_int, C.c_float, C.POINTER(LossCfg)]),
    'dnnca_staged_out': (C.c_int, [_VP, C.c_int, C.POINTER(StepOut)]),
    'dnnca_eval_begin': (C.c_int, [_VP, _VP, C.c_int]),
    'dnnca_eval_step_staged': (C.c_int, [_VP, C.c_int, _VP, _VP, C.c_int, C.POINTER(LossCfg)]),
    'dnnca_eval_end': (C.c_int, [_VP, C.POINTER(Confusion)]),
    'dnnca_train_metrics': (C.c_int, [_VP, _FP, C.c_int]),
    'dnnca_last_step_confusion': (C.c_int, [_VP, C.POINTER(Confusion)]),
    'dnnca_staged_confusion': (C.c_int, [_VP, C.c_int, C.POINTER(Confusion)]),
    'dnnca_get_prob': (C.c_int, [_VP, _FP, C.c_int64]),
    'dnnca_model_set_region_loss': (C.c_int, [_VP, C.POINTER(RegionLoss)]),
    'dnnca_region_loss_sums': (C.c_int, [_VP, C.c_int, C.POINTER(C.c_double)]),
    'dnnca_model_set_boundary_loss': (C.c_int, [_VP, C.c_float]),
    'dnnca_boundary_loss_sums': (C.c_int, [_VP, C.c_int, C.POINTER(C.c_double)]),
    'dnnca_boundary_distance': (C.c_int, [_VP, C.c_int, _FP]),
    'dnnca_signed_distance_of': (C.c_int, [_VP, _FP, C.c_int, C.c_int, C.c_int, _FP, C.POINTER(C.c_int32)]),
    'dnnca_model_set_topk_loss': (C.c_int, [_VP, C.c_double]),
    'dnnca_topk_loss_state': (C.c_int, [_VP, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _FP, C.POINTER(C.c_double)]),
    'dnnca_topk_pixel_loss': (C.c_int, [_VP, C.c_int, _FP]),
    'dnnca_topk_select_of': (C.c_int, [_VP, _FP, C.c_int, C.c_int, C.c_int, _FP, C.POINTER(C.c_int32)]),
    'dnnca_pixel_confusion': (C.c_int, [_VP, _FP, C.c_int, _FP, C.c_int, C.POINTER(Confusion)]),
    'dnnca_pixel_confusion_of': (C.c_int, [_VP, _FP, _FP, C.c_int64, _FP, C.c_int, C.POINTER(Confusion)]),
    'dnnca_region_confusion_of': (C.c_int, [_VP, _FP, _FP, C.c_int, C.c_int, C.c_int, C.POINTER(RegionSpec), C.POINTER(RegionCounts)]),
    'dnnca_region_confusion': (C.c_int, [_VP, _FP, C.c_int, C.POINTER(RegionSpec), C.POINTER(RegionCounts)]),
    'dnnca_eval_region_begin': (C.c_int, [_VP, C.POINTER(RegionSpec), C.c_int]),
    'dnnca_eval_region_end': (C.c_int, [_VP, C.POINTER(RegionCounts)]),
    'dnnca_region_confusion_slices': (C.c_int, [_VP, _FP, _FP, C.c_int, C.POINTER(RegionSpec), C.c_int, C.POINTER(RegionCounts)]),
    'dnnca_render_composite': (C.c_int, [_VP, _FP, C.c_int, C.c_float, C.c_int, _VP, C.c_int64, C.POINTER(C.c_int32)]),
    'dnnca_lesion_table': (C.c_int, [_VP, _FP, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(LesionRow), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _VP, C.c_int64,
                                     C.POINTER(C.c_int32)]),
    'dnnca_model_set_lesion_refine': (C.c_int, [_VP, C.POINTER(LesionRefine)]),
    'dnnca_model_get_lesion_refine': (C.c_int, [_VP, C.POINTER(LesionRefine)]),
    'dnnca_lesion_table_spread': (C.c_int, [_VP, _FP, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(LesionRow), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _VP, C.c_int64,
                                            C.POINTER(C.c_int32), _FP, C.POINTER(LesionSpread), C.POINTER(SliceSpread)]),
    'dnnca_lesion_table_features': (C.c_int, [_VP, _FP, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                              C.POINTER(LesionRow), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _VP,
                                              C.c_int64, C.POINTER(C.c_int32), _FP, C.c_int, C.c_int, C.c_int, C.POINTER(LesionShape),
                                              C.POINTER(LesionIntensity), C.POINTER(LesionIntensity), C.POINTER(C.c_uint32)]),
    'dnnca_spread_by_outcome': (C.c_int, [_VP, _FP, _FP, _FP, C.c_int, C.c_int, C.c_int, _FP, C.c_int, C.POINTER(SpreadOutcome)]),
    'dnnca_calibration': (C.c_int, [_VP, _FP, _FP, C.c_int, C.c_int, C.c_int, C.c_int, _FP, C.c_int, C.POINTER(CalibBin),
                                    C.POINTER(CalibTotal), C.POINTER(C.c_double)]),
    'dnnca_prob_temperature': (C.c_int, [_VP, _FP, C.c_int, C.c_int, C.c_int, C.c_float, _FP]),
    'dnnca_detection_map': (C.c_int, [_VP, _FP, C.c_int, C.c_int, C.c_int, C.POINTER(DetectionCfg), _FP, C.POINTER(DetectionRow),
                                      C.POINTER(C.c_int64), C.POINTER(DetectionSlice)]),
    'dnnca_bootstrap_sums': (C.c_int, [_VP, C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int,
                                       C.c_int, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_uint16)]),
    'dnnca_bootstrap_detection': (C.c_int, [_VP, C.POINTER(BootstrapExam), C.c_int, C.POINTER(BootstrapCandidate), C.c_int,
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_uint64,
                                            C.POINTER(BootstrapDetectionRow), C.POINTER(C.c_uint16)]),
    'dnnca_lesion_table_linked': (C.c_int, [_VP, _FP, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                            C.POINTER(LesionRow), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _VP, C.c_int64,
                                            C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(LesionLink), C.c_int64,
                                            C.POINTER(C.c_int64)]),
    'dnnca_lesion_table_matched': (C.c_int, [_VP, _FP, _FP, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                             C.POINTER(C.c_uint8), C.POINTER(LesionPlaneOut), _VP, C.c_int64, C.POINTER(LesionPlaneOut),
                                             C.POINTER(LesionPairsOut), C.POINTER(C.c_int32)]),
    'dnnca_surface_distances': (C.c_int, [_VP, _FP, _FP, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(C.c_int32), C.POINTER(SurfaceSample), C.c_int64, C.POINTER(C.c_int64), _VP, C.c_int64,
                                          C.POINTER(C.c_int32)]),
    'dnnca_input_sensitivity': (C.c_int, [_VP, _FP, C.c_int, C.POINTER(C.c_double)]),
    'dnnca_integrated_gradients': (C.c_int, [_VP, _FP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                             C.POINTER(C.c_double), _FP]),
    'dnnca_comm_unique_id': (C.c_int, [_VP]),
    'dnnca_comm_init': (C.c_int, [_VP, C.c_int, C.c_int, _VP, C.c_size_t]),
    'dnnca_comm_world': (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'dnnca_comm_collectives': (C.c_int, [_VP, C.POINTER(C.c_int)]),
    'dnnca_comm_collective_floats': (C.c_int, [_VP, C.POINTER(C.c_int64)]),
    'dnnca_comm_broadcast_weights': (C.c_int, [_VP, C.c_int]),
    'dnnca_comm_average_state': (C.c_int, [_VP]),
    'dnnca_comm_allreduce_host': (C.c_int, [_VP, C.POINTER(C.c_double), C.c_int64, C.c_int]),
    'dnnca_timer_start': (C.c_int, [_VP]),
    'dnnca_timer_stop': (C.c_int, [_VP, C.POINTER(C.c_float)]),
    'dnnca_profile_enable': (C.c_int, [_VP, C.c_int]),
    'dnnca_profile_focus': (C.c_int, [_VP, C.c_char_p]),
    'dnnca_profile_sample': (C.c_int, [_VP, C.c_int]),
    'dnnca_profile_reset': (C.c_int, [_VP]),
    'dnnca_profile_count': (C.c_int, [_VP, C.POINTER(C.c_int)]),
    'dnnca_profile_get': (C.c_int, [_VP, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'dnnca_plan_dump': (C.c_int, [_VP, C.c_char_p, C.c_size_t]),
    'dnnca_plan_dump_pass': (C.c_int, [_VP, C.c_int, C.c_int, C.c_char_p, C.c_size_t]),
    'dnnca_store_image_fits': (C.c_int, [C.c_longlong, C.c_longlong, C.c_longlong]),
}

_lib = None


def _hip_runtime_mapped():
    """Is a HIP runtime already mapped into this process (somebody else may have initialised it)?"""
    try:
        with open('/proc/self/maps') as f:
            return any('libamdhip64' in line for line in f)
    except OSError:
        return False


def load():
    """dlopen libdnnca.so and declare every prototype.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError('%s is missing: run `python -m dnncancerannotator_amd.build` (hipcc, gfx950). '
                          'There is no CPU fallback.' % LIB_PATH)
    # Multi-process GPU work on this platform needs dmabuf IPC: with the legacy mode RCCL's communicator set-up fails with
    # `hipIpcGetMemHandle: invalid argument` (the host driver only supports dmabuf).  The ROCm runtime reads the variable when it
    # initialises, i.e. at the first HIP call behind this dlopen -- so this is the ONE place every process of the package passes
    # through in time: workers of `python -m dnncancerannotator_amd.launch`, ranks started by torch.distributed.run (bench.py),
    # single-GPU runs.  A value the caller exported wins.
    if 'HSA_ENABLE_IPC_MODE_LEGACY' not in os.environ:
        os.environ['HSA_ENABLE_IPC_MODE_LEGACY'] = '0'
        if _hip_runtime_mapped():
            import warnings
            warnings.warn('libamdhip64 was already loaded when dnncancerannotator_amd set HSA_ENABLE_IPC_MODE_LEGACY=0: if the ROCm '
                          'runtime has initialised, the setting is ignored and multi-process RCCL set-up may fail '
                          '(hipIpcGetMemHandle: invalid argument).  Export it before starting the process.', RuntimeWarning)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code):
    if code != OK:
        raise DnncaError(code, load().dnnca_last_error().decode(errors='replace'))


def fptr(a):
    return a.ctypes.data_as(_FP)


def as_f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)
