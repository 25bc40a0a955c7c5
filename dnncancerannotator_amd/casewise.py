"""Host side of the Visualizer of `annotator evaluate` (annotator/utils/callbacks.py:55-446, wired at engine.py:165-208): the
casewise region counts and composite images come from the device (DeviceModel.region_confusion_slices / render_composite); this
module names, places and writes them, with the standard library only.

Settings engine.eval gives the reference's Visualizer: ratio 0.5, no prediction threshold, 100 region thresholds i / 99, IoU 0.30,
export_path_depth 3 and export_casewise_metrics True (hard-coded there, so --export_casewise_metrics changes nothing).

Files under <export_path>/<tag>/ (callbacks.py _emit):
    images/<last 3 components of the exam path>/<sliceID %02d>/step_<step %08d>.png           (--export_images)
    csv/<last 3 components of the exam path>/<sliceID %02d>/step_<step %08d>_metrics.csv      (--export_csv)
    casewise_results.csv: every slice of every evaluated checkpoint, in dataset order          (--export_csv)
    images/.../step_<step %08d>_sensitivity.png and csv/.../step_<step %08d>_sensitivity.csv  (--visualize_sensitivity, per slice)
    images/.../step_<step %08d>_attribution.png and csv/.../step_<step %08d>_attribution.csv  (--visualize_attribution, per slice)
    attribution_results.csv: one line per evaluated checkpoint                                (--visualize_attribution)
The CSV bytes are those of pandas' to_csv (`pd.DataFrame(series).T.to_csv()`, `pd.DataFrame(rows).to_csv()`): csv-module
quoting, '\\n' line ends, an empty header cell for the index."""

import csv
import io
import math
import os
import re
import struct
import zlib
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

RATIO = 0.5                      # Visualizer(ratio=0.5)
N_THRESHOLDS = 100               # pr_region_nthreshold
IOU_THRESHOLD = 0.30             # pr_IoU_threshold
MORPH_FILTER_SIZE = 5            # RegionBasedConfusionMatrix's default
EXPORT_PATH_DEPTH = 3
THRESHOLDS = [i / float(N_THRESHOLDS - 1) for i in range(N_THRESHOLDS)]      # prepare_internal_metrics
MAX_WORKERS = 16                 # PNG encoding and file writes: zlib releases the GIL
PNG_LEVEL = 6                    # zlib's default level

_TAG = re.compile(r'^path:(.*),sliceID:(.*)$')


def device_spec():
    """the region spec of the casewise counts: RegionBasedConfusionMatrix(THRESHOLDS, 0.30, resize_factor=RATIO), k = 5"""
    return (np.asarray(THRESHOLDS, np.float32), IOU_THRESHOLD, RATIO, MORPH_FILTER_SIZE)


def column_names(thresholds=THRESHOLDS):
    """region_tp@PixelThreshold{t:.2} for every threshold, then region_fn@..., region_fp@..., then `tag`"""
    return ['region_%s@PixelThreshold%s' % (kind, format(t, '.2')) for kind in ('tp', 'fn', 'fp') for t in thresholds] + ['tag']


def tag_of(path, slice_id):
    """make_summary_constructor: 'path:<exam path>,sliceID:<n>'"""
    return 'path:%s,sliceID:%d' % (path, int(slice_id))


def row_values(counts, tag):
    """device counts [T, 4] (tp_label, fn, tp_pred, fp) of one slice -> the values of its row: tp..., fn..., fp..., tag
    (get_tp_fn_fp(return_raw=True) counts detected lesions as tp)"""
    c = np.asarray(counts, np.int64)
    return [int(v) for v in c[:, 0]] + [int(v) for v in c[:, 1]] + [int(v) for v in c[:, 3]] + [tag]


def export_dir(root, kind, tag, depth=EXPORT_PATH_DEPTH):
    """<root>/<kind>/<last `depth` components of the exam path>/<sliceID %02d> for a tag (callbacks.py _emit)"""
    m = _TAG.match(tag)
    if m is None:
        raise ValueError('not a Visualizer tag: %r' % (tag,))
    parts = m.group(1).split('/')[-depth:]
    return os.path.join(root, kind, *parts, '%02d' % int(m.group(2)))


def image_path(root, tag, step):
    return os.path.join(export_dir(root, 'images', tag), 'step_%08d.png' % int(step))


def csv_path(root, tag, step):
    return os.path.join(export_dir(root, 'csv', tag), 'step_%08d_metrics.csv' % int(step))


def _csv(rows):
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator='\n')
    for r in rows:
        w.writerow(r)
    return buf.getvalue()


def series_csv(names, values):
    """pd.DataFrame(pd.Series(dict(zip(names, values)))).T.to_csv(): a header ',name1,...' and the row '0,v1,...'"""
    return _csv([[''] + list(names), [0] + list(values)])


def table_csv(names, rows):
    """pd.DataFrame([series, ...]).to_csv(): rows numbered from 0; no rows -> '""\\n' (an empty frame)"""
    if not rows:
        return _csv([['']])
    return _csv([[''] + list(names)] + [[i] + list(r) for i, r in enumerate(rows)])


# ---- channel sensitivity (callbacks.py:290-313, 352-398): DeviceModel.input_sensitivity gives the raw sums -----------------------
def sensitivity_path(root, tag, step, kind):
    """kind 'csv' -> csv/<exam>/<slice>/step_<step>_sensitivity.csv, 'images' -> images/<exam>/<slice>/step_<step>_sensitivity.png"""
    ext = {'csv': 'csv', 'images': 'png'}[kind]
    return os.path.join(export_dir(root, kind, tag), 'step_%08d_sensitivity.%s' % (int(step), ext))


def modality_names(slice_types, n_channels):
    """the dataset's slice_types without the label, in their order; a dataset without them (synthetic, .npz): ch0, ch1, ..."""
    if slice_types:
        names = [str(t) for t in slice_types if t != 'label']
        if len(names) == int(n_channels):
            return names
    return ['ch%d' % i for i in range(int(n_channels))]


def normalise_sensitivity(sums):
    """raw sums [B, C] -> rows divided by their sum; an all-zero row is 0 / 0 = NaN, as in the reference"""
    s = np.asarray(sums, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return s / s.sum(axis=-1, keepdims=True)


def sensitivity_csv(names, values):
    """pd.Series(values, index=names).to_csv(): the header ',0', then 'name,value' per modality (repr of the float64; NaN: empty)"""
    rows = [['', 0]]
    for n, v in zip(names, values):
        v = float(v)
        rows.append([n, '' if v != v else repr(v)])
    return _csv(rows)


# the bar chart: a white canvas, a black frame around the plot area (y from 0 at its bottom to 1 at its top), one bar per modality
CHART_PLOT_H = 200               # pixels of y = 0 .. 1
CHART_MARGIN = 20
CHART_SLOT = 48                  # horizontal room of one modality; its bar is the middle CHART_BAR pixels
CHART_BAR = 32
CHART_BAR_RGB = (31, 119, 180)


def chart_bar_columns(n):
    """[(x0, x1)] pixel columns [x0, x1) of each of the n bars"""
    off = CHART_MARGIN + 1 + (CHART_SLOT - CHART_BAR) // 2
    return [(off + i * CHART_SLOT, off + i * CHART_SLOT + CHART_BAR) for i in range(int(n))]


def chart_bar_height(v):
    """pixels of a bar of value v: round(v * CHART_PLOT_H), v clipped to [0, 1]; NaN: no bar"""
    v = float(v)
    if v != v:
        return 0
    return int(round(min(max(v, 0.0), 1.0) * CHART_PLOT_H))


def sensitivity_chart(values):
    """normalised sensitivities of one slice -> uint8 RGB [h, w, 3] bar chart (modality order = value order, y range 0 .. 1).
    Plain numpy: not the pixels of the reference's matplotlib figure."""
    n = len(values)
    h, w = CHART_PLOT_H + 2 * CHART_MARGIN + 2, n * CHART_SLOT + 2 * CHART_MARGIN + 2
    img = np.full((h, w, 3), 255, np.uint8)
    top, bottom, left, right = CHART_MARGIN, CHART_MARGIN + CHART_PLOT_H + 1, CHART_MARGIN, w - CHART_MARGIN - 1
    img[top, left:right + 1] = 0
    img[bottom, left:right + 1] = 0
    img[top:bottom + 1, left] = 0
    img[top:bottom + 1, right] = 0
    for (x0, x1), v in zip(chart_bar_columns(n), values):
        bh = chart_bar_height(v)
        if bh:
            img[bottom - bh:bottom, x0:x1] = CHART_BAR_RGB
    return img


# ---- integrated-gradients attribution (--visualize_attribution): DeviceModel.integrated_gradients gives sums, endpoints and map --
ATTRIBUTION_STEPS = 32                   # --attribution_steps
ATTRIBUTION_STEP_RANGE = (1, 256)        # what the library accepts
ATTRIBUTION_BASELINES = ('black', 'mean')
ATTRIBUTION_RESULT_COLUMNS = ['steps', 'baseline', 'slices']     # then share_<modality>..., mean_relative_gap, max_relative_gap
ATTRIBUTION_GAP = 2                      # white pixels between two panels of attribution_image
ATTRIBUTION_FOR_RGB = (255, 0, 0)        # the colour of +scale (evidence for a lesion); 0 is white
ATTRIBUTION_AGAINST_RGB = (0, 0, 255)    # the colour of -scale (evidence against)


def attribution_path(root, tag, step, kind):
    """kind 'csv' -> csv/<exam>/<slice>/step_<step>_attribution.csv, 'images' -> images/<exam>/<slice>/step_<step>_attribution.png"""
    ext = {'csv': 'csv', 'images': 'png'}[kind]
    return os.path.join(export_dir(root, kind, tag), 'step_%08d_attribution.%s' % (int(step), ext))


def attribution_shares(absolute):
    """sums of |attr| [B, C] -> rows divided by their sum: the share of each modality; an all-zero row is NaN, as in
    normalise_sensitivity"""
    return normalise_sensitivity(absolute)


def attribution_gap(signed, endpoints):
    """(gap, relative gap) per slice, float64 [B] each: gap = sum over the modalities of signed[b] - (F(x) - F(baseline)), the
    completeness error of the quadrature; relative to |F(x) - F(baseline)| (NaN where that is 0)"""
    s, e = np.asarray(signed, np.float64), np.asarray(endpoints, np.float64)
    delta = e[..., 0] - e[..., 1]
    gap = s.sum(axis=-1) - delta
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.where(delta != 0, gap / np.abs(delta), np.nan)
    return gap, rel


def _float_cell(v):
    v = float(v)
    return '' if v != v else repr(v)


def attribution_csv(names, shares, signed, absolute, endpoints):
    """the per-slice file: 'modality,share,signed,absolute' and one line per modality, then the lines f_x, f_baseline, gap and
    relative_gap with their value in the second cell (repr of the float64; NaN: empty)"""
    gap, rel = attribution_gap(signed, endpoints)
    rows = [['modality', 'share', 'signed', 'absolute']]
    for n, sh, s, a in zip(names, shares, signed, absolute):
        rows.append([n, _float_cell(sh), _float_cell(s), _float_cell(a)])
    rows += [['f_x', _float_cell(endpoints[0])], ['f_baseline', _float_cell(endpoints[1])], ['gap', _float_cell(gap)],
             ['relative_gap', _float_cell(rel)]]
    return _csv(rows)


def attribution_image(amap, names=None):
    """attr of one slice [H, W, C] -> uint8 RGB [H, C * W + (C - 1) * ATTRIBUTION_GAP, 3]: one panel per modality (the order of
    `names`; they only fix the number of panels), side by side, white columns between them.  Diverging colours on one common scale
    s = the slice's largest |attr|: 0 is white, +s ATTRIBUTION_FOR_RGB (red: evidence for), -s ATTRIBUTION_AGAINST_RGB (blue: evidence
    against), linear in between, rounded to nearest.  An all-zero or non-finite map is all white.  Plain numpy."""
    a = np.asarray(amap, np.float64)
    if a.ndim != 3 or (names is not None and len(names) != a.shape[2]):
        raise ValueError('attribution_image: a map [H, W, C] and C names, got %s and %r' % (a.shape, names))
    h, w, c = a.shape
    img = np.full((h, c * w + (c - 1) * ATTRIBUTION_GAP, 3), 255, np.uint8)
    scale = float(np.abs(a).max()) if a.size else 0.0
    if not (scale > 0 and math.isfinite(scale)):
        return img
    t = a / scale                                                        # in [-1, 1]
    white = np.array([255.0, 255.0, 255.0])
    for j in range(c):
        u = t[:, :, j, None]
        tip = np.where(u >= 0, np.array(ATTRIBUTION_FOR_RGB, np.float64), np.array(ATTRIBUTION_AGAINST_RGB, np.float64))
        panel = white + np.abs(u) * (tip - white)
        img[:, j * (w + ATTRIBUTION_GAP):j * (w + ATTRIBUTION_GAP) + w] = np.rint(panel).astype(np.uint8)
    return img


def attribution_summary(steps, baseline, shares, relative_gaps):
    """the attribution_results.csv values of one checkpoint: steps, baseline, slices, the mean share per modality over the slices
    whose shares are numbers, the mean and the largest |relative gap| over the slices where it is a number ('' where none is)"""
    sh, rel = np.asarray(shares, np.float64), np.abs(np.asarray(relative_gaps, np.float64)).ravel()
    sh = sh.reshape(len(sh), -1) if len(sh) else np.zeros((0, sh.shape[1] if sh.ndim == 2 else 0))
    ok = ~np.isnan(sh).any(axis=1)
    mean_share = sh[ok].mean(axis=0) if ok.any() else np.full(sh.shape[1], np.nan)
    rel = rel[~np.isnan(rel)]
    return [int(steps), str(baseline), len(sh)] + [_float_cell(v) for v in mean_share] + \
        [_float_cell(rel.mean() if len(rel) else np.nan), _float_cell(rel.max() if len(rel) else np.nan)]


# ---- `annotator predict`: the lesion table of slices without a label (DeviceModel.lesion_table gives the integer sums) ----------
LESION_COLUMNS = ['exam', 'slice', 'lesion', 'area_px', 'x0', 'y0', 'x1', 'y1', 'centroid_x', 'centroid_y', 'mean_prob', 'max_prob']
SLICE_COLUMNS = ['exam', 'slice', 'n_lesions', 'lesion_area_px', 'max_prob', 'truncated']
Q24 = float(1 << 24)             # sum_prob_q24 is the sum of rint(p * 2^24)


def lesion_values(exam, slice_id, row):
    """one record of lesion_table's rows -> the values of its lesions.csv line.  centroid = sum / area and mean = sum_q24 / area /
    2^24 in float64 (repr, so they read back exactly); max_prob with the 9 digits that give the float32 back"""
    area = int(row['area'])
    return [exam, int(slice_id), int(row['row']), area, int(row['x0']), int(row['y0']), int(row['x1']), int(row['y1']),
            repr(int(row['sum_x']) / area), repr(int(row['sum_y']) / area), repr(int(row['sum_prob_q24']) / area / Q24),
            '%.9g' % float(row['max_prob'])]


def slice_values(exam, slice_id, rows, total):
    """the slices.csv line of one slice: `rows` are the slice's records (at most max_lesions), `total` its kept components.
    n_lesions = total; lesion_area_px and max_prob cover the rows that came back; truncated = 1 when total exceeds them"""
    return [exam, int(slice_id), int(total), int(sum(int(r['area']) for r in rows)),
            '%.9g' % max([float(r['max_prob']) for r in rows], default=0.0), int(int(total) > len(rows))]


# ---- `annotator predict --link_slices`: the 2-D lesions of an exam joined through its slices -----------------------------------
EXAM_LESION_COLUMNS = ['exam', 'exam_lesion', 'first_slice', 'last_slice', 'n_slices', 'n_parts', 'volume_px', 'x0', 'y0', 'x1', 'y1',
                       'centroid_x', 'centroid_y', 'centroid_slice', 'mean_prob', 'max_prob', 'truncated']
EXAM_PART_COLUMNS = ['exam', 'slice', 'lesion', 'exam_lesion']


def link_lesions(exam, slices, links, min_overlap=1):
    """The lesions of one exam joined across its slices: (exam_lesions.csv values, exam_lesion_parts.csv values).

    slices: [(slice_id, rows, total)] in the order the exam's slices were analysed -- `rows` the slice's records of lesion_table (at
    most max_lesions), `total` its kept components.  links: one sequence per entry of `slices`: the (row_prev, row, overlap) of
    lesion_table_linked between the entry before (row_prev) and this one (row); empty where the slice does not continue the one
    before (the first slice, a gap in the slice numbers).  Two lesions belong together when a link of at least min_overlap pixels
    joins them, directly or through others (union-find).  Exam lesions are numbered by their first member in (slice order, lesion
    number) order.  Volume, bounding box, sums and the maximum are integer sums / extrema over the members; the centroids (the
    slice's is the area-weighted mean slice_id) and mean_prob are float64 quotients written with repr; truncated = 1 when a
    slice the lesion touches had more components than rows (those beyond max_lesions are in no table and link to nothing).
    The parts come one per row, slice after slice: the order of the exam's lines in lesions.csv."""
    if len(links) != len(slices):
        raise ValueError('link_lesions: %d slices but %d link lists' % (len(slices), len(links)))
    first, nodes = [], []                                           # first[i]: the node of row 0 of slices[i]; nodes: (i, row record)
    for i, (_, rows, _) in enumerate(slices):
        first.append(len(nodes))
        nodes += [(i, r) for r in rows]
    parent = list(range(len(nodes)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i, mine in enumerate(links):
        for row_prev, row, overlap in mine:
            if i == 0 or not (0 <= int(row_prev) < len(slices[i - 1][1]) and 0 <= int(row) < len(slices[i][1])):
                raise ValueError('link_lesions: link (%d, %d) into slice %d of the exam joins no rows' % (row_prev, row, i))
            if int(overlap) >= min_overlap:
                a, b = find(first[i - 1] + int(row_prev)), find(first[i] + int(row))
                parent[max(a, b)] = min(a, b)                       # the root is the first member
    number, members = {}, []
    for n in range(len(nodes)):
        root = find(n)
        if root not in number:
            number[root] = len(members)
            members.append([])
        members[number[root]].append(n)
    table = []
    for e, ms in enumerate(members):
        rows = [nodes[n][1] for n in ms]
        ids = [int(slices[nodes[n][0]][0]) for n in ms]
        area = [int(r['area']) for r in rows]
        volume = sum(area)
        touched = sorted(set(nodes[n][0] for n in ms))
        table.append([exam, e, min(ids), max(ids), len(touched), len(ms), volume,
                      min(int(r['x0']) for r in rows), min(int(r['y0']) for r in rows), max(int(r['x1']) for r in rows),
                      max(int(r['y1']) for r in rows), repr(sum(int(r['sum_x']) for r in rows) / volume),
                      repr(sum(int(r['sum_y']) for r in rows) / volume), repr(sum(k * a for k, a in zip(ids, area)) / volume),
                      repr(sum(int(r['sum_prob_q24']) for r in rows) / volume / Q24), '%.9g' % max(float(r['max_prob']) for r in rows),
                      int(any(int(slices[i][2]) > len(slices[i][1]) for i in touched))])
    parts = [[exam, int(slices[i][0]), int(r['row']), number[find(n)]] for n, (i, r) in enumerate(nodes)]
    return table, parts


# one slice of a DeviceModel.lesion_table_matched call: rows / total / links of the predicted plane, the same of the labelled one and
# the pairs between them.  A lesion_table_linked call has one plane: its records leave the last four fields None
SliceRecord = namedtuple('SliceRecord', 'exam slice rows total links true_rows true_total true_links pairs', defaults=(None,) * 4)


def triples(records, first='row_prev'):
    """link records -> [(row_prev, row, overlap)] as link_lesions takes them; pair records with first='row_true'"""
    return [(int(r[first]), int(r['row']), int(r['overlap'])) for r in records]


def slice_records(out, pk):
    """what lesion_table_matched returned (rows, totals, masks, links, true_rows, true_totals, true_links, pairs) -- or the four values
    of lesion_table_linked -- for the slices pk = [(path, sliceID)] of one call -> one SliceRecord per slice, in their order"""
    rows, totals, _, links, *labelled = out
    of = lambda records, b: records[records['slice'] == b]          # noqa: E731
    found = []
    for b, (p, k) in enumerate(pk):
        rec = SliceRecord(p, int(k), of(rows, b), totals[b], triples(of(links, b)))
        if labelled:
            true_rows, true_totals, true_links, pairs = labelled
            rec = rec._replace(true_rows=of(true_rows, b), true_total=true_totals[b], true_links=triples(of(true_links, b)),
                               pairs=triples(of(pairs, b), 'row_true'))
        found.append(rec)
    return found


def by_exam(records):
    """records whose first field is the exam path -> {exam: its records}, exams and records in the order of the data set (the slices
    of two exams may come interleaved)"""
    exams = {}
    for rec in records:
        exams.setdefault(rec[0], []).append(rec)
    return exams


def link_records(exam, records, min_overlap=1):
    """link_lesions on the predicted plane of an exam's SliceRecords"""
    return link_lesions(exam, [(r.slice, r.rows, r.total) for r in records], [r.links for r in records], min_overlap=min_overlap)


def match_records(matcher, exam, records, min_overlap=1, **kw):
    """an exam's SliceRecords: either plane linked through the slices (link_lesions), then both handed to `matcher`
    (match_exam_lesions or detection_match, which get **kw) -> what it returns"""
    pred_slices, true_slices = [(r.slice, r.rows, r.total) for r in records], [(r.slice, r.true_rows, r.true_total) for r in records]
    pred_linked = link_records(exam, records, min_overlap)
    true_linked = link_lesions(exam, true_slices, [r.true_links for r in records], min_overlap=min_overlap)
    return matcher(exam, true_slices, pred_slices, true_linked, pred_linked, [r.pairs for r in records], **kw)


# ---- `annotator evaluate --exam_lesions`: the predicted exam lesions of link_lesions scored against the labelled ones --------------
EXAM_MATCH_COLUMNS = ['kind', 'exam', 'exam_lesion', 'first_slice', 'last_slice', 'n_slices', 'volume_px', 'partner', 'overlap_px', 'iou',
                      'dice', 'hit']
EXAM_CASE_COLUMNS = ['exam', 'true', 'predicted', 'detected', 'missed', 'matched', 'false', 'truncated']
EXAM_RESULT_COLUMNS = ['exams', 'true', 'predicted', 'detected', 'missed', 'matched', 'false', 'recall', 'precision', 'f1',
                       'false_per_exam']
EXAM_IOU = 0.30                  # IoU_threshold / pr_IoU_threshold of the reference
EXAM_EPSILON = 1e-07             # region_metrics._RegionBasedMetric's epsilon


def exam_overlaps(true_slices, pred_slices, true_linked, pred_linked, pairs, who='match_exam_lesions'):
    """the common voxels of the labelled and the predicted exam lesions of one exam: ({(T, P): overlap}, volumes of the labelled,
    volumes of the predicted ones), from the arguments of match_exam_lesions (shared with detection_match)"""
    if not len(true_slices) == len(pred_slices) == len(pairs):
        raise ValueError('%s: %d / %d slices and %d pair lists' % (who, len(true_slices), len(pred_slices), len(pairs)))

    def part_numbers(slices, parts):
        """[slice][row] -> the exam lesion; the parts come one per row, slice after slice"""
        out, at = [], 0
        for _, rows, _ in slices:
            out.append([int(p[3]) for p in parts[at:at + len(rows)]])
            at += len(rows)
        if at != len(parts):
            raise ValueError('%s: %d parts for %d rows' % (who, len(parts), at))
        return out
    of_true, of_pred = part_numbers(true_slices, true_linked[1]), part_numbers(pred_slices, pred_linked[1])
    overlap = {}                                                    # (T, P) -> common voxels
    for i, mine in enumerate(pairs):
        for row_true, row, n in mine:
            if not (0 <= int(row_true) < len(of_true[i]) and 0 <= int(row) < len(of_pred[i])):
                raise ValueError('%s: pair (%d, %d) of slice %d of the exam joins no rows' % (who, row_true, row, i))
            key = of_true[i][int(row_true)], of_pred[i][int(row)]
            overlap[key] = overlap.get(key, 0) + int(n)
    return overlap, [int(r[6]) for r in true_linked[0]], [int(r[6]) for r in pred_linked[0]]


def match_exam_lesions(exam, true_slices, pred_slices, true_linked, pred_linked, pairs, iou=EXAM_IOU):
    """The labelled and the predicted exam lesions of one exam held against each other: (case values, match values).

    true_slices / pred_slices: [(slice_id, rows, total)] of the two planes as link_lesions takes them (the same slices in the same
    order); true_linked / pred_linked: what link_lesions returned for them, (table, parts); pairs: one sequence per slice, the
    (row_true, row, overlap) of lesion_table_matched.  The 3-D overlap of a labelled tumour T and a predicted tumour P is the sum
    of `overlap` over the pairs whose row_true is a part of T and whose row is a part of P; union = volume(T) + volume(P) -
    overlap.  T and P hit when overlap >= 1 and overlap / union >= iou (plain float division).  A labelled tumour is detected when
    some P hits it; a predicted tumour is matched when it hits some T, else false (the two directions of the reference's
    get_tp_fn / get_tp_fp).
    Case values (EXAM_CASE_COLUMNS): the counts of the exam; truncated = 1 when a slice of either plane had more components than
    rows.  Match values (EXAM_MATCH_COLUMNS): one line per tumour, the labelled ones (kind 'true') before the predicted ones, each
    with its best partner on the other side -- the largest IoU, the smaller number on a tie; -1, 0, 0.0, 0.0 without any -- and
    hit = 1 for detected / matched.  iou and dice (2 overlap / (volume(T) + volume(P))) are float64 quotients written with repr."""
    overlap, vol_true, vol_pred = exam_overlaps(true_slices, pred_slices, true_linked, pred_linked, pairs)
    best = {'true': [None] * len(vol_true), 'predicted': [None] * len(vol_pred)}      # (iou, -partner, overlap, dice, hit)
    hit = {'true': [0] * len(vol_true), 'predicted': [0] * len(vol_pred)}
    for (t, q), n in sorted(overlap.items()):
        union = vol_true[t] + vol_pred[q] - n
        score, dice = n / union, 2 * n / (vol_true[t] + vol_pred[q])
        hits = int(n >= 1 and score >= iou)
        for kind, me, other in (('true', t, q), ('predicted', q, t)):
            hit[kind][me] |= hits
            cand = (score, -other, n, dice)
            if n >= 1 and (best[kind][me] is None or cand[:2] > best[kind][me][:2]):
                best[kind][me] = cand
    lines = []
    for kind, table in (('true', true_linked[0]), ('predicted', pred_linked[0])):
        for e, r in enumerate(table):
            b = best[kind][e]
            lines.append([kind, exam, int(r[1]), int(r[2]), int(r[3]), int(r[4]), int(r[6])] +
                         ([-1, 0, repr(0.0), repr(0.0)] if b is None else [-b[1], b[2], repr(b[0]), repr(b[3])]) + [hit[kind][e]])
    detected, matched = sum(hit['true']), sum(hit['predicted'])
    truncated = int(any(int(total) > len(rows) for sl in (true_slices, pred_slices) for _, rows, total in sl))
    case = [exam, len(vol_true), len(vol_pred), detected, len(vol_true) - detected, matched, len(vol_pred) - matched, truncated]
    return case, lines


def exam_match_summary(cases):
    """the EXAM_CASE_COLUMNS values of every exam -> the EXAM_RESULT_COLUMNS values: the summed counts, recall = detected / true and
    precision = matched / predicted as region_metrics writes region/recall and region/precision (float32 count / (float32 sum +
    epsilon)), F1 = 2 P R / (P + R + epsilon) likewise, false_per_exam = false / exams (0.0 without exams)"""
    n = [sum(int(c[i]) for c in cases) for i in range(1, 7)]        # true, predicted, detected, missed, matched, false
    return [len(cases)] + n + [repr(v) for v in _exam_match_ratios(n, len(cases), EXAM_EPSILON)]


def _exam_match_ratios(n, exams, epsilon):
    """the summed counts (true, predicted, detected, missed, matched, false) of `exams` exams -> [recall, precision, f1,
    false_per_exam] as Python floats: the float32 arithmetic of exam_match_summary, shared with exam_match_replicate_values"""
    f32 = np.float32
    recall = f32(n[2]) / (f32(n[2] + n[3]) + f32(epsilon))
    precision = f32(n[4]) / (f32(n[4] + n[5]) + f32(epsilon))
    f1 = f32(2) * precision * recall / (precision + recall + f32(epsilon))
    return [float(recall), float(precision), float(f1), n[5] / exams if exams else 0.0]


# ---- `annotator evaluate --detection`: ranked lesion candidates, AP, FROC and AUROC -----------------------------------------------
# DeviceModel.detection_map gives every candidate one confidence (the peak it grew from); lesion_table_matched on the map gives the
# candidates as rows (max_prob = confidence) and their overlaps with the labelled lesions; link_lesions joins both planes through the
# slices.  Everything here is Python integers and float64; pooled values come from summed counts, never from per-exam ratios.
DETECTION_DEFAULTS = dict(min_confidence=0.1, factor=0.4, max_candidates=5, min_area=10, rounds=16)      # PI-CAI: factor = 1 / 2.5
DETECTION_RANGES = dict(min_confidence=(0.001, 1.0), factor=(0.01, 1.0), max_candidates=(1, 64), min_area=(1, 1 << 30), rounds=(1, 256))
DETECTION_IOU = 0.10             # --detection_iou: PI-CAI's hit criterion
DETECTION_FP_RATES = (0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0)       # false positives per exam at which the sensitivity is read (CPM)
DETECTION_RESULT_COLUMNS = (['exams', 'positive_exams', 'tumours', 'candidates', 'tp', 'fp', 'fn', 'ap', 'auroc', 'score'] +
                            ['sensitivity_at_%g' % x for x in DETECTION_FP_RATES] + ['cpm', 'slices_exhausted'])
DETECTION_FROC_COLUMNS = ['confidence', 'tp', 'fp', 'sensitivity', 'fp_per_exam', 'precision']
DETECTION_CASE_COLUMNS = ['exam', 'positive', 'score', 'candidates', 'tp', 'fp', 'fn']
DETECTION_CANDIDATE_COLUMNS = ['exam', 'candidate', 'first_slice', 'last_slice', 'volume_px', 'confidence', 'tumour', 'iou', 'outcome']
CANDIDATE_COLUMNS = LESION_COLUMNS + ['confidence']               # predict --detection_map: candidates.csv
SLICE_CANDIDATE_COLUMNS = ['exam', 'slice', 'candidates', 'rounds', 'dropped', 'exhausted']
EXAM_CANDIDATE_COLUMNS = EXAM_LESION_COLUMNS + ['confidence']


def detection_table_args(cfg, max_lesions=256):
    """the lesion_table* keywords that read a detection map: every pixel of a candidate is >= min_confidence, nothing is opened,
    resized or filtered, so the rows are the candidates (touching ones joined, max_prob = the larger confidence)"""
    return dict(threshold=float(cfg['min_confidence']), filter_size=1, resize_factor=1.0, min_area=0, max_lesions=int(max_lesions))


def detection_match(exam, true_slices, pred_slices, true_linked, pred_linked, pairs, iou=DETECTION_IOU):
    """The candidates of one exam held against its labelled tumours: (case, candidate lines).  The arguments are those of
    match_exam_lesions, the prediction plane being the detection map.  A candidate's confidence is the largest max_prob of its parts.
    Voxel IoU per candidate / tumour pair = overlap / (volume(T) + volume(P) - overlap).  Candidates in descending confidence (ties:
    the lower number): each takes the not-yet-taken tumour of largest IoU >= iou with overlap >= 1 (ties: the lower number) and is
    a TP; otherwise -- no tumour reached, or only taken ones -- it is an FP.  Tumours never taken are FN.
    case: dict(exam, tumours, confidences [float per candidate, by number], hits [1 TP / 0 FP per candidate]).
    Lines (DETECTION_CANDIDATE_COLUMNS), by candidate number: tumour and iou are the tumour a TP took; for an FP the tumour of largest
    IoU whatever it is (-1 and 0.0 without any overlap)."""
    overlap, vol_true, vol_pred = exam_overlaps(true_slices, pred_slices, true_linked, pred_linked, pairs, who='detection_match')
    conf = [float(np.float32(r[15])) for r in pred_linked[0]]      # the 9 digits of link_lesions give the float32 back
    reach = [[] for _ in vol_pred]                                  # per candidate: (iou, tumour)
    for (t, q), n in sorted(overlap.items()):
        if n >= 1:
            reach[q].append((n / (vol_true[t] + vol_pred[q] - n), t))
    taken, hits, partner = set(), [0] * len(vol_pred), [(-1, 0.0)] * len(vol_pred)
    for q in sorted(range(len(vol_pred)), key=lambda q: (-conf[q], q)):
        free = [(s, -t) for s, t in reach[q] if s >= iou and t not in taken]
        if free:
            s, t = max(free)
            taken.add(-t)
            hits[q], partner[q] = 1, (-t, s)
        elif reach[q]:
            s, t = max((s, -t) for s, t in reach[q])
            partner[q] = (-t, s)
    lines = [[exam, int(r[1]), int(r[2]), int(r[3]), int(r[6]), '%.9g' % conf[q], partner[q][0], repr(float(partner[q][1])),
              'tp' if hits[q] else 'fp'] for q, r in enumerate(pred_linked[0])]
    return dict(exam=exam, tumours=len(vol_true), confidences=conf, hits=hits), lines


def detection_case_values(case):
    """the DETECTION_CASE_COLUMNS values of one detection_match case: the exam's score is its largest confidence, 0 without one"""
    tp = sum(case['hits'])
    return [case['exam'], int(case['tumours'] > 0), '%.9g' % max(case['confidences'], default=0.0), len(case['hits']), tp,
            len(case['hits']) - tp, case['tumours'] - tp]


def detection_curves(cases):
    """The lesion-level ranking statistics of all exams: dict(exams, tumours, candidates, tp, fp, fn, levels, ap, sensitivities, cpm).
    levels: one (confidence, TP, FP, sensitivity, FP per exam, precision) per distinct confidence in descending order -- equal
    confidences enter together -- with cumulative counts; sensitivity = TP / tumours (None without tumours), precision = TP /
    (TP + FP).  ap = sum_k (R_k - R_{k-1}) P_k over the levels, R_0 = 0 (None without tumours; 0.0 without candidates).
    sensitivities: at every one of DETECTION_FP_RATES the largest sensitivity of a level whose FP per exam is <= x (the comparison
    is FP <= x * exams in integers), 0.0 when none (None without tumours); cpm their mean."""
    exams, tumours = len(cases), sum(int(c['tumours']) for c in cases)
    ranked = sorted(((float(s), int(h)) for c in cases for s, h in zip(c['confidences'], c['hits'])), key=lambda v: -v[0])
    levels, tp, fp, i = [], 0, 0, 0
    while i < len(ranked):
        j = i
        while j < len(ranked) and ranked[j][0] == ranked[i][0]:
            tp, fp, j = tp + ranked[j][1], fp + 1 - ranked[j][1], j + 1
        levels.append((ranked[i][0], tp, fp, tp / tumours if tumours else None, fp / exams, tp / (tp + fp)))
        i = j
    ap = sens = cpm = None
    if tumours:
        ap, before = 0.0, 0.0
        for _, _, _, recall, _, precision in levels:
            ap, before = ap + (recall - before) * precision, recall
        sens = [max([l[1] for l in levels if l[2] * 8 <= int(x * 8) * exams], default=0) / tumours for x in DETECTION_FP_RATES]
        cpm = math.fsum(sens) / len(sens)
    return dict(exams=exams, tumours=tumours, candidates=len(ranked), tp=tp, fp=fp, fn=tumours - tp, levels=levels, ap=ap,
                sensitivities=sens, cpm=cpm)


def detection_auroc(cases):
    """exam-level AUROC: an exam's score is its largest candidate confidence (0 without a candidate), it is positive when it has a
    labelled tumour.  (#[s+ > s-] + 1/2 #[s+ = s-]) / (P N), the pairs counted exactly; None when one class is absent"""
    pos = [max(c['confidences'], default=0.0) for c in cases if c['tumours'] > 0]
    neg = [max(c['confidences'], default=0.0) for c in cases if c['tumours'] == 0]
    if not pos or not neg:
        return None
    twice = sum(2 * (p > n) + (p == n) for p in pos for n in neg)
    return twice / (2 * len(pos) * len(neg))


def detection_summary(cases, slices_exhausted=0):
    """all exams' detection_match cases -> (the DETECTION_RESULT_COLUMNS values, the DETECTION_FROC_COLUMNS lines); undefined values
    are blank cells; score = (AP + AUROC) / 2"""
    c, auroc = detection_curves(cases), detection_auroc(cases)
    score = None if c['ap'] is None or auroc is None else (c['ap'] + auroc) / 2
    result = ([c['exams'], sum(1 for k in cases if k['tumours'] > 0), c['tumours'], c['candidates'], c['tp'], c['fp'], c['fn'],
               _blank(c['ap']), _blank(auroc), _blank(score)] +
              [_blank(None if c['sensitivities'] is None else s) for s in (c['sensitivities'] or DETECTION_FP_RATES)] +
              [_blank(c['cpm']), int(slices_exhausted)])
    froc = [['%.9g' % l[0], l[1], l[2], _blank(l[3]), repr(l[4]), repr(l[5])] for l in c['levels']]
    return result, froc


def candidate_values(exam, slice_id, row):
    """the candidates.csv line of one row of the lesion table read from a detection map: the lesions.csv values plus the confidence"""
    return lesion_values(exam, slice_id, row) + ['%.9g' % float(row['max_prob'])]


def detection_image(D):
    """detection.png of one slice: 8-bit grey, rint(D * 255)"""
    return np.rint(np.asarray(D, np.float64) * 255.0).astype(np.uint8)


def detection_path(root, tag):
    """<root>/<last 3 components of the exam path>/<sliceID %02d>/detection.png"""
    return os.path.join(export_dir(root, '', tag), 'detection.png')


# ---- `annotator evaluate --bootstrap`: intervals of the detection and exam-lesion figures from a bootstrap over exams -------------
# DeviceModel.bootstrap_detection / bootstrap_sums resample the exams (include/dnnca.h states the draws) and return, per replicate,
# the integers from which the functions here form the same values as detection_summary / exam_match_summary, by the same arithmetic.
BOOTSTRAP_RANGE = (100, 1 << 20)         # --bootstrap
BOOTSTRAP_LEVEL = 0.95                   # --bootstrap_level, strictly between 0.5 and 1
BOOTSTRAP_COLUMNS = ['metric', 'estimate', 'mean', 'std', 'lo', 'hi', 'level', 'replicates', 'undefined', 'seed', 'stratified']
DETECTION_BOOTSTRAP_METRICS = ['ap', 'auroc', 'score'] + ['sensitivity_at_%g' % x for x in DETECTION_FP_RATES] + ['cpm']
DETECTION_REPLICATE_INTEGERS = (['positive_exams', 'tumours', 'candidates', 'tp', 'fp', 'auroc_pairs', 'auroc_twice'] +
                                ['tp_at_%g' % x for x in DETECTION_FP_RATES])
DETECTION_REPLICATE_COLUMNS = ['replicate'] + DETECTION_REPLICATE_INTEGERS + DETECTION_BOOTSTRAP_METRICS
EXAM_BOOTSTRAP_METRICS = ['recall', 'precision', 'f1', 'false_per_exam']


def bootstrap_pool(positive_flags, stratified):
    """(pool int32 [E], strata int32 [S]) of the exams 0 .. E-1 for DeviceModel.bootstrap_*: plain, the identity and one stratum;
    stratified, the exams whose flag is set first, then the others, each in their order, an empty stratum left out"""
    flags = [bool(f) for f in positive_flags]
    if not stratified:
        return np.arange(len(flags), dtype=np.int32), np.array([len(flags)], np.int32)
    groups = [[e for e, f in enumerate(flags) if f], [e for e, f in enumerate(flags) if not f]]
    return np.array(groups[0] + groups[1], np.int32), np.array([len(g) for g in groups if g], np.int32)


def detection_bootstrap_inputs(cases):
    """all exams' detection_match cases (what detection_summary reads) -> (exams, candidates) for DeviceModel.bootstrap_detection:
    exams [E] (tumours, score_rank: the dense rank of the exam's score -- its largest confidence, 0.0 without a candidate -- among
    all exams, 0 the lowest); candidates [N] (exam, hit, level) sorted by descending confidence, ties by (exam, number), level the
    index of the distinct confidence, 0 the highest"""
    from . import _lib
    scores = [max((float(s) for s in c['confidences']), default=0.0) for c in cases]
    rank = {s: i for i, s in enumerate(sorted(set(scores)))}
    exams = np.zeros(len(cases), _lib.BOOTSTRAP_EXAM_DTYPE)
    exams['tumours'] = [int(c['tumours']) for c in cases]
    exams['score_rank'] = [rank[s] for s in scores]
    ranked = sorted((-float(s), e, k, int(h)) for e, c in enumerate(cases) for k, (s, h) in enumerate(zip(c['confidences'], c['hits'])))
    cands = np.zeros(len(ranked), _lib.BOOTSTRAP_CANDIDATE_DTYPE)
    level = -1
    for i, (s, e, _, h) in enumerate(ranked):
        level += int(i == 0 or s != ranked[i - 1][0])
        cands[i] = (e, h, level)
    return exams, cands


def detection_replicate_values(row, exams):
    """one row of DeviceModel.bootstrap_detection over `exams` exams -> the DETECTION_BOOTSTRAP_METRICS values of the resample: ap,
    auroc, score, the seven sensitivities, cpm; None where detection_curves / detection_auroc give None (no tumour drawn; one class
    of exams not drawn), by their float64 arithmetic on the row's integers"""
    tumours, pairs = int(row['tumours']), int(row['auroc_pairs'])
    ap = float(row['ap']) if tumours else None
    sens = [int(t) / tumours for t in row['tp_at']] if tumours else [None] * len(DETECTION_FP_RATES)
    cpm = math.fsum(sens) / len(sens) if tumours else None
    auroc = int(row['auroc_twice']) / (2 * pairs) if pairs else None
    score = None if ap is None or auroc is None else (ap + auroc) / 2
    return [ap, auroc, score] + sens + [cpm]


def exam_match_replicate_values(sums, exams):
    """one row of DeviceModel.bootstrap_sums over the EXAM_CASE_COLUMNS counts (true, predicted, detected, missed, matched, false)
    of `exams` exams -> the EXAM_BOOTSTRAP_METRICS values of the resample, by exam_match_summary's float32 arithmetic"""
    return _exam_match_ratios([int(v) for v in sums], int(exams), EXAM_EPSILON)


def bootstrap_interval(values, level=BOOTSTRAP_LEVEL):
    """the replicate values of one metric (None: undefined in that replicate) -> dict(mean, std, lo, hi, n, undefined): over the n
    defined values v sorted ascending, lo and hi the quantiles at (1 - level) / 2 and 1 - (1 - level) / 2, a quantile at q being
    v[i] + (h - i) (v[i + 1] - v[i]) with h = q (n - 1) and i = floor(h); mean = fsum / n; std the population standard deviation.
    With n = 0 the four values are None (blank cells)"""
    v = sorted(float(x) for x in values if x is not None)
    n, out = len(v), dict(mean=None, std=None, lo=None, hi=None, n=len(v), undefined=len(values) - len(v))
    if not n:
        return out

    def quantile(q):
        h = q * (n - 1)
        i = min(int(math.floor(h)), n - 1)
        return v[i] + (h - i) * (v[min(i + 1, n - 1)] - v[i])
    mean = math.fsum(v) / n
    out.update(mean=mean, std=math.sqrt(math.fsum((x - mean) ** 2 for x in v) / n), lo=quantile((1 - level) / 2),
               hi=quantile(1 - (1 - level) / 2))
    return out


def bootstrap_lines(metrics, estimates, replicate_values, cfg):
    """the BOOTSTRAP_COLUMNS lines of one summary: per metric its estimate (the cell of the results file, as written there) and the
    interval of its column of replicate_values [R][len(metrics)].  cfg: what engine.check_bootstrap returned"""
    lines = []
    for k, (name, estimate) in enumerate(zip(metrics, estimates)):
        b = bootstrap_interval([r[k] for r in replicate_values], cfg['level'])
        lines.append([name, estimate, _blank(b['mean']), _blank(b['std']), _blank(b['lo']), _blank(b['hi']), repr(cfg['level']),
                      len(replicate_values), b['undefined'], cfg['seed'], int(cfg['stratified'])])
    return lines


def detection_replicate_line(replicate, row, values):
    """the DETECTION_REPLICATE_COLUMNS line of one replicate: its number, the row's integers and detection_replicate_values"""
    return ([int(replicate)] + [int(row[k]) for k in DETECTION_REPLICATE_INTEGERS[:7]] + [int(t) for t in row['tp_at']] +
            [_blank(v) for v in values])


# ---- `annotator evaluate --surface_distances`: how far the predicted outline lies from the labelled one ----------------------------
# DeviceModel.surface_distances gives, per boundary pixel of either mask, the exact squared distance to the nearest boundary pixel of
# the other mask; everything here is float64 from those integers, d = sqrt(d2).  Distances are in pixels of the analysed plane and
# in-plane: slices have no spacing.
SURFACE_STATUSES = ['both', 'pred_only', 'label_only', 'neither', 'truncated']
SURFACE_SLICE_COLUMNS = ['exam', 'slice', 'status', 'area_pred', 'area_true', 'common', 'edge_pred', 'edge_true', 'dice', 'hd',
                         'hd_percentile', 'assd']
SURFACE_CASE_COLUMNS = ['exam', 'slices'] + SURFACE_STATUSES + ['hd', 'hd_percentile', 'assd']
SURFACE_RESULT_COLUMNS = ['slices'] + SURFACE_STATUSES + ['exams', 'dice', 'hd', 'hd_percentile', 'assd', 'exam_hd',
                                                           'exam_hd_percentile', 'exam_assd']
SURFACE_PERCENTILE = 95.0


def surface_distance_values(d2_pred, d2_true, percentile=SURFACE_PERCENTILE):
    """squared distances of the prediction's and of the label's boundary pixels (both non-empty) -> (hd, hd_percentile, assd) as
    float64: the largest d of either side, numpy.percentile (linear interpolation) over the d of both sides concatenated, the mean
    of the two sides' mean d"""
    dp, dt = np.sqrt(np.asarray(d2_pred, np.float64)), np.sqrt(np.asarray(d2_true, np.float64))
    if not (dp.size and dt.size):
        raise ValueError('surface distances need samples of both sides, got %d and %d' % (dp.size, dt.size))
    both = np.concatenate([dp, dt])
    return float(both.max()), float(np.percentile(both, float(percentile))), float((dp.mean() + dt.mean()) / 2.0)


def surface_status(counts, n_pred, n_true):
    """counts (area_pred, area_true, common, edge_pred, edge_true) of one slice and the samples that came back for either side ->
    its status.  A slice with both outlines and no samples was cut by max_samples"""
    edge_pred, edge_true = int(counts[3]), int(counts[4])
    if edge_pred > 0 and edge_true > 0:
        if n_pred == 0 and n_true == 0:
            return 'truncated'
        if (n_pred, n_true) != (edge_pred, edge_true):
            raise ValueError('surface distances: %d / %d samples for %d / %d boundary pixels' % (n_pred, n_true, edge_pred, edge_true))
        return 'both'
    if n_pred or n_true:
        raise ValueError('surface distances: samples of a slice with an empty outline')
    return 'pred_only' if edge_pred > 0 else 'label_only' if edge_true > 0 else 'neither'


def surface_slice_values(exam, slice_id, counts, d2_pred, d2_true, percentile=SURFACE_PERCENTILE):
    """the surface_slices.csv values of one slice (SURFACE_SLICE_COLUMNS).  dice = 2 common / (area_pred + area_true), blank when
    both masks are empty; hd, hd_percentile and assd (surface_distance_values) are blank unless the status is `both`.  Floats are
    written with repr"""
    status = surface_status(counts, len(d2_pred), len(d2_true))
    total = int(counts[0]) + int(counts[1])
    dice = repr(2 * int(counts[2]) / total) if total else ''
    dist = [repr(v) for v in surface_distance_values(d2_pred, d2_true, percentile)] if status == 'both' else ['', '', '']
    return [exam, int(slice_id), status] + [int(c) for c in counts[:5]] + [dice] + dist


def surface_exam_values(exam, slices, percentile=SURFACE_PERCENTILE):
    """the surface_cases.csv values of one exam (SURFACE_CASE_COLUMNS).  slices: [(counts, d2_pred, d2_true)] of the exam's slices;
    the samples of its `both` slices are pooled per side and go through surface_distance_values; blank without such a slice"""
    status = [surface_status(c, len(p), len(t)) for c, p, t in slices]
    pooled = [[np.asarray(sl[side], np.int64) for sl, st in zip(slices, status) if st == 'both'] for side in (1, 2)]
    dist = ['', '', '']
    if pooled[0]:
        dist = [repr(v) for v in surface_distance_values(np.concatenate(pooled[0]), np.concatenate(pooled[1]), percentile)]
    return [exam, len(slices)] + [status.count(s) for s in SURFACE_STATUSES] + dist


def surface_summary(slice_values, exam_values):
    """the SURFACE_SLICE_COLUMNS values of every slice and the SURFACE_CASE_COLUMNS values of every exam -> the
    SURFACE_RESULT_COLUMNS values: the slice counts per status, the exams that have a `both` slice, the means of dice, hd,
    hd_percentile and assd over the `both` slices and of the three per-exam distances over those exams (blank without any)"""
    def mean(values):
        values = [float(v) for v in values]
        return repr(float(np.mean(np.asarray(values, np.float64)))) if values else ''
    both = [v for v in slice_values if v[2] == 'both']
    exams = [v for v in exam_values if v[-1] != '']
    return ([len(slice_values)] + [sum(1 for v in slice_values if v[2] == s) for s in SURFACE_STATUSES] + [len(exams)] +
            [mean(v[i] for v in both) for i in (8, 9, 10, 11)] + [mean(v[i] for v in exams) for i in (-3, -2, -1)])


# ---- `annotator predict --lesion_features`: what a lesion looks like in the input channels -------------------------------------------
# DeviceModel.lesion_table_features gives, per lesion, integer moments and outline counts (shape), and per lesion and modality the
# pixel count, float32 extrema and the integer sums of q = rint(v * 2^16) and q^2 of the lesion's own pixels (body) and of the
# background around it (ring), plus a histogram of the body.  Every difference of products is taken in Python integers before the
# one float64 division; floats are written with repr, float32 extrema with the 9 digits that give them back.
FEATURE_BINS = 32                # --feature_bins
FEATURE_RING = 3                 # --feature_ring
FEATURE_BIN_RANGE = (0, 256)     # what the library accepts
FEATURE_RING_RANGE = (0, 8)
FEATURE_PERCENTILES = (10, 50, 90)
FEATURE_SHAPE_COLUMNS = ['boundary_px', 'edge_len', 'extent', 'major_axis', 'minor_axis', 'eccentricity', 'orientation_deg']
Q16 = float(1 << 16)             # sum_q16 is the sum of rint(v * 2^16)


def check_features(lesion_features, bins=None, ring=None):
    """the values of --feature_bins / --feature_ring (None: not given) -> (bins, ring) with the defaults filled in.  They mean
    nothing without --lesion_features"""
    if not lesion_features:
        if bins is not None or ring is not None:
            raise ValueError('--feature_bins / --feature_ring set the histogram and the ring of --lesion_features: add --lesion_features')
        return None, None
    bins = FEATURE_BINS if bins is None else int(bins)
    ring = FEATURE_RING if ring is None else int(ring)
    if not FEATURE_BIN_RANGE[0] <= bins <= FEATURE_BIN_RANGE[1]:
        raise ValueError('--feature_bins %d outside %d..%d' % ((bins,) + FEATURE_BIN_RANGE))
    if not FEATURE_RING_RANGE[0] <= ring <= FEATURE_RING_RANGE[1]:
        raise ValueError('--feature_ring %d outside %d..%d' % ((ring,) + FEATURE_RING_RANGE))
    return bins, ring


def feature_intensity_columns(names):
    cols = []
    for m in names:
        cols += ['%s_%s' % (c, m) for c in ['mean', 'std', 'min', 'max'] + ['p%d' % p for p in FEATURE_PERCENTILES] +
                 ['ring_px', 'ring_mean', 'ring_std', 'contrast']]
    return cols


def lesion_feature_columns(names):
    return ['exam', 'slice', 'lesion'] + FEATURE_SHAPE_COLUMNS + feature_intensity_columns(names)


def exam_lesion_feature_columns(names):
    return ['exam', 'exam_lesion', 'surface_px'] + feature_intensity_columns(names)


def feature_shape_values(row, shape):
    """boundary_px, edge_len, extent (area / box area), major_axis and minor_axis (4 sqrt(lambda) of the coordinate covariance),
    eccentricity (sqrt(1 - lambda2 / lambda1); 0 for a point) and orientation_deg (0.5 atan2(2 cxy, cxx - cyy): the major axis
    against the x axis, y pointing down) of one lesion: `row` its record of lesion_table's rows, `shape` the shape record beside it"""
    if (int(shape['row']), int(shape['area'])) != (int(row['row']), int(row['area'])):
        raise ValueError('shape record of lesion %d (%d px) beside lesion %d (%d px)' % (shape['row'], shape['area'], row['row'], row['area']))
    n, sx, sy = int(row['area']), int(row['sum_x']), int(row['sum_y'])
    cxx = (n * int(shape['sum_xx']) - sx * sx) / (n * n)
    cyy = (n * int(shape['sum_yy']) - sy * sy) / (n * n)
    cxy = (n * int(shape['sum_xy']) - sx * sy) / (n * n)
    d = math.sqrt((cxx - cyy) ** 2 + 4.0 * cxy * cxy)
    l1, l2 = (cxx + cyy + d) / 2.0, max((cxx + cyy - d) / 2.0, 0.0)
    box = (int(row['x1']) - int(row['x0']) + 1) * (int(row['y1']) - int(row['y0']) + 1)
    return [int(shape['boundary']), int(shape['edges']), repr(n / box), repr(4.0 * math.sqrt(l1)), repr(4.0 * math.sqrt(l2)),
            repr(math.sqrt(max(1.0 - l2 / l1, 0.0)) if l1 > 0 else 0.0), repr(math.degrees(0.5 * math.atan2(2.0 * cxy, cxx - cyy)))]


def feature_percentile(hist, fraction, lo, hi):
    """the value below which `fraction` of the histogram's pixels lie: with t = fraction * n, k the first bin whose inclusive
    cumulative count reaches t: (k + (t - count before k) / count of k) / bins, clipped to [lo, hi] (the extrema of the values)"""
    counts = [int(c) for c in hist]
    t, before = fraction * sum(counts), 0
    for k, c in enumerate(counts):
        if before + c >= t and c:
            return min(max((k + (t - before) / c) / len(counts), lo), hi)
        before += c
    raise ValueError('feature_percentile: an empty histogram')


def pool_intensity(records):
    """body or ring records of one modality (one per part; None: none) -> (n, sum_q16, sum_sq_q16, min, max) over all their pixels;
    records without a pixel have no extrema"""
    held = [r for r in records or [] if int(r['n'])]
    return (sum(int(r['n']) for r in held), sum(int(r['sum_q16']) for r in held), sum(int(r['sum_sq_q16']) for r in held),
            min([float(r['min']) for r in held], default=0.0), max([float(r['max']) for r in held], default=0.0))


def _mean_std(n, sq, ssq):
    """mean and population standard deviation from the integer sums of q and q^2 over n pixels"""
    return sq / n / Q16, math.sqrt(n * ssq - sq * sq) / n / Q16


def feature_intensity_values(body, ring, hist):
    """the cells of one modality: body / ring: (n, sum_q16, sum_sq_q16, min, max) as pool_intensity gives them (ring None: the ring
    is off), hist: the body's counts per bin (None: --feature_bins 0).  Blank: the percentiles without a histogram; ring_px,
    ring_mean, ring_std and contrast with the ring off; the last three also for a ring without a pixel"""
    n, sq, ssq, lo, hi = body
    mean, std = _mean_std(n, sq, ssq)
    cells = [repr(mean), repr(std), '%.9g' % lo, '%.9g' % hi]
    cells += ['' if hist is None else repr(feature_percentile(hist, p / 100.0, lo, hi)) for p in FEATURE_PERCENTILES]
    if ring is None:
        return cells + ['', '', '', '']
    if not ring[0]:
        return cells + [0, '', '', '']
    ring_mean, ring_std = _mean_std(*ring[:3])
    return cells + [int(ring[0]), repr(ring_mean), repr(ring_std), repr(mean - ring_mean)]


def lesion_feature_values(exam, slice_id, row, shape, body, ring, hist):
    """the lesion_features.csv line of one lesion: `row` its record of lesion_table's rows; shape, body [C], ring [C] or None, hist
    [C, bins] or None: the records of lesion_table_features beside it"""
    cells = [exam, int(slice_id), int(row['row'])] + feature_shape_values(row, shape)
    for c in range(len(body)):
        if (int(body[c]['row']), int(body[c]['n'])) != (int(row['row']), int(row['area'])):
            raise ValueError('body record of lesion %d (%d px) beside lesion %d (%d px)' % (body[c]['row'], body[c]['n'], row['row'], row['area']))
        cells += feature_intensity_values(pool_intensity([body[c]]), None if ring is None else pool_intensity([ring[c]]),
                                          None if hist is None else hist[c])
    return cells


def exam_lesion_feature_values(exam, exam_lesion, parts):
    """the exam_lesion_features.csv line of one exam lesion.  parts: the (shape, body, ring, hist) of its 2-D lesions.  Pooled from
    the summed integers, the extrema and the summed histograms of the parts -- the values of all their pixels together, never a
    mean of means; surface_px: the parts' edge_len summed (the faces towards the slices above and below are not counted)"""
    cells = [exam, int(exam_lesion), sum(int(s['edges']) for s, _, _, _ in parts)]
    _, body0, ring0, hist0 = parts[0]
    for c in range(len(body0)):
        hist = None if hist0 is None else [sum(col) for col in zip(*[[int(v) for v in h[c]] for _, _, _, h in parts])]
        cells += feature_intensity_values(pool_intensity([b[c] for _, b, _, _ in parts]),
                                          None if ring0 is None else pool_intensity([r[c] for _, _, r, _ in parts]), hist)
    return cells


# ---- `--uncertainty`: how much the test-time-augmentation views disagree ------------------------------------------------------------
# DeviceModel.lesion_table_spread and spread_by_outcome give integer sums of rint(spread * 2^24) and float32 maxima; a mean is
# sum / pixels / 2^24 in float64 (repr), a maximum is written with the 9 digits that give the float32 back.
LESION_UNCERTAINTY_COLUMNS = ['exam', 'slice', 'lesion', 'mean_spread', 'max_spread']
SLICE_UNCERTAINTY_COLUMNS = ['exam', 'slice', 'mean_spread', 'max_spread', 'mean_spread_in_lesions', 'truncated']
OUTCOMES = ['tn', 'fp', 'fn', 'tp']      # class 2 (y > 0.5) + (prob >= threshold)
UNCERTAINTY_SLICE_COLUMNS = (['exam', 'slice'] + ['%s_px' % o for o in OUTCOMES] + ['mean_spread_%s' % o for o in OUTCOMES] +
                             ['mean_spread_wrong', 'mean_spread_right', 'wrong_to_right'])
UNCERTAINTY_RESULT_COLUMNS = ['slices'] + UNCERTAINTY_SLICE_COLUMNS[2:]
UNCERTAINTY_WHITE = 510.0        # uncertainty.png: grey = min(255, rint(spread * 510)), a spread of 0.5 is white


def _mean_q24(total, pixels):
    return repr(int(total) / int(pixels) / Q24) if int(pixels) else ''


def lesion_uncertainty_values(exam, slice_id, row, srow):
    """the lesion_uncertainty.csv line of one lesion: `row` its record of lesion_table's rows, `srow` the spread record beside it"""
    if (int(srow['row']), int(srow['area'])) != (int(row['row']), int(row['area'])):
        raise ValueError('spread record of lesion %d (%d px) beside lesion %d (%d px)' % (srow['row'], srow['area'], row['row'], row['area']))
    return [exam, int(slice_id), int(row['row']), _mean_q24(srow['sum_spread_q24'], row['area']), '%.9g' % float(srow['max_spread'])]


def slice_uncertainty_values(exam, slice_id, rows, srows, total, stotal):
    """the slice_uncertainty.csv line of one slice: mean and maximum over every pixel of the analysed plane (`stotal`), the mean over
    the pixels of the listed lesions (blank without any), truncated as in slices.csv"""
    area = sum(int(r['area']) for r in rows)
    return [exam, int(slice_id), _mean_q24(stotal['sum_spread_q24'], stotal['pixels']), '%.9g' % float(stotal['max_spread']),
            _mean_q24(sum(int(r['sum_spread_q24']) for r in srows), area), int(int(total) > len(rows))]


def _outcome_values(n, q):
    """pixels n [4] and q24 sums q [4] of TN, FP, FN, TP -> the values from tn_px on"""
    n, q = [int(v) for v in n], [int(v) for v in q]
    wrong, right = _mean_q24(q[1] + q[2], n[1] + n[2]), _mean_q24(q[0] + q[3], n[0] + n[3])
    ratio = repr(float(wrong) / float(right)) if wrong and right and float(right) > 0 else ''
    return n + [_mean_q24(q[c], n[c]) for c in range(4)] + [wrong, right, ratio]


def outcome_slice_values(exam, slice_id, outcome):
    """one entry of spread_by_outcome (n [4], sum_q24 [4]) -> the uncertainty_slices.csv values of its slice"""
    return [exam, int(slice_id)] + _outcome_values(outcome['n'], outcome['sum_q24'])


def outcome_summary(outcomes):
    """the entries of all slices at one threshold -> the uncertainty_results.csv values: the sums over the slices"""
    n = [sum(int(o['n'][c]) for o in outcomes) for c in range(4)]
    q = [sum(int(o['sum_q24'][c]) for o in outcomes) for c in range(4)]
    return [len(outcomes)] + _outcome_values(n, q)


# `--ensemble ... --uncertainty`: the spread of an ensemble in its two components.  between: how much the members' means disagree;
# within: the root mean square of the members' own view spreads; total^2 = between^2 + within^2 is what every other file reads
ENSEMBLE_COMPONENTS = ['between', 'within', 'total']
ENSEMBLE_UNCERTAINTY_RESULT_COLUMNS = (['slices'] + ['%s_px' % o for o in OUTCOMES] +
                                       sum([['mean_%s_%s' % (c, o) for o in OUTCOMES + ['wrong', 'right']] + ['%s_wrong_to_right' % c]
                                            for c in ENSEMBLE_COMPONENTS], []))
SLICE_ENSEMBLE_UNCERTAINTY_COLUMNS = ['exam', 'slice', 'mean_between', 'max_between', 'mean_within', 'max_within']


def ensemble_outcome_summary(between, within, total):
    """the spread_by_outcome entries of all slices at one threshold on the three planes -> the ensemble_uncertainty_results.csv
    values: the pixels per outcome (the same on every plane: the classes come from the mean), then per component what
    outcome_summary gives behind them"""
    sums = [outcome_summary(list(o)) for o in (between, within, total)]
    if len({tuple(s[:5]) for s in sums}) != 1:
        raise ValueError('the three spread planes of an ensemble were classed differently: %s' % [s[:5] for s in sums])
    return sums[0][:5] + sum([s[5:] for s in sums], [])


def slice_ensemble_uncertainty_values(exam, slice_id, between, within):
    """the slice_ensemble_uncertainty.csv line of one slice from its two planes [h, w] read back: mean (float64) and maximum"""
    out = [exam, int(slice_id)]
    for plane in (between, within):
        plane = np.asarray(plane, np.float32)
        out += [repr(float(plane.astype(np.float64).mean())), '%.9g' % float(plane.max())]
    return out


def uncertainty_image(spread):
    """float32 spread [h, w] -> uint8 grey: min(255, rint(spread * 510)) (the product is exact in float64)"""
    return np.minimum(255, np.rint(np.asarray(spread, np.float32).astype(np.float64) * UNCERTAINTY_WHITE)).astype(np.uint8)


def uncertainty_path(root, tag):
    """<root>/<last 3 components of the exam path>/<sliceID %02d>/uncertainty.png"""
    return os.path.join(export_dir(root, '', tag), 'uncertainty.png')


# ---- `--calibration`: can the probability be believed? ------------------------------------------------------------------------------
# DeviceModel.calibration gives exact integers per slice -- pixels and sums of q = rint(p * 2^24) per bin and class, the sum of q^2
# per class in two words -- and the NLL sums at a grid of temperatures in float64.  Everything here is Python integers and float64:
# a pooled value comes from the integer tables summed over the slices and from the NLL rows summed, never from per-slice values.
CALIBRATION_RESULT_COLUMNS = ['pixels', 'positives', 'mean_prob', 'prevalence', 'ece', 'mce', 'brier', 'nll', 'temperature',
                              'nll_at_temperature', 'at_grid_edge']
CALIBRATION_BIN_COLUMNS = ['bin', 'lower', 'upper', 'pixels', 'positives', 'mean_prob', 'frequency', 'gap']
CALIBRATION_SLICE_COLUMNS = ['exam', 'slice', 'pixels', 'positives', 'ece', 'brier', 'nll']
CALIBRATION_BINS = 15
CALIBRATION_GRID = tuple(2.0 ** ((j - 20) / 10.0) for j in range(41))       # 0.25 .. 4, ten points per octave
CALIBRATION_MAX_TEMPERATURES = 64                                            # one DeviceModel.calibration call
TEMPERATURE_RANGE = (0.05, 20.0)                                             # what the library accepts


def calibration_grid(temperatures=None):
    """the temperatures of one calibration call: the given ones (None: CALIBRATION_GRID) as float32 values, sorted, without
    duplicates, with T = 1 added when it is missing"""
    t = sorted(set(float(np.float32(v)) for v in (CALIBRATION_GRID if temperatures is None else temperatures)) | {1.0})
    if len(t) > CALIBRATION_MAX_TEMPERATURES:
        raise ValueError('--calibration_temperatures: %d temperatures (T = 1 included), at most %d' % (len(t), CALIBRATION_MAX_TEMPERATURES))
    if not all(TEMPERATURE_RANGE[0] <= v <= TEMPERATURE_RANGE[1] for v in t):
        raise ValueError('--calibration_temperatures: every temperature must lie in [%g, %g]' % TEMPERATURE_RANGE)
    return t


def calibration_counts(bins):
    """bin records (n [2], sum_q24 [2]) of one slice [n_bins], or of several slices [S, n_bins] -> (n, q): per bin the Python
    integers [class 0, class 1], summed over the slices"""
    bins = np.asarray(bins)
    bins = bins.reshape((-1, bins.shape[-1]))
    n = [[sum(int(v) for v in bins['n'][:, k, c]) for c in (0, 1)] for k in range(bins.shape[1])]
    q = [[sum(int(v) for v in bins['sum_q24'][:, k, c]) for c in (0, 1)] for k in range(bins.shape[1])]
    return n, q


def calibration_table(bins):
    """the reliability table: per bin [bin, lower edge, upper edge, pixels, positives, mean probability, observed frequency, gap =
    |mean probability - frequency|]; the last three are None in an empty bin"""
    n, q = calibration_counts(bins)
    rows = []
    for k, ((n0, n1), (q0, q1)) in enumerate(zip(n, q)):
        pixels = n0 + n1
        mean = (q0 + q1) / Q24 / pixels if pixels else None
        freq = n1 / pixels if pixels else None
        rows.append([k, k / len(n), (k + 1) / len(n), pixels, n1, mean, freq, abs(mean - freq) if pixels else None])
    return rows


def calibration_errors(table):
    """(ECE, MCE) of a calibration_table: sum_k n_k / N |mean probability - frequency| over the non-empty bins, and the largest gap"""
    total = sum(r[3] for r in table)
    gaps = [(r[3], r[7]) for r in table if r[3]]
    if not total:
        return None, None
    return sum(n / total * g for n, g in gaps), max(g for _, g in gaps)


def brier_score(totals):
    """the mean of (p - class)^2 from the integers of one total record or of several: class 0 adds sum q^2, class 1
    n 2^48 - 2^25 sum q + sum q^2; all of it over 2^48 N"""
    totals = np.asarray(totals).reshape(-1)
    tot = lambda f, c: sum(int(v) for v in totals[f][:, c])
    sq = [(tot('sq_hi', c) << 32) + tot('sq_lo', c) for c in (0, 1)]
    n = [tot('n', c) for c in (0, 1)]
    if not n[0] + n[1]:
        return None
    return (sq[0] + (n[1] << 48) - (tot('sum_q24', 1) << 25) + sq[1]) / ((n[0] + n[1]) << 48)      # integers: one rounding


def fit_temperature(temperatures, nll):
    """the temperature with the smallest NLL: (temperature, NLL there, at_grid_edge).  The grid point with the smallest NLL; when it
    is interior, the vertex of the parabola through it and its two neighbours in (log T, NLL), clamped to their interval, and the
    parabola's value there; at an end of the grid that end, the grid's value and at_grid_edge = 1"""
    pts = sorted((float(t), float(v)) for t, v in zip(temperatures, nll))
    if not pts:
        raise ValueError('fit_temperature: no temperatures')
    i = min(range(len(pts)), key=lambda j: pts[j][1])
    if i == 0 or i == len(pts) - 1:
        return pts[i][0], pts[i][1], 1
    (x0, y0), (x1, y1), (x2, y2) = [(math.log(t), v) for t, v in pts[i - 1:i + 2]]
    den = (x1 - x0) * (y1 - y2) - (x1 - x2) * (y1 - y0)
    if den == 0:                                 # three equal values: the grid point
        return pts[i][0], y1, 0
    x = x1 - 0.5 * ((x1 - x0) ** 2 * (y1 - y2) - (x1 - x2) ** 2 * (y1 - y0)) / den
    x = min(max(x, x0), x2)
    y = (y0 * (x - x1) * (x - x2) / ((x0 - x1) * (x0 - x2)) + y1 * (x - x0) * (x - x2) / ((x1 - x0) * (x1 - x2)) +
         y2 * (x - x0) * (x - x1) / ((x2 - x0) * (x2 - x1)))
    return math.exp(x), y, 0


def _blank(v):
    return '' if v is None else repr(float(v))


def calibration_slice_values(exam, slice_id, bins, total, nll_at_1):
    """the calibration_slices.csv line of one slice: `bins` its [n_bins] records, `total` its total record, the NLL per pixel"""
    pixels = int(total['n'][0]) + int(total['n'][1])
    ece, _ = calibration_errors(calibration_table(bins))
    return [exam, int(slice_id), pixels, int(total['n'][1]), _blank(ece), _blank(brier_score(total)),
            _blank(float(nll_at_1) / pixels if pixels else None)]


def calibration_summary(bins, totals, temperatures, nll):
    """bins [S, n_bins], totals [S] and nll [S, T] of all slices -> (the calibration_results.csv values, the calibration_bins.csv
    lines): everything pooled from the summed integers and the summed NLL rows; NLL values are per pixel"""
    table = calibration_table(bins)
    pixels, positives = sum(r[3] for r in table), sum(r[4] for r in table)
    _, q = calibration_counts(bins)
    ece, mce = calibration_errors(table)
    curve = [math.fsum(col) / pixels if pixels else 0.0 for col in np.asarray(nll, np.float64).reshape(-1, len(temperatures)).T]
    at_1 = curve[[float(t) for t in temperatures].index(1.0)]
    t_fit, v_fit, edge = fit_temperature(temperatures, curve)
    result = [pixels, positives, _blank(sum(a + b for a, b in q) / Q24 / pixels if pixels else None),
              _blank(positives / pixels if pixels else None), _blank(ece), _blank(mce), _blank(brier_score(totals)), _blank(at_1),
              repr(t_fit), repr(v_fit), edge]
    lines = [r[:1] + [repr(r[1]), repr(r[2])] + r[3:5] + [_blank(v) for v in r[5:]] for r in table]
    return result, lines


def plain_csv(names, rows):
    """a header line and one line per row, csv-module quoting, no index column"""
    return _csv([list(names)] + [list(r) for r in rows])


def mask_path(root, tag):
    """<root>/<last 3 components of the exam path>/<sliceID %02d>/mask.png"""
    return os.path.join(export_dir(root, '', tag), 'mask.png')


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(img, level=PNG_LEVEL):
    """uint8 [h, w] / [h, w, 1] (8-bit grey) or [h, w, 3] (8-bit RGB) -> PNG bytes: one IDAT chunk, filter 0 on every row"""
    a = np.ascontiguousarray(img, np.uint8)
    if a.ndim == 2:
        a = a[..., None]
    h, w, c = a.shape
    if c not in (1, 3):
        raise ValueError('PNG: 1 or 3 channels, got %d' % c)
    raw = np.zeros((h, 1 + w * c), np.uint8)
    raw[:, 1:] = a.reshape(h, w * c)
    ihdr = struct.pack('>IIBBBBB', w, h, 8, 0 if c == 1 else 2, 0, 0, 0)
    return b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(raw.tobytes(), level)) + _chunk(b'IEND', b'')


def _write(path, make, *args):
    data = make(*args)
    if isinstance(data, str):
        data = data.encode()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'wb') as f:
        f.write(data)


class Writer:
    """Files of the Visualizer pass, encoded and written on up to MAX_WORKERS threads; at most `backlog` files wait at a time.
    close() waits for every file and raises the first error."""

    def __init__(self, workers=MAX_WORKERS, backlog=256):
        self.pool = ThreadPoolExecutor(max(1, min(int(workers), MAX_WORKERS)), thread_name_prefix='dnnca-casewise')
        self.backlog, self.pending = int(backlog), []

    def submit(self, path, make, *args):
        """writes make(*args) (bytes or str) to `path`, creating its directory"""
        self.pending.append(self.pool.submit(_write, path, make, *args))
        while len(self.pending) > self.backlog:
            self.pending.pop(0).result()

    def close(self):
        try:
            while self.pending:
                self.pending.pop(0).result()
        finally:
            self.pool.shutdown(wait=True)
