"""numpy statement of dnnca_lesion_table_matched, built on tests/link_oracle.py, tests/lesion_oracle.py and
tests/region_oracle.py by import.  The prediction plane is the linked call's.  The label plane goes through the same steps with
the threshold nextafter(0.5, 1) (y' > 0.5 in float32), no opening and no area filter.  The pairs of a slice are the distinct
(row of the labelled lesion, row of the predicted lesion) of its pixels that lie in both, with their number of pixels."""

import numpy as np

import lesion_oracle as LO
import link_oracle as KO

PAIR_DTYPE = np.dtype([('slice', '<i4'), ('row_true', '<i4'), ('row', '<i4'), ('overlap', '<i4')])
TRUE_THRESHOLD = np.nextafter(np.float32(0.5), np.float32(1))


def pred_maps(prob, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256):
    return KO.row_maps(prob, threshold, rf, k, min_area, max_lesions)


def true_maps(y, rf=1.0, max_lesions=256):
    return KO.row_maps(y, threshold=TRUE_THRESHOLD, rf=rf, k=1, min_area=0, max_lesions=max_lesions)


def pairs_of_maps(tmaps, pmaps):
    """int32 [B, hw] row maps of the label and the prediction -> pairs PAIR_DTYPE sorted by (slice, row_true, row)"""
    out = []
    for b in range(len(pmaps)):
        both = (tmaps[b] >= 0) & (pmaps[b] >= 0)
        if not both.any():
            continue
        pairs, n = np.unique(np.stack([tmaps[b][both], pmaps[b][both]], 1), axis=0, return_counts=True)
        out += [(b, int(t), int(p), int(m)) for (t, p), m in zip(pairs, n)]
    return np.array(out, PAIR_DTYPE)


def true_table(y, rf=1.0, max_lesions=256):
    """(rows, totals) of the label plane: the sums and the maximum are taken on the resized label values"""
    return LO.lesion_table(y, TRUE_THRESHOLD, rf, 1, 0, max_lesions)[:2]


def matched(prob, y, continues, threshold=0.5, rf=1.0, k=5, min_area=0, max_lesions=256, carry=None, true_carry=None):
    """the eight outputs of one call: (rows, totals, masks, links, true_rows, true_totals, true_links, pairs); carry / true_carry:
    the row maps of the last slice of the matched call before (pred_maps(...)[-1], true_maps(...)[-1])"""
    pm = pred_maps(prob, threshold, rf, k, min_area, max_lesions)
    tm = true_maps(y, rf, max_lesions)
    rows, totals, masks = LO.lesion_table(prob, threshold, rf, k, min_area, max_lesions)
    true_rows, true_totals = true_table(y, rf, max_lesions)
    return (rows, totals, masks, KO.links_of_maps(pm, continues, carry), true_rows, true_totals,
            KO.links_of_maps(tm, continues, true_carry), pairs_of_maps(tm, pm))
