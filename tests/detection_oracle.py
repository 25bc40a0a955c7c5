"""The detection map of dnnca_detection_map, stated literally in numpy with a Python flood fill (no GPU, no library).

Per slice p [H, W] float32:
    w = min(max(p, 0), 1), a NaN counts as 0;  D = 0;  n = 0
    for round = 1 .. rounds:
        m = max(w);  s = the smallest pixel index with w == m;  if m < min_confidence: stop
        t = (float32) m * (float32) factor
        C = the 4-connected component of { w >= t } that contains s
        if |C| >= min_area: D[C] = m, candidate n = (seed s, area |C|, confidence m), n += 1;  else dropped += 1
        w[C] = 0;  if n == max_candidates: stop
    exhausted = all rounds spent, n < max_candidates and max(w) >= min_confidence
"""
import numpy as np

ROW_DTYPE = np.dtype([('slice', '<i4'), ('number', '<i4'), ('seed', '<i4'), ('area', '<i4'), ('confidence', '<f4')])
SLICE_DTYPE = np.dtype([('candidates', '<i4'), ('rounds', '<i4'), ('dropped', '<i4'), ('exhausted', '<i4')])


def flood(mask, seed):
    """the pixel indices of the 4-connected component of the boolean plane `mask` that contains the pixel index `seed`"""
    H, W = mask.shape
    seen = np.zeros(H * W, bool)
    seen[seed] = True
    stack, out = [seed], []
    flat = mask.reshape(-1)
    while stack:
        q = stack.pop()
        out.append(q)
        y, x = divmod(q, W)
        for ok, r in ((x > 0, q - 1), (x < W - 1, q + 1), (y > 0, q - W), (y < H - 1, q + W)):
            if ok and flat[r] and not seen[r]:
                seen[r] = True
                stack.append(r)
    return np.asarray(out, np.int64)


def detection_slice(p, min_confidence=0.1, factor=0.4, max_candidates=5, min_area=10, rounds=16):
    """one slice: (D [H, W] float32, [(seed, area, confidence)], (candidates, rounds, dropped, exhausted))"""
    p = np.asarray(p, np.float32)
    H, W = p.shape
    with np.errstate(invalid='ignore'):
        w = np.where(p > 0, np.minimum(p, np.float32(1)), np.float32(0)).astype(np.float32)      # NaN > 0 is False
    D = np.zeros((H, W), np.float32)
    c0, f = np.float32(min_confidence), np.float32(factor)
    found, spent, dropped, exhausted = [], 0, 0, 0
    while True:
        m = w.max()
        if m < c0:
            break
        if spent == rounds:
            exhausted = 1
            break
        s = int(np.argmax(w.reshape(-1) == m))
        t = np.float32(m * f)
        assert t.dtype == np.float32
        C = flood(w >= t, s)
        if C.size >= min_area:
            D.reshape(-1)[C] = m
            found.append((s, int(C.size), np.float32(m)))
        else:
            dropped += 1
        w.reshape(-1)[C] = 0
        spent += 1
        if len(found) == max_candidates:
            break
    return D, found, (len(found), spent, dropped, exhausted)


def detection_map(prob, **cfg):
    """prob [B, H, W] -> (D [B, H, W] float32, rows ROW_DTYPE sorted by (slice, number), slices SLICE_DTYPE [B])"""
    prob = np.asarray(prob, np.float32)
    D = np.zeros(prob.shape, np.float32)
    rows, slices = [], np.zeros(prob.shape[0], SLICE_DTYPE)
    for b in range(prob.shape[0]):
        D[b], found, rec = detection_slice(prob[b], **cfg)
        slices[b] = rec
        rows += [(b, k, s, a, m) for k, (s, a, m) in enumerate(found)]
    return D, np.array(rows, ROW_DTYPE), slices
