"""CPU: the host side of `annotator predict --link_slices` -- casewise.link_lesions (union-find over the links) and the numpy oracle
of the links (tests/link_oracle.py) against a brute-force 6-connected flood fill that shares no code with either, the table's
semantics on hand-drawn cases, the `continues` flags TFKerasModel.annotate derives (on a fake device that serves the oracles'
tables), the files it writes and the command-line flags."""

import csv
import io
import os

import numpy as np
import pytest

import lesion_oracle as LO
import link_cases as KC
import link_oracle as KO
from dnncancerannotator_amd import casewise as CW
from dnncancerannotator_amd.__main__ import build_parser
from fake_link_device import Slices, fake_engine


def exam_tables(prob, continues=None, exam='e', ids=None, min_overlap=1, **kw):
    """casewise.link_lesions fed with the oracles' rows and links of prob [B, H, W] (one exam): (table, parts, rows)"""
    B = len(prob)
    continues = [b > 0 for b in range(B)] if continues is None else continues
    ids = list(range(B)) if ids is None else ids
    rows, totals, _ = LO.lesion_table(prob, **kw)
    links = KO.links(prob, continues, **kw)
    slices = [(ids[b], rows[rows['slice'] == b], totals[b]) for b in range(B)]
    per = [[(l['row_prev'], l['row'], l['overlap']) for l in links[links['slice'] == b]] for b in range(B)]
    table, parts = CW.link_lesions(exam, slices, per, min_overlap=min_overlap)
    return table, parts, rows


def col(table, name):
    return [r[CW.EXAM_LESION_COLUMNS.index(name)] for r in table]


# ---- an independent statement: 6-connected components of the stacked masks ------------------------------------------------------
def flood_fill_3d(fg):
    """brute force: label [B, H, W] (-1 background) of the 6-connected components, numbered in (slice, row, column) order of their
    first voxel; one voxel at a time off a stack"""
    B, H, W = fg.shape
    lab = np.full(fg.shape, -1, np.int64)
    n = 0
    for b in range(B):
        for y in range(H):
            for x in range(W):
                if not fg[b, y, x] or lab[b, y, x] >= 0:
                    continue
                stack = [(b, y, x)]
                lab[b, y, x] = n
                while stack:
                    cb, cy, cx = stack.pop()
                    for db, dy, dx in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                        nb_, ny, nx = cb + db, cy + dy, cx + dx
                        if 0 <= nb_ < B and 0 <= ny < H and 0 <= nx < W and fg[nb_, ny, nx] and lab[nb_, ny, nx] < 0:
                            lab[nb_, ny, nx] = n
                            stack.append((nb_, ny, nx))
                n += 1
    return lab, n


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_exam_lesions_are_the_6_connected_components(seed):
    """6 x 12 x 14 random volumes, k = 1, no area filter, no truncation, min_overlap 1: membership, numbering and volumes"""
    rng = np.random.default_rng(seed)
    fg = rng.random((6, 12, 14)) < (0.35, 0.45, 0.5, 0.55)[seed]
    prob = np.where(fg, 0.75, 0.25).astype(np.float32)
    kw = dict(threshold=0.5, rf=1.0, k=1, min_area=0, max_lesions=1 << 20)
    table, parts, rows = exam_tables(prob, **kw)
    lab, n = flood_fill_3d(fg)
    assert n > 3 and len(table) == n and col(table, 'exam_lesion') == list(range(n))
    assert col(table, 'volume_px') == [int((lab == i).sum()) for i in range(n)]
    # every 2-D lesion lies, with all its pixels, in the component its part line names
    maps = KO.row_maps(prob, **kw).reshape(6, 12, 14)
    assert len(parts) == len(rows)
    for (exam, k, lesion, exam_lesion), r in zip(parts, rows):
        assert (k, lesion) == (r['slice'], r['row'])
        inside = lab[k][maps[k] == lesion]
        assert len(inside) == r['area'] and (inside == exam_lesion).all()
    assert col(table, 'n_parts') == [sum(1 for p in parts if p[3] == i) for i in range(n)]
    assert col(table, 'first_slice') == [int(np.nonzero((lab == i).any(axis=(1, 2)))[0][0]) for i in range(n)]
    assert col(table, 'n_slices') == [int((lab == i).any(axis=(1, 2)).sum()) for i in range(n)]


# ---- the oracle of the links by hand -------------------------------------------------------------------------------------------
def test_link_oracle_by_hand():
    prob, spec = KC.checker_on_checker()
    links = KO.links(prob, [0, 1], max_lesions=512, **spec)
    assert len(links) == 512 and links['slice'].tolist() == [1] * 512
    assert links['row_prev'].tolist() == links['row'].tolist() == list(range(512)) and links['overlap'].tolist() == [1] * 512
    few = KO.links(prob, [0, 1], max_lesions=16, **spec)
    assert few['row'].tolist() == list(range(16)) and len(KO.links(prob, [0, 0], max_lesions=512, **spec)) == 0
    prob, spec = KC.crossing_stripes()
    links = KO.links(prob, [0, 1], **spec)
    assert [(l['row_prev'], l['row']) for l in links] == [(c, r) for c in range(16) for r in range(16)] and set(links['overlap']) == {1}
    prob, spec = KC.full_planes()
    assert KO.links(prob, [0, 1, 1], **spec).tolist() == [(1, 0, 0, 72 * 80), (2, 0, 0, 12)]
    prob, spec = KC.shifted_snake()
    links = KO.links(prob, [0, 1], **spec)
    assert links.tolist() == [(1, 1, 1, 126), (1, 2, 2, 54)]      # the snake's two horizontal arms; the blocks; the pixels miss
    prob, spec = KC.graded_half()
    assert [l[:3] for l in KO.links(prob, [0, 1], **spec).tolist()] == [(1, 0, 0), (1, 1, 1), (1, 1, 2)]
    assert [l[:3] for l in KO.links(prob, [0, 1], min_area=40, **spec).tolist()] == [(1, 0, 1)]
    maps = KO.row_maps(prob, min_area=40, **spec).reshape(2, 20, 24)
    assert maps[0, 3, 3] == -1 and maps[0, 10, 10] == 0 and maps[1, 12, 3] == -1 and maps[1, 4, 4] == 0 and maps[1, 15, 15] == 1
    # a call boundary: A B | C with the carry of B is A B C
    prob, spec = KC.three_blocks()
    whole = KO.links(prob, [0, 1, 1], **spec)
    head = KO.links(prob[:2], [0, 1], **spec)
    tail = KO.links(prob[2:], [1], carry=KO.row_maps(prob[:2], **spec)[-1], **spec)
    tail['slice'] += 2
    assert len(tail) == 3 and np.concatenate([head, tail]).tolist() == whole.tolist()


@pytest.mark.parametrize('name', sorted(KC.ALL))
def test_float32_and_float64_resize_give_the_same_cases(name):
    """no drawn case hangs on how a product or a sum of the resize was rounded (as for tests/lesion_cases.py)"""
    prob, spec = KC.ALL[name]()
    assert np.array_equal(np.round(prob * 64), prob * 64)
    a = LO.lesion_table(prob, spec['threshold'], spec['rf'], spec['k'], max_lesions=512)
    b = LO.lesion_table(prob, spec['threshold'], spec['rf'], spec['k'], max_lesions=512, resize=LO.resize64)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist() and np.array_equal(a[2], b[2])


# ---- the table's semantics ------------------------------------------------------------------------------------------------------
def _draw(*slices, shape=(8, 10)):
    """each slice: a list of (y0, y1, x0, x1, p) blocks -> prob [B, H, W]"""
    prob = np.zeros((len(slices),) + shape, np.float32)
    for b, blocks in enumerate(slices):
        for y0, y1, x0, x1, p in blocks:
            prob[b, y0:y1, x0:x1] = p
    return prob


KW = dict(threshold=0.5, rf=1.0, k=1)


def test_y_shaped_lesion_aggregates_and_centroid_slice():
    """two parts in slice 4 joined by slice 5, and a lesion of its own in slice 5 that comes first in raster order"""
    prob = _draw([(2, 4, 1, 3, 0.75), (2, 4, 6, 9, 0.5)], [(0, 1, 0, 2, 0.625), (3, 4, 2, 7, 1.0)])
    table, parts, rows = exam_tables(prob, exam='/d/p/e', ids=[4, 5], **KW)
    assert [p[1:] for p in parts] == [[4, 0, 0], [4, 1, 0], [5, 0, 1], [5, 1, 0]]
    y, alone = table
    assert y == ['/d/p/e', 0, 4, 5, 2, 3, 4 + 6 + 5, 1, 2, 8, 3,
                 repr((2 * (1 + 2) + 2 * (6 + 7 + 8) + (2 + 3 + 4 + 5 + 6)) / 15), repr((2 * (2 + 3) + 3 * (2 + 3) + 5 * 3) / 15),
                 repr((4 * 10 + 5 * 5) / 15), repr((4 * 0.75 + 6 * 0.5 + 5 * 1.0) / 15), '1', 0]
    assert alone[:7] == ['/d/p/e', 1, 5, 5, 1, 1, 2] and alone[-2:] == ['0.625', 0]
    text = CW.plain_csv(CW.EXAM_LESION_COLUMNS, table)
    assert text.splitlines()[0] == ('exam,exam_lesion,first_slice,last_slice,n_slices,n_parts,volume_px,x0,y0,x1,y1,centroid_x,centroid_y,'
                                    'centroid_slice,mean_prob,max_prob,truncated')
    back = list(csv.DictReader(io.StringIO(text)))
    assert float(back[0]['centroid_slice']) == 65 / 15 and back[1]['centroid_slice'] == '5.0'
    assert CW.plain_csv(CW.EXAM_PART_COLUMNS, parts).splitlines()[:2] == ['exam,slice,lesion,exam_lesion', '/d/p/e,4,0,0']


def test_min_overlap_and_numbering_order():
    """slice 0: P (rows 1..2), Q (rows 5..6); slice 1: one block on 1 pixel of P and 4 of Q, and R first in raster order"""
    prob = _draw([(1, 3, 1, 3, 0.75), (5, 7, 1, 3, 0.75)], [(0, 1, 8, 9, 0.75), (2, 7, 2, 4, 0.75)])
    links = KO.links(prob, [0, 1], **KW)
    assert links.tolist() == [(1, 0, 1, 1), (1, 1, 1, 2)]
    table, parts, _ = exam_tables(prob, **KW)
    assert [p[1:] for p in parts] == [[0, 0, 0], [0, 1, 0], [1, 0, 1], [1, 1, 0]] and col(table, 'n_parts') == [3, 1]
    table, parts, _ = exam_tables(prob, min_overlap=2, **KW)
    # P is alone now; exam lesions are numbered by their first member: P (slice 0, lesion 0), Q + block (slice 0, lesion 1), R
    assert [p[3] for p in parts] == [0, 1, 2, 1] and col(table, 'n_parts') == [1, 2, 1] and col(table, 'first_slice') == [0, 0, 1]
    table, parts, _ = exam_tables(prob, min_overlap=3, **KW)
    assert [p[3] for p in parts] == [0, 1, 2, 3] and col(table, 'volume_px') == [4, 4, 1, 10]


def test_truncated_and_unlinked_beyond_max_lesions():
    """slice 0 holds three lesions, max_lesions = 2: the third is in no table and links to nothing; every exam lesion that touches
    slice 0 is marked truncated, the one that lives in slice 1 alone is not"""
    prob = _draw([(0, 2, 0, 2, 0.75), (0, 2, 4, 6, 0.75), (4, 6, 0, 2, 0.75)], [(1, 2, 1, 5, 0.75), (5, 6, 1, 2, 0.75)])
    table, parts, rows = exam_tables(prob, max_lesions=2, **KW)
    assert len(rows) == 4 and [p[1:] for p in parts] == [[0, 0, 0], [0, 1, 0], [1, 0, 0], [1, 1, 1]]
    assert col(table, 'truncated') == [1, 0] and col(table, 'n_parts') == [3, 1]
    table, parts, _ = exam_tables(prob, max_lesions=3, **KW)
    assert col(table, 'truncated') == [0, 0] and col(table, 'n_parts') == [3, 2]


def test_a_cleared_flag_breaks_the_chain_and_bad_links_are_refused():
    prob = _draw([(1, 3, 1, 3, 0.75)], [(1, 3, 1, 3, 0.75)], [(1, 3, 1, 3, 0.75)])
    assert col(exam_tables(prob, **KW)[0], 'n_slices') == [3]
    table, parts, _ = exam_tables(prob, continues=[0, 1, 0], ids=[0, 1, 5], **KW)
    assert col(table, 'n_slices') == [2, 1] and col(table, 'first_slice') == [0, 5] and [p[3] for p in parts] == [0, 0, 1]
    assert CW.link_lesions('e', [], []) == ([], [])
    rows = LO.lesion_table(prob, **KW)[0]
    with pytest.raises(ValueError):
        CW.link_lesions('e', [(0, rows[:1], 1)], [[(0, 0, 4)]])                       # a link into the first slice
    with pytest.raises(ValueError):
        CW.link_lesions('e', [(0, rows[:1], 1), (1, rows[1:2], 1)], [[], [(0, 1, 4)]])    # a row the slice does not have
    with pytest.raises(ValueError):
        CW.link_lesions('e', [(0, rows[:1], 1)], [])


# ---- annotate on a fake device ---------------------------------------------------------------------------------------------------
def _run(tmp_path, monkeypatch, prob, exams, ids, batch, max_batch=None, **kw):
    e = fake_engine(monkeypatch, max_batch)
    ds = Slices(prob, exams, ids, batch)
    e._build(ds)
    e.current_step = 1
    e.save(str(tmp_path / 'run' / 'checkpoints' / 'ckpt-1'))
    out = str(tmp_path / ('out%d' % len(os.listdir(str(tmp_path)))))
    res = e.annotate(ds, str(tmp_path / 'run'), out, threshold=0.5, filter_size=1, **kw)
    texts = {}
    for name in sorted(os.listdir(out)):
        with open(os.path.join(out, name), newline='') as f:
            texts[name] = f.read()
    return res, texts, [c for c in e.device_model.calls if c[0].startswith('lesion')]


def test_annotate_derives_the_flags_and_writes_the_exam_tables(tmp_path, monkeypatch):
    """7 slices of one column of pixels each: exam a slices 0 1 2 (3 is missing) 4, exam b slices 0 1, exam a slice 5; data set
    batches of 4 on a device of 3 slices per call: calls of 3, 1, 3"""
    prob = np.zeros((7, 8, 10), np.float32)
    prob[:, 2:5, 3:6] = 0.75
    prob[5, 0, 9] = 0.75                                             # a second lesion in b 1
    exams, ids = ['a', 'a', 'a', 'a', 'b', 'b', 'a'], [0, 1, 2, 4, 0, 1, 5]
    res, texts, calls = _run(tmp_path, monkeypatch, prob, exams, ids, 4, max_batch=3, link_slices=True)
    assert calls == [('lesion_table_linked', 3, False, [False, True, True]),          # the first slice of the run never continues
                     ('lesion_table_linked', 1, False, [False]),                      # a 4 after a 2: a gap in the slice numbers
                     ('lesion_table_linked', 3, False, [False, True, False])]         # b 0; b 1; a 5 after b 1: another exam
    assert res == dict(step=1, slices=7, lesions=8, exam_lesions=5)
    assert sorted(texts) == ['exam_lesion_parts.csv', 'exam_lesions.csv', 'lesions.csv', 'slices.csv']
    table = list(csv.DictReader(io.StringIO(texts['exam_lesions.csv'])))
    assert [(r['exam'], r['exam_lesion'], r['first_slice'], r['last_slice'], r['n_parts']) for r in table] == [
        ('a', '0', '0', '2', '3'), ('a', '1', '4', '4', '1'), ('a', '2', '5', '5', '1'), ('b', '0', '0', '1', '2'), ('b', '1', '1', '1', '1')]
    parts = list(csv.DictReader(io.StringIO(texts['exam_lesion_parts.csv'])))
    lesions = list(csv.DictReader(io.StringIO(texts['lesions.csv'])))
    assert [(p['exam'], p['slice'], p['lesion']) for p in parts] == [(l['exam'], l['slice'], l['lesion']) for l in lesions]
    assert [p['exam_lesion'] for p in parts] == ['0', '0', '0', '1', '0', '1', '0', '2']
    # a split by max_batch in the middle of an exam links: one exam of 7 slices in calls of 3, 3, 1
    res, texts2, calls = _run(tmp_path, monkeypatch, prob, ['a'] * 7, range(7), 7, max_batch=3, link_slices=True, link_min_overlap=9)
    assert [c[3] for c in calls] == [[False, True, True], [True, True, True], [True]] and res['exam_lesions'] == 2
    assert _run(tmp_path, monkeypatch, prob, ['a'] * 7, range(7), 7, max_batch=3, link_slices=True, link_min_overlap=10)[0]['exam_lesions'] == 8
    # without the flag: the plain call, the two old files, and byte for byte what the linked run wrote into them
    res, plain, calls = _run(tmp_path, monkeypatch, prob, exams, ids, 4, max_batch=3)
    assert res == dict(step=1, slices=7, lesions=8) and [c[:2] for c in calls] == [('lesion_table', 3), ('lesion_table', 1), ('lesion_table', 3)]
    assert sorted(plain) == ['lesions.csv', 'slices.csv'] and all(plain[k] == texts[k] for k in plain)


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_parser_link_flags(capsys):
    p = build_parser()
    base = ['predict', '--save_path', 's', '--data_path', 'd', '--output', 'o']
    a = vars(p.parse_args(base))
    assert 'link_slices' not in a and 'link_min_overlap' not in a          # the defaults are those of runs.predict.predict
    a = vars(p.parse_args(base + ['--link_slices', '--link_min_overlap', '3']))
    assert a['link_slices'] is True and a['link_min_overlap'] == 3
    for bad in ('0', '-2', 'x'):
        with pytest.raises(SystemExit) as e:
            p.parse_args(base + ['--link_slices', '--link_min_overlap', bad])
        assert e.value.code == 2 and 'link_min_overlap' in capsys.readouterr().err
    import inspect
    from dnncancerannotator_amd.runs.predict import predict
    sig = inspect.signature(predict).parameters
    assert sig['link_slices'].default is False and sig['link_min_overlap'].default == 1
    with pytest.raises(ValueError, match='link_min_overlap'):
        predict('s', ['d'], 'o', link_slices=True, link_min_overlap=0)
