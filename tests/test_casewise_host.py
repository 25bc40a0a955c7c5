"""CPU: the host side of the Visualizer pass of `annotator evaluate` (dnncancerannotator_amd/casewise.py): column names, CSV bytes
(pandas' to_csv where pandas is importable), export paths, the PNG writer, and the slice metadata of the data sets."""

import os
import struct
import zlib

import numpy as np
import pytest

from dnncancerannotator_amd import casewise as CW
from dnncancerannotator_amd import data, tfrecord as T


def test_column_names():
    names = CW.column_names()
    assert len(names) == 301 and names[-1] == 'tag'
    for j, kind in enumerate(('tp', 'fn', 'fp')):
        block = names[100 * j:100 * (j + 1)]
        assert len(set(block)) == 100
        assert all(n.startswith('region_%s@PixelThreshold' % kind) for n in block)
    th = [n.split('PixelThreshold')[1] for n in names[:100]]
    assert th[:3] == ['0.0', '0.01', '0.02'] and th[-1] == '1.0'
    assert th[5] == '0.051' and th[9] == '0.091' and '0.051' in th and '0.091' in th
    assert th == [f'{i / 99.0:.2}' for i in range(100)]          # callbacks.py's f-string on i / float(99)


def test_tag_and_row_values():
    assert CW.tag_of('/data/a/b/c', 7) == 'path:/data/a/b/c,sliceID:7'
    c = np.zeros((100, 4), np.int64)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = 1, 2, 3, 4
    v = CW.row_values(c, 't')
    assert v == [1] * 100 + [2] * 100 + [4] * 100 + ['t']


def test_series_csv_bytes():
    names = ['region_tp@PixelThreshold0.0', 'region_fn@PixelThreshold0.0', 'region_fp@PixelThreshold0.0', 'tag']
    values = [1, 0, 2, 'path:/x/y,sliceID:3']
    text = CW.series_csv(names, values)
    assert text == (',region_tp@PixelThreshold0.0,region_fn@PixelThreshold0.0,region_fp@PixelThreshold0.0,tag\n'
                    '0,1,0,2,"path:/x/y,sliceID:3"\n')
    pd = pytest.importorskip('pandas')
    series = pd.Series(dict(zip(names[:-1], np.array(values[:-1], np.int32)), tag=values[-1]))
    assert pd.DataFrame(series).T.to_csv() == text


def test_table_csv_bytes():
    names = CW.column_names()
    rng = np.random.default_rng(0)
    rows = [CW.row_values(rng.integers(0, 5, (100, 4)), CW.tag_of('/e/%d/x' % i, i)) for i in range(3)]
    text = CW.table_csv(names, rows)
    lines = text.split('\n')
    assert lines[0] == ',' + ','.join(names) and lines[-1] == '' and len(lines) == 5
    assert lines[1].startswith('0,') and lines[3].startswith('2,') and lines[2].endswith(',"path:/e/1/x,sliceID:1"')
    assert CW.table_csv(names, []) == '""\n'
    small = CW.table_csv(['a', 'tag'], [[1, 'p,1'], [2, 'q']])
    assert small == ',a,tag\n0,1,"p,1"\n1,2,q\n'
    pd = pytest.importorskip('pandas')
    series = [pd.Series(dict(zip(names[:-1], np.array(r[:-1], np.int32)), tag=r[-1])) for r in rows]
    assert pd.DataFrame(series).to_csv() == text
    assert pd.DataFrame([]).to_csv() == '""\n'
    assert pd.DataFrame([pd.Series(dict(a=np.int32(1), tag='p,1')), pd.Series(dict(a=np.int32(2), tag='q'))]).to_csv() == small


def test_export_paths():
    root = '/out/val'
    tag = CW.tag_of('/data/exams/p1/e2/s3', 4)
    assert CW.image_path(root, tag, 12) == '/out/val/images/p1/e2/s3/04/step_00000012.png'
    assert CW.csv_path(root, tag, 12) == '/out/val/csv/p1/e2/s3/04/step_00000012_metrics.csv'
    assert CW.image_path(root, CW.tag_of('e2/s3', 123), 0) == '/out/val/images/e2/s3/123/step_00000000.png'
    assert CW.image_path(root, CW.tag_of('s3', 0), 5) == '/out/val/images/s3/00/step_00000005.png'
    assert CW.csv_path(root, CW.tag_of('a,b/c', 1), 99999999) == '/out/val/csv/a,b/c/01/step_99999999_metrics.csv'
    with pytest.raises(ValueError):
        CW.export_dir(root, 'csv', 'no tag')


def decode_png(blob):
    """test-side PNG reader: 8-bit grey / RGB, filter 0 rows (what casewise.encode_png writes), every CRC checked"""
    assert blob[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(blob):
        n, = struct.unpack('>I', blob[pos:pos + 4])
        kind, body = blob[pos + 4:pos + 8], blob[pos + 8:pos + 8 + n]
        crc, = struct.unpack('>I', blob[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        pos += 12 + n
    kinds = [k for k, _ in chunks]
    assert kinds[0] == b'IHDR' and kinds[-1] == b'IEND' and kinds.count(b'IDAT') == 1
    w, h, depth, ctype, _, _, _ = struct.unpack('>IIBBBBB', chunks[0][1])
    assert depth == 8 and ctype in (0, 2)
    c = 1 if ctype == 0 else 3
    raw = np.frombuffer(zlib.decompress(dict(chunks)[b'IDAT']), np.uint8).reshape(h, 1 + w * c)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, c)


@pytest.mark.parametrize('shape', [(7, 13), (7, 13, 1), (32, 48, 3), (1, 1, 3)])
def test_png_round_trip(shape):
    img = np.random.default_rng(len(shape)).integers(0, 256, shape, dtype=np.uint8)
    blob = CW.encode_png(img)
    want = img if img.ndim == 3 else img[..., None]
    assert np.array_equal(decode_png(blob), want)
    try:
        from PIL import Image
    except ImportError:
        return
    import io
    im = Image.open(io.BytesIO(blob))
    assert im.mode == ('L' if want.shape[2] == 1 else 'RGB')
    got = np.asarray(im)
    assert np.array_equal(got.reshape(want.shape), want)


def test_writer_writes_files(tmp_path):
    w = CW.Writer()
    img = np.arange(12, dtype=np.uint8).reshape(3, 4)
    for i in range(40):
        w.submit(str(tmp_path / 'a' / str(i) / 'x.png'), CW.encode_png, img)
    w.submit(str(tmp_path / 'b' / 'm.csv'), CW.series_csv, ['a', 'tag'], [1, 't,1'])
    w.close()
    assert np.array_equal(decode_png((tmp_path / 'a' / '39' / 'x.png').read_bytes())[..., 0], img)
    assert (tmp_path / 'b' / 'm.csv').read_text() == ',a,tag\n0,1,"t,1"\n'
    assert CW.MAX_WORKERS <= 16 and w.pool._max_workers <= 16


def write_exams(tmp_path, h=40, w=36):
    """two exam records (3 and 2 slices) in one file and one in another, with distinct paths"""
    rng = np.random.default_rng(5)
    types = ['TRA', 'ADC', 'label']
    files, expect = [], []
    for f, exams in enumerate([[('/root/p1/e1/s', 3), ('/root/p2/e7/s', 2)], [('/other/p3/e9/s', 4)]]):
        payloads = []
        for path, n in exams:
            sl = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
            sl[..., 2] = (sl[..., 2] > 128) * 255
            payloads.append(T.make_example(sl, f, len(payloads), path, 'cancer', types))
            expect += [(path, k) for k in range(n)]
        p = str(tmp_path / ('exams%d.tfrecords' % f))
        T.write_records(p, payloads)
        files.append(p)
    return files, types, expect


@pytest.mark.parametrize('batch', [4, 9])
def test_tfrecord_meta(tmp_path, batch):
    files, types, expect = write_exams(tmp_path)
    kw = dict(output_size=(32, 32))
    plain = list(T.TFRecordDataset(files, types, batch, **kw))
    meta = list(T.TFRecordDataset(files, types, batch, include_meta=True, **kw))
    assert len(plain) == len(meta) == -(-len(expect) // batch)
    got = []
    for (x, y), (xm, ym, paths, ids) in zip(plain, meta):
        assert np.array_equal(x, xm) and np.array_equal(y, ym) and x.dtype == xm.dtype == np.float32
        assert len(paths) == len(ids) == len(x)
        got += list(zip(paths, [int(k) for k in ids]))
    assert got == expect
    # the device-converted evaluation path (uint8 to the device) gives the same floats
    conv = list(T.TFRecordDataset(files, types, batch, device_convert=True, **kw))
    from dnncancerannotator_amd import augment
    for rb, (xm, ym, _, _) in zip(conv, meta):
        x, y = augment.raw_to_float(rb)
        assert np.array_equal(x, xm) and np.array_equal(y, ym)
    with pytest.raises(ValueError):
        T.TFRecordDataset(files, types, batch, include_meta=True, augment_options=None)


def test_make_dataset_meta(tmp_path, monkeypatch):
    from dnncancerannotator_amd.runs.train import make_dataset
    files, types, expect = write_exams(tmp_path)
    opts = dict(batch_size=4, output_size=[32, 32], slice_types=types)
    ds = make_dataset(files, opts, training=False, include_meta=True)
    assert not ds.pre_sharded and not ds.device_convert
    el = list(ds)
    assert [(p, int(k)) for b in el for p, k in zip(b[2], b[3])] == expect
    syn = list(make_dataset(['synthetic:16x16'], dict(batch_size=3), training=False, include_meta=True))
    ref = list(make_dataset(['synthetic:16x16'], dict(batch_size=3), training=False))
    assert len(syn) == len(ref)
    ids = []
    for (x, y, paths, k), (xr, yr) in zip(syn, ref):
        assert np.array_equal(x, xr) and np.array_equal(y, yr) and paths == ['synthetic:16x16'] * len(x)
        ids += list(k)
    assert ids == list(range(len(ids)))
    z = str(tmp_path / 'a.npz')
    np.savez(z, x=np.zeros((5, 8, 8, 1), np.float32), y=np.zeros((5, 8, 8), np.float32))
    npz = list(make_dataset([z], dict(batch_size=2), training=False, include_meta=True))
    assert [list(b[3]) for b in npz] == [[0, 1], [2, 3], [4]] and npz[0][2] == [z, z]
    with pytest.raises(ValueError):
        make_dataset([z], dict(batch_size=2), training=True, include_meta=True)


def test_array_dataset_without_meta_unchanged():
    ds = data.ArrayDataset(np.zeros((3, 4, 4, 1)), np.zeros((3, 4, 4)), 2)
    assert [len(b) for b in ds] == [2, 2]


# ---- the records of a matched call, the exam grouping and the slice chain (shared by evaluate's passes and predict) -------------
def _matched_tuple():
    """what lesion_table_matched returns for two slices: slice 0 has two predicted lesions and one labelled, slice 1 has none"""
    from dnncancerannotator_amd import _lib
    rows = np.zeros(2, _lib.LESION_ROW_DTYPE)
    rows['row'], rows['area'] = [0, 1], [5, 7]
    true_rows = np.zeros(1, _lib.LESION_ROW_DTYPE)
    true_rows['area'] = 9
    links = np.array([(0, 3, 1, 4)], _lib.LESION_LINK_DTYPE)                 # lesion 1 of slice 0 continues row 3 of the slice before
    true_links = np.array([(0, 2, 0, 6)], _lib.LESION_LINK_DTYPE)
    pairs = np.array([(0, 0, 0, 2), (0, 0, 1, 3)], _lib.LESION_PAIR_DTYPE)
    return (rows, np.array([2, 0], np.int32), np.zeros((2, 0, 0), np.uint8), links, true_rows, np.array([1, 0], np.int32),
            true_links, pairs)


def test_slice_records_of_a_matched_call():
    out = _matched_tuple()
    first, second = CW.slice_records(out, [('exam/a', np.int64(4)), ('exam/a', np.int64(5))])
    assert (first.exam, first.slice, second.exam, second.slice) == ('exam/a', 4, 'exam/a', 5) and type(first.slice) is int
    assert first.rows.tolist() == out[0].tolist() and first.total == 2 and first.links == [(3, 1, 4)]
    assert first.true_rows.tolist() == out[4].tolist() and first.true_total == 1 and first.true_links == [(2, 0, 6)]
    assert first.pairs == [(0, 0, 2), (0, 1, 3)]
    assert len(second.rows) == 0 and second.total == 0 and second.links == [] and len(second.true_rows) == 0
    assert second.true_total == 0 and second.true_links == [] and second.pairs == []
    # the four values of lesion_table_linked: one plane, the labelled fields stay None
    linked = CW.slice_records(out[:4], [('exam/a', 4), ('exam/a', 5)])
    assert (linked[0].exam, linked[0].slice, linked[0].total, linked[0].links) == ('exam/a', 4, 2, [(3, 1, 4)])
    assert linked[0].rows.tolist() == out[0].tolist() and linked[0][5:] == (None,) * 4 and linked[1].links == []
    assert CW.triples(out[7], 'row_true') == [(0, 0, 2), (0, 1, 3)] and all(type(v) is int for t in first.pairs for v in t)


def test_by_exam_keeps_the_order_of_the_data_set():
    recs = [('b', 0), ('a', 0), ('b', 1), ('c', 7), ('a', 1)]                # the slices of b and a come interleaved
    exams = CW.by_exam(recs)
    assert list(exams) == ['b', 'a', 'c']
    assert exams == {'b': [('b', 0), ('b', 1)], 'a': [('a', 0), ('a', 1)], 'c': [('c', 7)]}
    assert CW.by_exam([]) == {}
    named = CW.slice_records(_matched_tuple(), [('x', 1), ('y', 1)])
    assert CW.by_exam(named) == {'x': [named[0]], 'y': [named[1]]}


def test_match_records_links_both_planes_and_calls_the_matcher():
    recs = CW.slice_records(_matched_tuple(), [('e', 4), ('e', 5)])
    recs = [recs[0]._replace(links=[], true_links=[]), recs[1]]              # the exam's first slice continues nothing
    seen = []
    got = CW.match_records(lambda *a, **k: seen.append((a, k)) or 'result', 'e', recs, 2, iou=0.25)
    (exam, true_slices, pred_slices, true_linked, pred_linked, pairs), kw = seen[0]
    assert got == 'result' and exam == 'e' and kw == dict(iou=0.25)
    assert [(s[0], len(s[1]), s[2]) for s in pred_slices] == [(4, 2, 2), (5, 0, 0)]
    assert [(s[0], len(s[1]), s[2]) for s in true_slices] == [(4, 1, 1), (5, 0, 0)]
    assert pred_linked == CW.link_lesions('e', pred_slices, [[], []], min_overlap=2) == CW.link_records('e', recs, 2)
    assert true_linked == CW.link_lesions('e', true_slices, [[], []], min_overlap=2)
    assert pairs == [[(0, 0, 2), (0, 1, 3)], []]
    assert CW.match_records(CW.match_exam_lesions, 'e', recs)[0] == ['e', 1, 2, 0, 1, 0, 2, 0]


def test_slice_chain(caplog):
    from dnncancerannotator_amd.engine import _SliceChain
    chain, dm = _SliceChain('evaluate'), object()
    # the first slice of a run continues nothing; the same exam and the next number continues; a gap and another exam do not
    assert chain.continues(dm, [('a', 3), ('a', 4), ('a', 6), ('b', 7), ('b', np.int64(8))]) == [False, True, False, False, True]
    # the first slice of a second batch continues the last of the first
    assert chain.continues(dm, [('b', '9'), ('b', 9)]) == [True, False]
    assert not caplog.records
    # a re-sized model: a warning, and the chain breaks
    with caplog.at_level('WARNING'):
        assert chain.continues(object(), [('b', 10), ('b', 11)]) == [False, True]
    assert [r.getMessage() for r in caplog.records] == [
        'evaluate: the model was re-sized before slice 10 of b: it is not linked to the slice before']
    caplog.clear()
    other = _SliceChain('predict')
    first = object()
    other.continues(first, [('c', 0)])
    with caplog.at_level('WARNING'):
        assert other.continues(object(), [('c', 1)]) == [False]
    assert caplog.records[0].getMessage().startswith('predict: the model was re-sized before slice 1 of c')
