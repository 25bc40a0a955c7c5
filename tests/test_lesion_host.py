"""CPU: the host side of `annotator predict` -- the numpy oracle of the lesion table against hand-counted drawings (and its float32
and float64 statements of the resize against each other on every drawn case the GPU tests use), the CSV bytes and their
arithmetic, the command-line parser, the label-free data sets, and TFKerasModel.annotate on a fake device that serves the
oracle's tables."""

import csv
import io
import os

import numpy as np
import pytest

import lesion_cases as LC
import lesion_oracle as LO
from dnncancerannotator_amd import casewise as CW
from dnncancerannotator_amd import tfrecord as T
from dnncancerannotator_amd.__main__ import build_parser
from dnncancerannotator_amd.runs.train import make_dataset
from test_casewise_host import decode_png


def table(name, **kw):
    prob, spec = LC.ALL[name]()
    return LO.lesion_table(prob, spec['threshold'], spec['rf'], spec['k'], **kw)


# ---- the oracle against hand counts -------------------------------------------------------------------------------------------
def test_oracle_tile_borders_by_hand():
    rows, totals, mask = table('tile_borders')
    assert totals.tolist() == [3, 3] and len(rows) == 6
    a, b = rows[:3], rows[3:]
    assert a['slice'].tolist() == [0, 0, 0] and b['slice'].tolist() == [1, 1, 1] and a['row'].tolist() == [0, 1, 2]
    for f in LO.ROW_DTYPE.names[2:]:
        assert a[f].tolist() == b[f].tolist(), f                    # the same drawing under another slice number
    assert a['area'].tolist() == [1, 66 + 40 + 65, 81]
    assert [tuple(r[f] for f in ('x0', 'y0', 'x1', 'y1')) for r in a] == [(0, 0, 0, 0), (5, 10, 70, 50), (36, 36, 44, 44)]
    assert int(a['sum_x'][2]) == 9 * sum(range(36, 45)) and int(a['sum_y'][2]) == 9 * sum(range(36, 45))
    prob = LC.tile_borders()[0]
    assert float(a['max_prob'][0]) == float(prob[0, 0, 0]) and int(a['sum_prob_q24'][0]) == int(round(float(prob[0, 0, 0]) * 2 ** 24))
    block = prob[0, 36:45, 36:45].astype(np.float64)
    assert int(a['sum_prob_q24'][2]) == int(round(block.sum() * 2 ** 24)) and float(a['max_prob'][2]) == block.max()
    assert mask.shape == (2, 72, 80) and int((mask == 255).sum()) == 2 * (1 + 171 + 81) and set(np.unique(mask)) == {0, 255}


def test_oracle_opening_borders_and_plateau_by_hand():
    rows, totals, mask = table('odd_graded')
    assert totals.tolist() == [2] and rows['area'].tolist() == [41 * 53 - 29 * 41, 12 * 14]
    assert tuple(rows[0][f] for f in ('x0', 'y0', 'x1', 'y1')) == (0, 0, 52, 40)          # touches all four borders
    assert not mask[0, 10:32, 34:37].any() and not mask[0, 30, 20]                      # thinner than k: gone
    rows, totals, mask = table('odd_plateau')
    assert mask.shape == (1, 20, 26) and totals.tolist() == [2]
    assert tuple(rows[0][f] for f in ('x0', 'y0', 'x1', 'y1')) == (0, 0, 25, 19)
    assert rows['max_prob'].tolist() == [0.5, 0.5] and all(int(r['sum_prob_q24']) == int(r['area']) << 23 for r in rows)
    assert not mask[0, 7:13, 16:19].any()                                                # the 4-pixel bar: 2 resized pixels, opened away


def test_oracle_area_filter_and_truncation_by_hand():
    rows, totals, mask = table('areas', min_area=5)
    assert totals.tolist() == [2] and rows['area'].tolist() == [9, 100] and rows['row'].tolist() == [0, 1]
    assert int((mask == 255).sum()) == 109 and not mask[0, 3, 20] and not mask[0, 20:22, 30:32].any()
    rows, totals, _ = table('areas')
    assert rows['area'].tolist() == [9, 1, 100, 4]
    rows, totals, mask = table('checkerboard', max_lesions=16)
    assert totals.tolist() == [480] and len(rows) == 16 and rows['row'].tolist() == list(range(16))
    assert rows['y0'].tolist() == [0] * 16 and rows['x0'].tolist() == list(range(0, 32, 2))     # raster order
    assert int((mask == 255).sum()) == 480                                                        # the mask is not truncated
    rows, totals, _ = table('checkerboard', max_lesions=512)
    assert len(rows) == 480 and rows['area'].tolist() == [1] * 480
    rows, totals, mask = table('empty_and_full')
    assert totals.tolist() == [0, 1] and len(rows) == 1 and rows[0]['slice'] == 1 and rows[0]['area'] == 40 * 72
    assert tuple(rows[0][f] for f in ('x0', 'y0', 'x1', 'y1')) == (0, 0, 71, 39)
    assert not mask[0].any() and (mask[1] == 255).all()


@pytest.mark.parametrize('name', sorted(LC.ALL))
def test_float32_and_float64_resize_give_the_same_table(name):
    """no drawn case hangs on how a product or a sum of the resize was rounded"""
    prob, spec = LC.ALL[name]()
    assert np.array_equal(np.round(prob * 64), prob * 64)                 # multiples of 1 / 64
    a = LO.lesion_table(prob, spec['threshold'], spec['rf'], spec['k'], max_lesions=512)
    b = LO.lesion_table(prob, spec['threshold'], spec['rf'], spec['k'], max_lesions=512, resize=LO.resize64)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist() and np.array_equal(a[2], b[2])


def test_resized_statistics_differ_from_raw_ones():
    """even_graded_half is the case that tells a lesion_stats reading the raw plane from one reading the resized one"""
    prob, spec = LC.even_graded_half()
    rows, _, _ = LO.lesion_table(prob, **{'threshold': spec['threshold'], 'rf': spec['rf'], 'k': spec['k']})
    assert len(rows) == 2
    r = rows[0]
    raw = prob[0, r['y0']:r['y1'] + 1, r['x0']:r['x1'] + 1]
    assert int(np.rint(raw.astype(np.float64) * 2 ** 24).sum()) != int(r['sum_prob_q24'])


# ---- CSV -----------------------------------------------------------------------------------------------------------------------
def _row(**kw):
    r = np.zeros((), LO.ROW_DTYPE)
    for k, v in kw.items():
        r[k] = v
    return r


def test_lesion_and_slice_csv_bytes_and_arithmetic():
    r = _row(slice=1, row=2, area=4, x0=3, y0=5, x1=4, y1=6, max_prob=0.875, sum_x=14, sum_y=22, sum_prob_q24=3 * (1 << 24))
    v = CW.lesion_values('/data/p1/e2,x', 7, r)
    assert v == ['/data/p1/e2,x', 7, 2, 4, 3, 5, 4, 6, '3.5', '5.5', '0.75', '0.875']
    text = CW.plain_csv(CW.LESION_COLUMNS, [v])
    assert text == ('exam,slice,lesion,area_px,x0,y0,x1,y1,centroid_x,centroid_y,mean_prob,max_prob\n'
                    '"/data/p1/e2,x",7,2,4,3,5,4,6,3.5,5.5,0.75,0.875\n')
    # the float64 quotients read back exactly; max_prob gives its float32 back
    r2 = _row(area=3, sum_x=10, sum_y=11, sum_prob_q24=41234567, max_prob=np.float32(0.7))
    v2 = CW.lesion_values('e', 0, r2)
    assert float(v2[8]) == 10 / 3 and float(v2[9]) == 11 / 3 and float(v2[10]) == 41234567 / 3 / 2 ** 24
    assert np.float32(float(v2[11])) == np.float32(0.7)
    s = CW.slice_values('e', 3, [r, r2], 5)
    assert s == ['e', 3, 5, 7, '0.875', 1]
    assert CW.slice_values('e', 3, [r, r2], 2)[-1] == 0
    assert CW.slice_values('e', 4, [], 0) == ['e', 4, 0, 0, '0', 0]
    assert CW.plain_csv(CW.SLICE_COLUMNS, [s]) == 'exam,slice,n_lesions,lesion_area_px,max_prob,truncated\ne,3,5,7,0.875,1\n'
    assert CW.plain_csv(CW.SLICE_COLUMNS, []) == 'exam,slice,n_lesions,lesion_area_px,max_prob,truncated\n'
    assert CW.mask_path('/out', CW.tag_of('/data/exams/p1/e2/s3', 4)) == '/out/p1/e2/s3/04/mask.png'
    assert CW.mask_path('/out', CW.tag_of('synthetic:64x64x2', 11)) == '/out/synthetic:64x64x2/11/mask.png'


def test_parser_predict():
    p = build_parser()
    a = vars(p.parse_args(['predict', '--save_path', 's', '--data_path', 'a.npz', 'b.npz', '--output', 'o']))
    assert a == dict(command='predict', save_path='s', data_path=['a.npz', 'b.npz'], output='o', config=None, step=None, threshold=0.5,
                     min_area=0, filter_size=5, resize_factor=1.0, max_lesions=256, export_images=False)
    a = vars(p.parse_args(['predict', '--save_path', 's', '--data_path', 'd', '--output', 'o', '--config', 'c1', 'c2', '--step', '40',
                           '--threshold', '0.7', '--min_area', '9', '--filter_size', '3', '--resize_factor', '0.5', '--max_lesions',
                           '8', '--export_images']))
    assert (a['step'], a['threshold'], a['min_area'], a['filter_size'], a['resize_factor'], a['max_lesions'], a['export_images'],
            a['config']) == (40, 0.7, 9, 3, 0.5, 8, True, ['c1', 'c2'])
    with pytest.raises(SystemExit):
        p.parse_args(['predict', '--save_path', 's', '--data_path', 'd'])              # --output is required


# ---- data sets without labels --------------------------------------------------------------------------------------------------
def test_make_dataset_without_labels_npz_and_synthetic(tmp_path):
    x = np.random.default_rng(0).random((5, 8, 8, 2)).astype(np.float32)
    only_x, with_y = str(tmp_path / 'a.npz'), str(tmp_path / 'b.npz')
    np.savez(only_x, x=x)
    np.savez(with_y, x=x, y=np.ones((5, 8, 8), np.float32))
    for path in (only_x, with_y):                                   # a file that carries labels is accepted, they are not read on
        ds = make_dataset([path], dict(batch_size=2), training=False, include_meta=True, labels=False)
        got = list(ds)
        assert [len(el) for el in got] == [3, 3, 3] and [len(el[0]) for el in got] == [2, 2, 1]
        assert np.array_equal(np.concatenate([el[0] for el in got]), x)
        assert got[1][1] == [path, path] and got[2][2].tolist() == [4]
        assert len(ds.element_spec) == 1 and tuple(ds.element_spec[0].shape) == (2, 8, 8, 2)
    with pytest.raises(KeyError):
        make_dataset([only_x], dict(batch_size=2), training=False, include_meta=True)        # labels=True stays the default
    plain = list(make_dataset([only_x], dict(batch_size=4), training=False, labels=False))
    assert [len(el) for el in plain] == [1, 1] and plain[1][0].shape == (1, 8, 8, 2)
    with pytest.raises(ValueError):
        make_dataset([only_x], dict(batch_size=2), training=True, labels=False)
    syn = make_dataset(['synthetic:16x24x2'], dict(batch_size=3), training=False, include_meta=True, labels=False)
    ref = make_dataset(['synthetic:16x24x2'], dict(batch_size=3), training=False, include_meta=True)
    a, b = list(syn), list(ref)
    assert len(a) == len(b) == 2
    for ea, eb in zip(a, b):
        assert len(ea) == 3 and len(eb) == 4 and np.array_equal(ea[0], eb[0]) and ea[1] == eb[2] and ea[2].tolist() == eb[3].tolist()


def _exam(rng, n, h, w, types, path):
    return T.make_example(rng.integers(0, 256, (n, h, w, len(types)), dtype=np.uint8), 1, 2, path, 'c', types)


def test_make_dataset_without_labels_tfrecords(tmp_path):
    """exam files written without a label slice (and one with): slice_types less `label` are read, every channel is a feature"""
    rng = np.random.default_rng(3)
    bare, full = str(tmp_path / 'bare.tfrecords'), str(tmp_path / 'full.tfrecords')
    T.write_records(bare, [_exam(rng, 3, 20, 24, ['TRA', 'ADC'], '/d/p1/e1'), _exam(rng, 2, 20, 24, ['TRA', 'ADC'], '/d/p1/e2')])
    T.write_records(full, [_exam(rng, 2, 20, 24, ['TRA', 'label', 'ADC'], '/d/p2/e1')])
    opts = dict(batch_size=2, slice_types=['TRA', 'ADC', 'label'], output_size=[16, 16])
    ds = make_dataset([bare, full], opts, training=False, include_meta=True, labels=False)
    got = list(ds)
    assert [len(el) for el in got] == [3, 3, 3, 3] and [len(el[0]) for el in got] == [2, 2, 2, 1]
    assert ds.slice_types == ['TRA', 'ADC'] and tuple(ds.element_spec[0].shape) == (2, 16, 16, 2) and len(ds.element_spec) == 1
    assert sum((el[1] for el in got), []) == ['/d/p1/e1'] * 3 + ['/d/p1/e2'] * 2 + ['/d/p2/e1'] * 2
    assert np.concatenate([el[2] for el in got]).tolist() == [0, 1, 2, 0, 1, 0, 1]
    # the features are those the labelled reading of the labelled file gives
    lab = list(make_dataset([full], opts, training=False, include_meta=True))
    assert np.array_equal(np.concatenate([el[0] for el in got])[5:], lab[0][0])
    assert got[0][0].dtype == np.float32 and 0.0 <= got[0][0].min() and got[0][0].max() <= 1.0
    with pytest.raises(Exception):                                  # the bare file has no label slice to give
        list(make_dataset([bare], opts, training=False, include_meta=True))
    with pytest.raises(ValueError):
        T.TFRecordDataset([bare], ['TRA', 'label'], 2, labels=False)


# ---- annotate on a fake device --------------------------------------------------------------------------------------------------
def _fake_engine(monkeypatch, probs_of):
    """the engine on tests/fake_device.FakeDeviceModel with forward(return_prob=False) and lesion_table served by the oracle;
    probs_of(x) -> [B, H, W] are the probabilities the fake forward leaves 'on the device'"""
    from dnncancerannotator_amd import device, engine, models
    from fake_device import FakeDeviceModel

    class Dev(FakeDeviceModel):
        def forward(self, x, training=False, return_logits=False, return_prob=True):
            assert not training and not return_prob
            self._check(x)
            self.calls.append(('forward', len(x)))
            self.prob = probs_of(np.asarray(x))

        def lesion_table(self, batch=None, prob=None, threshold=0.5, resize_factor=1.0, filter_size=5, min_area=0, max_lesions=256,
                         mask=True):
            assert prob is None and batch == len(self.prob)
            self.calls.append(('lesion_table', batch, mask))
            rows, totals, masks = LO.lesion_table(self.prob, threshold, resize_factor, filter_size, min_area, max_lesions)
            return rows, totals, (masks if mask else None)

    def build(self, input_shape, max_batch=None, seed=None, force_generic=False):
        b, h, w, c = input_shape
        c_ = self.configs
        self.device_model = Dev(self.arch, c, h, w, max_batch or b or 1, c_['n_filters_first'], c_['n_downsample'], rate=c_['rate'],
                                kernel_size=c_['kernel_size'], conv_stride=c_['conv_stride'], bn=c_['bn'], padding=c_['padding'])
        return self.device_model
    monkeypatch.setattr(device, 'init_device', lambda ordinal=0: None)
    monkeypatch.setattr(device, 'device_count', lambda: 1)
    monkeypatch.setattr(models.UNetAnnotator, 'build', build)
    cfg = {'model': 'UNetAnnotator',
           'model_options': dict(n_filters_first=2, n_downsample=1, rate=2, kernel_size=3, conv_stride=1, bn=False, padding='same'),
           'deploy_options': {'optimizer': 'adam', 'enable_multigpu': False}}
    return engine.TFKerasModel(cfg)


class _Slices:
    """a label-free data set with meta: batches (x, paths, sliceIDs); the drawn probability rides in channel 0 of x"""

    def __init__(self, prob, batch):
        from dnncancerannotator_amd.data import Spec
        self.prob, self.batch = prob, batch
        self.element_spec = (Spec((batch,) + prob.shape[1:] + (1,), np.float32),)

    def __iter__(self):
        for i in range(0, len(self.prob), self.batch):
            p = self.prob[i:i + self.batch]
            yield p[..., None], ['/data/p%d/exam' % (k // 2) for k in range(i, i + len(p))], np.arange(i, i + len(p)) % 2


def test_annotate_writes_the_oracles_tables(tmp_path, monkeypatch):
    blocks, _ = LC.areas()
    board, _ = LC.checkerboard()
    prob = np.zeros((3, 32, 40), np.float32)
    prob[0], prob[1, :24, :40] = blocks[0], board[0]                 # slice 2 stays empty
    e = _fake_engine(monkeypatch, lambda x: x[..., 0])
    ds = _Slices(prob, 2)
    e._build(ds)
    for step in (3, 7):
        e.current_step = step
        e.save(str(tmp_path / 'run' / 'checkpoints' / ('ckpt-%d' % step)))
    out = str(tmp_path / 'out')
    res = e.annotate(ds, str(tmp_path / 'run'), out, threshold=0.5, filter_size=1, min_area=0, max_lesions=16, export_images=True)
    assert res == dict(step=7, slices=3, lesions=4 + 16)
    assert [c for c in e.device_model.calls if c[0] != 'eval'] == [('forward', 2), ('lesion_table', 2, True), ('forward', 1),
                                                                   ('lesion_table', 1, True)]
    rows, totals, masks = LO.lesion_table(prob, 0.5, 1.0, 1, 0, 16)
    with open(os.path.join(out, 'lesions.csv'), newline='') as f:
        text = f.read()
    exams, ids = ['/data/p0/exam', '/data/p0/exam', '/data/p1/exam'], [0, 1, 0]
    assert text == CW.plain_csv(CW.LESION_COLUMNS, [CW.lesion_values(exams[r['slice']], ids[r['slice']], r) for r in rows])
    table_ = list(csv.DictReader(io.StringIO(text)))
    assert len(table_) == 20 and [int(r['area_px']) for r in table_[:4]] == [9, 1, 100, 4]
    assert [(r['exam'], r['slice'], r['lesion']) for r in table_[:5]] == [('/data/p0/exam', '0', str(i)) for i in range(4)] + [
        ('/data/p0/exam', '1', '0')]
    assert float(table_[0]['centroid_x']) == 4.0 and float(table_[0]['centroid_y']) == 3.0
    assert float(table_[2]['mean_prob']) == float(blocks[0, 8:18, 10:20].astype(np.float64).mean())
    with open(os.path.join(out, 'slices.csv'), newline='') as f:
        srows = list(csv.DictReader(f))
    assert [(r['exam'], r['slice'], r['n_lesions'], r['truncated']) for r in srows] == [
        ('/data/p0/exam', '0', '4', '0'), ('/data/p0/exam', '1', '480', '1'), ('/data/p1/exam', '0', '0', '0')]
    assert [int(r['lesion_area_px']) for r in srows] == [114, 16, 0]
    files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert files == ['data/p0/exam/00/mask.png', 'data/p0/exam/01/mask.png', 'data/p1/exam/00/mask.png', 'lesions.csv', 'slices.csv']
    for b, name in enumerate(files[:3]):
        with open(os.path.join(out, name), 'rb') as f:
            assert np.array_equal(decode_png(f.read())[..., 0], masks[b])
    # an explicit step, no images: no mask is asked of the device and no PNG is written
    out2 = str(tmp_path / 'out2')
    e.device_model.calls.clear()
    assert e.annotate(ds, str(tmp_path / 'run'), out2, step=3, filter_size=1, min_area=5)['lesions'] == 2
    assert ('lesion_table', 2, False) in e.device_model.calls and sorted(os.listdir(out2)) == ['lesions.csv', 'slices.csv']
    with pytest.raises(ValueError):
        e.annotate(ds, str(tmp_path / 'run'), out2, step=5)
    e.ctx = e.ctx._replace(world=2)                               # multi-rank prediction is out of scope: a clear error
    with pytest.raises(RuntimeError, match='single process'):
        e.annotate(ds, str(tmp_path / 'run'), out2)
