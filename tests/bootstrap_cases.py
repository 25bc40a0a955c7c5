"""The 12-exam detection cases of the bootstrap tests (tests/test_bootstrap_host.py (a), the end-to-end test of
tests/test_bootstrap_gpu.py) and the resample written out: exams without candidates (with and without tumours), exams without
tumours, confidences tied across exams (0.75, 0.5, 0.625, 0.25), exam scores tied between a positive and a negative exam (0.875), and the
top-ranked candidate in an exam that about a third of the replicates leave out.  Test infrastructure only."""

REPLICATES, SEED = 64, 7

CASES = [
    dict(exam='e00', tumours=1, confidences=[0.96875, 0.5], hits=[1, 0]),
    dict(exam='e01', tumours=0, confidences=[0.75], hits=[0]),
    dict(exam='e02', tumours=2, confidences=[0.75, 0.625, 0.25], hits=[1, 1, 0]),
    dict(exam='e03', tumours=0, confidences=[], hits=[]),
    dict(exam='e04', tumours=1, confidences=[], hits=[]),
    dict(exam='e05', tumours=0, confidences=[0.5, 0.375], hits=[0, 0]),
    dict(exam='e06', tumours=1, confidences=[0.875], hits=[1]),
    dict(exam='e07', tumours=0, confidences=[0.875, 0.125], hits=[0, 0]),
    dict(exam='e08', tumours=3, confidences=[0.625, 0.5, 0.4375, 0.25], hits=[1, 0, 1, 0]),
    dict(exam='e09', tumours=0, confidences=[0.25], hits=[0]),
    dict(exam='e10', tumours=1, confidences=[0.3125], hits=[0]),
    dict(exam='e11', tumours=0, confidences=[], hits=[]),
]


def written_out(cases, m):
    """the resample as a list of cases: every exam repeated m[e] times"""
    return [c for c, k in zip(cases, m) for _ in range(int(k))]


def reference_values(cases, m):
    """what the existing functions give on the resample written out: (casewise.detection_curves, casewise.detection_auroc)"""
    from dnncancerannotator_amd import casewise
    drawn = written_out(cases, m)
    return casewise.detection_curves(drawn), casewise.detection_auroc(drawn)


def hold_to_reference(values, row, curves, auroc, levels):
    """detection_replicate_values `values` and the integers of `row` against the existing functions on the resample written out:
    integers equal, sensitivities, cpm and auroc equal as floats, AP within 4 L 2^-53 absolute (detection_curves rounds each recall
    before it subtracts)"""
    assert int(row['tumours']) == curves['tumours'] and int(row['candidates']) == curves['candidates']
    assert (int(row['tp']), int(row['fp'])) == (curves['tp'], curves['fp'])
    ap, au, score, sens, cpm = values[0], values[1], values[2], values[3:10], values[10]
    assert au == auroc and (au is None) == (int(row['auroc_pairs']) == 0)
    if curves['tumours'] == 0:
        assert ap is None and cpm is None and sens == [None] * 7 and score is None and curves['ap'] is None
        return
    assert sens == curves['sensitivities'] and cpm == curves['cpm']
    assert [int(t) for t in row['tp_at']] == [round(s * curves['tumours']) for s in curves['sensitivities']]
    assert abs(ap - curves['ap']) <= 4 * levels * 2.0 ** -53, (ap, curves['ap'])
    assert (score is None) == (auroc is None)
    if score is not None:
        assert score == (ap + au) / 2
