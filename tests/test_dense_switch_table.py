"""The dense path reads its environment in one place: dense_switches() (csrc/kernels_igemm.hip).  In the two dense source files no other
code may read a DNNCA_ variable, apart from the four that are deliberately read later because tests flip them in-process, and every name
the table reads is listed in DESIGN section 8.

The small-channel step does the same per model: step_switches() (csrc/model.hip) fills StepSwitches, Model::build() stores it, and
no other code of the step's source files reads a DNNCA_ variable."""

import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'dnncancerannotator_amd', 'csrc')
READ_LATER = {'DNNCA_NO_HALF', 'DNNCA_NO_HALF_Z', 'DNNCA_NO_HALF_DY', 'DNNCA_FOLD_BATCH'}
# (the build-time macro DNNCA_TUNING is no environment variable)
NAME = re.compile(r'"(DNNCA_[A-Z0-9_]+)"')


def _code(name):
    """the file without its comments"""
    text = open(os.path.join(CSRC, name)).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return re.sub(r'//[^\n]*', '', text)


def _split_table(code, head='const DenseSwitches& dense_switches() {'):
    """(body of the function that starts with `head`, everything else)"""
    start = code.find(head)
    if start < 0:
        return '', code
    depth, i = 0, code.index('{', start)
    for j in range(i, len(code)):
        depth += {'{': 1, '}': -1}.get(code[j], 0)
        if depth == 0:
            return code[i:j + 1], code[:start] + code[j + 1:]
    raise AssertionError('unbalanced braces in ' + head)


def test_dense_environment_is_read_in_one_table_and_documented():
    table_names = set()
    for name in ('kernels_igemm.hip', 'kernels_ig3x.hip'):
        table, rest = _split_table(_code(name))
        table_names |= set(NAME.findall(table))
        # outside the table: only the named exceptions, each read directly
        stray = set(NAME.findall(rest)) - READ_LATER
        assert not stray, '%s reads %s outside dense_switches()' % (name, sorted(stray))
        for m in re.finditer(r'getenv\s*\(([^)]*)\)', rest):
            assert m.group(1).strip().strip('"') in READ_LATER, '%s: getenv(%s) outside dense_switches()' % (name, m.group(1))
    assert len(table_names) >= 20, 'dense_switches() not found or nearly empty: %s' % sorted(table_names)
    # the dense-path reads of kernels_misc.hip live in the table too
    misc = set(NAME.findall(_code('kernels_misc.hip')))
    assert not misc & {'DNNCA_BN_BLOCKS', 'DNNCA_POOL_BLOCKS', 'DNNCA_NO_POOL_BN_BWD'}, sorted(misc)
    assert {'DNNCA_BN_BLOCKS', 'DNNCA_POOL_BLOCKS', 'DNNCA_NO_POOL_BN_BWD'} <= table_names
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('## 8. Switches'):design.index('## 9.')]
    documented = set(re.findall(r'`(DNNCA_[A-Z0-9_]+)', section))
    documented |= {'DNNCA' + s for s in re.findall(r'`(_[A-Z0-9_]+)', section)}          # the section abbreviates `_NO_X3`
    missing = (table_names | READ_LATER) - documented
    assert not missing, 'not in DESIGN section 8: %s' % sorted(missing)


STEP_FILES = ('model.hip', 'abi_analysis.hip', 'kernels_mfma.hip', 'kernels_fused.hip', 'kernels_fused_bwd.hip', 'kernels_first.hip',
              'kernels_misc.hip', 'kernels_generic.hip', 'kernels_region.hip', 'kernels_sens.hip')


def test_step_environment_is_read_once_per_model_and_documented():
    reader_names = set()
    for name in STEP_FILES:
        reader, rest = _split_table(_code(name), 'StepSwitches step_switches() {')
        assert bool(reader) == (name == 'model.hip'), name
        reader_names |= set(NAME.findall(reader))
        assert 'getenv' not in rest, '%s calls getenv outside step_switches()' % name
        assert not NAME.findall(rest), '%s names %s outside step_switches()' % (name, sorted(set(NAME.findall(rest))))
    assert len(reader_names) >= 30, 'step_switches() not found or nearly empty: %s' % sorted(reader_names)
    # the table is read in exactly one place: the top of Model::build()
    calls = [n for n in STEP_FILES + ('kernels_igemm.hip', 'kernels_ig3x.hip', 'kernels_aug.hip') if re.search(r'\bstep_switches\s*\(\)\s*;', _code(n))]
    assert calls == ['model.hip'] and len(re.findall(r'=\s*step_switches\s*\(\)\s*;', _code('model.hip'))) == 1, calls
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    section = design[design.index('## 8. Switches'):design.index('## 9.')]
    documented = set(re.findall(r'`(DNNCA_[A-Z0-9_]+)', section))
    documented |= {'DNNCA' + s for s in re.findall(r'`(_[A-Z0-9_]+)', section)}
    missing = reader_names - documented
    assert not missing, 'not in DESIGN section 8: %s' % sorted(missing)
