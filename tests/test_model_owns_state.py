"""What belongs to a model lives in Model (two models in one process each keep their own).  Read from the sources,
comments stripped:

* no file under csrc/ keeps a map keyed by a model's address, and the three maps that did (g_plans, g_ig, g_ig3x) are gone: the
  kernel families' plans hang off Model (plan_pg, plan_ig, plan_ig3x);
* what a train step asks of its forward pass is an argument (StepRequest), never written into the model and cleared afterwards:
  `defer_head` and the head-in-conv request are assigned nowhere but in the struct's own definition."""

import os
import re

from test_dense_switch_table import CSRC, _code

SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith(('.hip', '.h', '.cpp')))


def test_no_map_is_keyed_by_a_model_pointer():
    assert len(SOURCES) > 20
    for name in SOURCES:
        code = _code(name)
        keyed = re.findall(r'\b(?:unordered_)?map\s*<\s*(?:const\s+)?(?:dnnca::)?Model\s*(?:const\s*)?\*', code)
        assert not keyed, '%s declares a map keyed by a Model pointer' % name


def test_the_three_plan_maps_are_gone():
    for name in SOURCES:
        found = re.findall(r'\b(g_plans|g_ig|g_ig3x)\b', _code(name))
        assert not found, '%s still names %s' % (name, sorted(set(found)))
    header = _code('model.h')
    for plan in ('PgPlan', 'IgPlan', 'Ig3xPlan'):
        assert re.search(r'\bstruct\s+%s\s*;' % plan, header), '%s is not forward-declared in model.h' % plan
        assert re.search(r'\b%s\s*\*\s*\w+\s*=\s*nullptr\s*;' % plan, header), 'Model holds no %s pointer' % plan


def test_the_train_steps_request_is_never_written_into_the_model():
    assign = re.compile(r'\b(defer_head|head_in_conv\s*\.\s*requested|head_in_conv)\s*=(?!=)')
    header = _code('model.h')
    start = header.index('struct StepRequest {')
    body = header[start:header.index('\n};', start)]
    assert {m.group(1) for m in assign.finditer(body)} == {'defer_head', 'head_in_conv'}       # the defaults of the two fields
    for name in SOURCES:
        code = _code(name)
        if name == 'model.h':
            code = code.replace(body, '')
        found = [m.group(0) for m in assign.finditer(code)]
        assert not found, '%s assigns %s' % (name, found)
    # ... and both callers of a train pass go through one function that builds it
    model = _code('model.hip')
    assert len(re.findall(r'\bStepRequest\s+\w+\s*\{', model)) == 1
    assert len(re.findall(r'\bhead_in_conv_requested\s*\(', model)) == 2          # its definition and that one use
