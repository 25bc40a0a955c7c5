"""-m gpu, runs last: every launch of the three single-GPU BASELINE configurations at their full sizes has met the oracle.

The full-size tests compare tuned kernels with other kernels of this library (generic vs tuned, fused vs per-layer, bf16 vs fp32);
that is parity with the oracle only if every kernel those plans launch is ALSO one that some oracle-compared test ran: the golden
fixtures (tests/test_parity_gpu.py), the float64-oracle tests of tests/test_engine_gpu.py (3-channel level, block-fused backward,
non-square LeakyReLU / L2, label smoothing, dense configurations at real widths), the bf16-emulating oracle.  Those tests register
their models' launch names (helpers.record_oracle_plan); here the three BASELINE plans are built and every name must be in that set.
The inference passes (eval_step, forward(training=False)) have a set of their own, closed by the second test below.
A launch name carries the kernel variant -- the pixel-group / fused kernels in the name itself (shape, ride-alongs), the dense
implicit-GEMM kernels as `name#variant` (channel tile, wave count, operand storage; DeviceModel.plan(variants=True)) -- so a
kernel that only a full-size shape selects shows up as a missing name."""

import pytest

import helpers as Hp

pytestmark = pytest.mark.gpu

REQUIRED = {'test_golden_tuned_kernels', 'test_vector_alu_kernels_of_the_3_channel_level_against_oracle',
            'test_block_fused_backward_against_oracle', 'test_bf16_kernels_against_bf16_emulating_oracle',
            'test_dense_configs_at_real_widths_against_oracle', 'test_fp32_eight_wave_conv_kernels_against_oracle'}
BASELINE = [
    ('configs/unet.yaml', 'unet', 1, 8, 'f32', dict(n_filters_first=3, n_downsample=3, bn=False)),
    ('configs/unet_big.yaml', 'unet', 1, 4, 'bf16', dict(n_filters_first=64, n_downsample=4, bn=True)),
    ('configs/mulmo_unet.yaml', 'mulmo', 3, 8, 'f32', dict(n_filters_first=16, n_downsample=4, bn=True)),
]
# bookkeeping launches without arithmetic of their own that only the dry plan shows (the live step folds them into neighbours)
BOOKKEEPING = {'g_step_init', 'g_finalize_scalars'}
# the inference passes: the tests that compare inference output with the oracle and register that pass's plan
REQUIRED_EVAL = {'test_golden_tuned_kernels', 'test_dense_configs_at_real_widths_against_oracle',
                 'test_bf16_kernels_against_bf16_emulating_oracle', 'test_baseline_inference_at_full_size_against_oracle',
                 'test_inference_of_the_3_channel_level_against_oracle', 'test_ragged_batches_against_oracle',
                 'test_inference_between_train_steps_against_oracle'}
# inference launches without arithmetic: g_step_init zeroes the step's scalars
BOOKKEEPING_EVAL = {'g_step_init'}


def test_every_kernel_of_the_baseline_plans_has_met_the_oracle(gpu):
    missing_tests = REQUIRED - Hp.ORACLE_TESTS
    if missing_tests:
        pytest.skip('partial run: the oracle tests %s did not run in this session' % sorted(missing_tests))
    gaps = {}
    for name, arch, C, B, dtype, opts in BASELINE:
        m = gpu.DeviceModel(arch, C, 512, 512, B, rate=2, kernel_size=3, conv_stride=1, padding='same', dtype=dtype, **opts)
        plan = set(r[0] for r in m.plan(variants=True))
        m.close()
        assert len(plan) >= 10, plan
        print(name, len(plan), 'distinct launches:', ' '.join(sorted(plan)))
        gap = sorted(plan - Hp.ORACLE_KERNELS - BOOKKEEPING)
        if gap:
            gaps[name] = gap
    print('kernel coverage: %d launch names registered by %d oracle tests; BASELINE plans closed' % (len(Hp.ORACLE_KERNELS), len(Hp.ORACLE_TESTS)))
    assert not gaps, 'launches of the BASELINE plans that no oracle-compared test ran: %s' % gaps


def test_every_inference_kernel_of_the_baseline_plans_has_met_the_oracle(gpu, request):
    """The same loop for the inference passes: eval_step and forward(training=False) of the three BASELINE configurations at
    B = max_batch and B = 1 launch only what some test has run in INFERENCE mode and compared with the oracle
    (helpers.ORACLE_EVAL_KERNELS: a set of its own -- in a train step the same kernel reads the batch statistics and takes other
    arms).  g_finalize_scalars, g_bn_finalize, g_head_fwd, g_loss and g_sigmoid compute what is reported: they are not bookkeeping."""
    missing_tests = REQUIRED_EVAL - Hp.ORACLE_EVAL_TESTS
    selected = set(getattr(item, 'originalname', None) or item.name.split('[')[0] for item in request.session.items)
    # a required test that was part of this session and has registered nothing lost its registration (or failed before it)
    assert not (missing_tests & selected), 'oracle tests that ran without registering an inference plan: %s' % sorted(missing_tests & selected)
    if missing_tests:
        pytest.skip('partial run: the inference oracle tests %s did not run in this session' % sorted(missing_tests))
    gaps = {}
    for name, arch, C, B, dtype, opts in BASELINE:
        m = gpu.DeviceModel(arch, C, 512, 512, B, rate=2, kernel_size=3, conv_stride=1, padding='same', dtype=dtype, **opts)
        for batch in (B, 1):
            for mode in ('eval', 'forward'):
                plan = set(r[0] for r in m.plan(variants=True, mode=mode, batch=batch))
                assert len(plan) >= 5, plan
                print(name, mode, 'B', batch, len(plan), 'distinct launches:', ' '.join(sorted(plan)))
                gap = sorted(plan - Hp.ORACLE_EVAL_KERNELS - BOOKKEEPING_EVAL)
                if gap:
                    gaps['%s %s B=%d' % (name, mode, batch)] = gap
        m.close()
    print('inference kernel coverage: %d launch names registered by %d oracle tests; BASELINE inference plans closed' % (
        len(Hp.ORACLE_EVAL_KERNELS), len(Hp.ORACLE_EVAL_TESTS)))
    assert not gaps, 'inference launches of the BASELINE plans that no oracle-compared test ran: %s' % gaps
