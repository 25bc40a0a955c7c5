"""Dumps the dry launch plan (dnnca_plan_dump: name#variant, bytes, flops) of every dense-path model shape, both dtypes, by default and
under every switch of the dense table, one child process per arm -- the table is read once per process.  Two
libraries are compared by running it once per library and diffing the two output directories:

    DNNCA_LIB=<a>/libdnnca.so python tools/dense_plan_matrix.py dump out_a
    DNNCA_LIB=<b>/libdnnca.so python tools/dense_plan_matrix.py dump out_b
    python tools/dense_plan_matrix.py compare out_a out_b

A dry plan launches nothing, so the whole matrix takes a minute or two.

A third argument `step` (`dump out_a step`) takes the matrix of the small-channel step instead: the configs/unet.yaml model at the
shapes that reach its pixel-group, column-strip and block-fused launchers, the train, eval and forward plans at max_batch and at one
image, by default and under every switch of the per-model table (StepSwitches), one child process per arm."""

import filecmp
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL = dict(rate=2, kernel_size=3, conv_stride=1, padding='same', bn=True)
# (name, arch, channels, H, W, batch, options): the BASELINE configurations at full size, then the dense shapes of
# tests/test_engine_gpu.py and tests/test_parity_gpu.py
SHAPES = [
    ('unet_yaml_512_b8', 'unet', 1, 512, 512, 8, dict(FULL, n_filters_first=3, n_downsample=3, bn=False)),
    ('unet_big_512_b4', 'unet', 1, 512, 512, 4, dict(FULL, n_filters_first=64, n_downsample=4)),
    ('mulmo_unet_512_b8', 'mulmo', 3, 512, 512, 8, dict(FULL, n_filters_first=16, n_downsample=4)),
    ('unet_big_512_b1', 'unet', 1, 512, 512, 1, dict(FULL, n_filters_first=64, n_downsample=4)),
    ('unet64x4_64_b1', 'unet', 1, 64, 64, 1, dict(FULL, n_filters_first=64, n_downsample=4)),
    ('unet64x4_64_b2', 'unet', 1, 64, 64, 2, dict(FULL, n_filters_first=64, n_downsample=4)),
    ('mulmo16x4_64_b2', 'mulmo', 3, 64, 64, 2, dict(FULL, n_filters_first=16, n_downsample=4)),
    ('mulmo16x4_128_b2', 'mulmo', 3, 128, 128, 2, dict(FULL, n_filters_first=16, n_downsample=4)),
    ('unet512x1_32_b2', 'unet', 1, 32, 32, 2, dict(FULL, n_filters_first=512, n_downsample=1)),
    ('unet64x2_64_b2', 'unet', 1, 64, 64, 2, dict(FULL, n_filters_first=64, n_downsample=2)),
    ('unet64x2_128_b4', 'unet', 1, 128, 128, 4, dict(FULL, n_filters_first=64, n_downsample=2)),
    ('unet64x1_32_b2', 'unet', 1, 32, 32, 2, dict(FULL, n_filters_first=64, n_downsample=1)),
    ('unet32x2_32x48_b2', 'unet', 1, 32, 48, 2, dict(FULL, n_filters_first=32, n_downsample=2)),
    ('mulmo16x3_40x48_b2', 'mulmo', 3, 40, 48, 2, dict(FULL, n_filters_first=16, n_downsample=3)),
    ('mulmo16x2_40x48_b2', 'mulmo', 3, 40, 48, 2, dict(FULL, n_filters_first=16, n_downsample=2)),
    ('mulmo2c_16x2_32_b2', 'mulmo', 2, 32, 32, 2, dict(FULL, n_filters_first=16, n_downsample=2)),
    ('unet16x1_rate4_32_b2', 'unet', 1, 32, 32, 2, dict(FULL, n_filters_first=16, n_downsample=1, rate=4)),
]
# every switch of the dense table, one arm each (plus the per-model and per-step ones that are read later)
ARMS = [{}] + [{k: '1'} for k in (
    'DNNCA_IGCONV1', 'DNNCA_WGRAD1', 'DNNCA_TCWGRAD1', 'DNNCA_TCONV_FWD1', 'DNNCA_NO_X3', 'DNNCA_NO_X3_WGRAD', 'DNNCA_NO_WG_PLAIN',
    'DNNCA_NO_WG_BUCKETS', 'DNNCA_WGRAD64_NARROW', 'DNNCA_NO_BN_FUSION', 'DNNCA_NO_POOL_STATS', 'DNNCA_NO_NORM_ON_LOAD',
    'DNNCA_NO_BN_BWD_RIDE', 'DNNCA_NO_POOL_BN_BWD', 'DNNCA_X3_NO_SPLIT', 'DNNCA_X3_NO_DB', 'DNNCA_NO_HALF', 'DNNCA_NO_HALF_Z',
    'DNNCA_NO_HALF_DY', 'DNNCA_FOLD_BATCH')] + [
    {'DNNCA_IG_NW': '4'}, {'DNNCA_IG_NW': '8'}, {'DNNCA_IGB_NW': '4'}, {'DNNCA_IGB_NW': '8'}, {'DNNCA_X3_NN': '1'}, {'DNNCA_X3_NN': '2'},
    {'DNNCA_X3_BLOCKS': '1'}, {'DNNCA_BN_BLOCKS': '64'}, {'DNNCA_POOL_BLOCKS': '256'},
    {'DNNCA_NO_X3': '1', 'DNNCA_NO_WG_PLAIN': '1'}, {'DNNCA_NO_X3_WGRAD': '1', 'DNNCA_IG_NW': '8'}]


YAML = dict(FULL, n_filters_first=3, n_downsample=3, bn=False)
# (name, batch, H, W, further DeviceModel options, train_metrics): whole tiles at every level / partial strips, the 12-channel level on
# the generic conv / one chunk / ... / the pool fold declines / the PROB variants of the head launches
STEP_SHAPES = [
    ('yaml_512_b8', 8, 512, 512, {}, False), ('b2_64x256', 2, 64, 256, {}, False), ('b3_24x200', 3, 24, 200, {}, False),
    ('b1_8x64', 1, 8, 64, {}, False), ('b2_40x128', 2, 40, 128, {}, False), ('b5_32x248', 5, 32, 248, {}, False),
    ('b2_64x256_leaky', 2, 64, 256, dict(leaky_alpha=0.3), False), ('b2_64x256_metrics', 2, 64, 256, {}, True),
]
TEN = ('DNNCA_NO_TAIL3', 'DNNCA_NO_FIRST3', 'DNNCA_NO_FIRST3F', 'DNNCA_NO_UP3F', 'DNNCA_NO_TCF', 'DNNCA_NO_FOLD_ADAM', 'DNNCA_NO_PREP_RIDE',
       'DNNCA_NO_TCONV_RIDE', 'DNNCA_NO_TCM', 'DNNCA_NO_FUSED_BWD')      # tests/test_engine_gpu.py: the strip kernels against the per-layer ones
STEP_ARMS = [{}] + [{k: '1'} for k in TEN + (
    'DNNCA_NO_FUSED', 'DNNCA_NO_POOL_FOLD', 'DNNCA_NO_BWD3V', 'DNNCA_NO_VW', 'DNNCA_NO_HEAD_IN_CONV', 'DNNCA_NO_LABEL_FUSION',
    'DNNCA_NO_WG_STREAM', 'DNNCA_FZ_UP2', 'DNNCA_FZ_ALL', 'DNNCA_LOCKSTEP', 'DNNCA_FORCE_RCCL', 'DNNCA_STAMPS_PF', 'DNNCA_DBG', 'DNNCA_FZB_DBG',
    'DNNCA_F3F_ABL', 'DNNCA_ABL', 'DNNCA_TAIL3_VARIANT')] + [
    {'DNNCA_FZ_ONLY': 'down1'}, {'DNNCA_FZ_ONLY': 'up1'}, {'DNNCA_FZB_ONLY': 'down2'}, {'DNNCA_FZB_ONLY': 'up1'}, {'DNNCA_STAMPS': '3,2,3'},
    {'DNNCA_NBLOCKS': '64'}, {'DNNCA_PG_MAXOCC': '2'}, {'DNNCA_TAIL3_SLOTS': '1024'}, {'DNNCA_TAIL3_LDS': '32768'}, {'DNNCA_LOCKSTEP_MAXH': '64'},
    {'DNNCA_WG_PRIO': '2'}, {'DNNCA_BUCKET_BYTES': '262144'},
    {k: '1' for k in TEN}, {'DNNCA_NO_TAIL3': '1', 'DNNCA_NO_FIRST3': '1'}, {'DNNCA_NO_TAIL3': '1', 'DNNCA_NO_HEAD_IN_CONV': '1'}]


def arm_name(arm):
    return '+'.join('%s=%s' % kv for kv in sorted(arm.items())) or 'default'


def child(out_dir, step):
    from dnncancerannotator_amd import device
    device.init_device(0)
    for name, B, H, W, opts, metrics in STEP_SHAPES if step else []:
        m = device.DeviceModel('unet', 1, H, W, B, **YAML, **opts)
        if metrics:
            m.train_metrics([0.25, 0.5, 0.75])
        for mode in ('train', 'eval', 'forward'):
            for batch in sorted({B, 1}):
                with open(os.path.join(out_dir, '%s.%s.b%d.plan' % (name, mode, batch)), 'w') as f:
                    for k, b, fl in m.plan(variants=True, mode=mode, batch=batch):
                        f.write('%s\t%r\t%r\n' % (k, b, fl))
        m.close()
    if step:
        return
    for name, arch, C, H, W, B, opts in SHAPES:
        for dtype in ('f32', 'bf16'):
            m = device.DeviceModel(arch, C, H, W, B, dtype=dtype, **opts)
            with open(os.path.join(out_dir, '%s.%s.plan' % (name, dtype)), 'w') as f:
                for k, b, fl in m.plan(variants=True):
                    f.write('%s\t%r\t%r\n' % (k, b, fl))
            m.close()


def dump(out, step):
    for arm in STEP_ARMS if step else ARMS:
        d = os.path.join(out, arm_name(arm) if len(arm) < 10 else 'TEN')
        os.makedirs(d, exist_ok=True)
        subprocess.run([sys.executable, os.path.abspath(__file__), 'child', d] + ['step'] * step, env=dict(os.environ, **arm), check=True,
                       timeout=300)
        print('dumped', arm_name(arm), flush=True)


def compare(a, b):
    arms, plans, bad, lines = sorted(os.listdir(a)), 0, [], 0
    assert arms == sorted(os.listdir(b)), 'different arms'
    for arm in arms:
        names = sorted(os.listdir(os.path.join(a, arm)))
        assert names == sorted(os.listdir(os.path.join(b, arm))) and names, 'different plans under ' + arm
        for n in names:
            plans += 1
            lines += sum(1 for _ in open(os.path.join(a, arm, n)))
            if not filecmp.cmp(os.path.join(a, arm, n), os.path.join(b, arm, n), shallow=False):
                bad.append(arm + '/' + n)
    print('%d arms x %d plans = %d plan texts, %d launch lines: %d differ %s' % (len(arms), plans // len(arms), plans, lines, len(bad), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    if sys.argv[1] == 'child':
        child(sys.argv[2], sys.argv[3:] == ['step'])
    elif sys.argv[1] == 'dump':
        dump(sys.argv[2], sys.argv[3:] == ['step'])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
