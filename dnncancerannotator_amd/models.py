"""Model registry -- annotator/models/tf_models/__init__.py:1-2.  engine.py:267-268 resolves the YAML `model:` name with
getattr(tf_models, name)(**model_options); the classes here take the same keyword arguments (unet.py:195-207) and are
materialised on the GPU by `.build(input_shape, max_batch)` (engine.py:93 model.build(element_spec.shape))."""

from . import device


def _solve_activation(identifier):
    """components.py:323-335: 'relu' or {'class_name': 'LeakyReLU', 'config': {'alpha': a}} -> leaky slope (0 = relu)."""
    if isinstance(identifier, str):
        if identifier != 'relu':
            raise ValueError(f'Failed to resolve activation: {identifier} (supported: relu, LeakyReLU)')
        return 0.0
    if isinstance(identifier, dict):
        if identifier.get('class_name') != 'LeakyReLU':
            raise ValueError(f'Failed to resolve activation: {identifier}')
        return float(identifier.get('config', {}).get('alpha', 0.3))
    raise ValueError(f'Failed to resolve activation: {identifier}')


def _solve_regularizer(spec):
    """configs/additionals/kernel_regularizer.yaml:1-4 -> l2 factor."""
    if spec is None:
        return 0.0
    if isinstance(spec, dict) and spec.get('class_name') in ('L2', 'l2'):
        return float(spec.get('config', {}).get('l2', 0.01))
    raise ValueError(f'unsupported kernel_regularizer: {spec}')


class UNetAnnotator:
    """models/tf_models/unet.py:194-282."""
    arch = 'unet'

    def __init__(self, n_filters_first, n_downsample, rate, kernel_size, conv_stride, bn=False, padding='valid',
                 activation='relu', kernel_regularizer=None, **kargs):
        self.configs = dict(n_filters_first=n_filters_first, n_downsample=n_downsample, rate=rate, kernel_size=kernel_size,
                            conv_stride=conv_stride, bn=bn, padding=padding, activation=activation,
                            kernel_regularizer=kernel_regularizer, **kargs)
        self.reference_index = kargs.get('reference_index', 0)
        self.dtype = kargs.get('dtype', 'f32')
        self.device_model = None

    def get_config(self):
        return self.configs

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def build(self, input_shape, max_batch=None, seed=None, force_generic=False):
        """input_shape = [B or None, H, W, C] (engine.py:93).  Allocates weights/activations in HBM, glorot-initialises."""
        b, h, w, c = input_shape
        c_ = self.configs
        self.device_model = device.DeviceModel(
            self.arch, c, h, w, max_batch or b or 1, c_['n_filters_first'], c_['n_downsample'], rate=c_['rate'],
            kernel_size=c_['kernel_size'], conv_stride=c_['conv_stride'], bn=c_['bn'], padding=c_['padding'],
            leaky_alpha=_solve_activation(c_['activation']), l2=_solve_regularizer(c_['kernel_regularizer']),
            reference_index=self.reference_index, dtype=self.dtype, force_generic=force_generic)
        self.device_model.init_glorot(seed)
        return self.device_model


class MulmoUNetAnnotator(UNetAnnotator):
    """models/tf_models/unet.py:285-300: one encoder per input channel, decoder fed by encoder[reference_index]."""
    arch = 'mulmo'


def _unsupported(name, why):
    class _Unsupported:
        def __init__(self, *a, **k):
            raise NotImplementedError(f'{name}: {why}')
    _Unsupported.__name__ = name
    return _Unsupported


# names exported by the reference that are outside the accelerated hot path
UNet = _unsupported('UNet', 'bare backbone without the annotator head is not a trainable model in the reference configs')
MulmoUNet = _unsupported('MulmoUNet', 'bare backbone without the annotator head is not a trainable model in the reference configs')


def multires_widths(n_filters_first=32, levels=5):
    """[(c1, c2, c3)] of the MultiRes blocks at U = n_filters_first, 2 U, ...: multiresunet.py MultiResBlock, W = 1.67 U and
    int(W * 0.167), int(W * 0.333), int(W * 0.5) in double, as the reference's Python evaluates them."""
    out = []
    for level in range(levels):
        w = 1.67 * (n_filters_first << level)
        out.append((int(w * 0.167), int(w * 0.333), int(w * 0.5)))
    return out


class MultiResUnet:
    """models/tf_models/multiresunet.py MultiResUnet(height, width, n_channels) (configs/multiresunet.yaml): five MultiRes blocks
    with ResPaths on the four skips, a fixed graph without further options.  height / width may be None (taken from the data).
    Private extensions, in kargs: n_filters_first (32: the U of the first block, doubled per level) and dtype (f32 only)."""
    arch = 'multires'
    supports_sensitivity = False         # the input-gradient pass of evaluate knows the U-Net op types only

    def __init__(self, height=None, width=None, n_channels=None, **kargs):
        if n_channels is None:
            # (models.MultiResUnet() without options keeps raising what it raised before this model was supported)
            raise NotImplementedError('MultiResUnet: n_channels must be given (configs/multiresunet.yaml: n_channels: 5)')
        unknown = sorted(set(kargs) - {'n_filters_first', 'dtype'})
        if unknown:
            raise ValueError('MultiResUnet has no option %s (height, width, n_channels; the graph is fixed)' % ', '.join(unknown))
        self.configs = dict(height=height, width=width, n_channels=n_channels, **kargs)
        self.n_filters_first = int(kargs.get('n_filters_first', 32))
        self.dtype = kargs.get('dtype', 'f32')
        if self.dtype != 'f32':
            raise ValueError('MultiResUnet: dtype %s is not supported (f32 only; bf16 is not implemented for this model)' % self.dtype)
        if self.n_filters_first < 1 or any(min(w) < 1 for w in multires_widths(self.n_filters_first)):
            raise ValueError('MultiResUnet: n_filters_first=%d gives a conv without channels (block widths %s)'
                             % (self.n_filters_first, multires_widths(max(self.n_filters_first, 0))))
        self.device_model = None

    def get_config(self):
        return self.configs

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def build(self, input_shape, max_batch=None, seed=None, force_generic=False):
        """input_shape = [B or None, H, W, C]; H and W come from the data (multiples of 16: four 2x2 poolings)."""
        b, h, w, c = input_shape
        c_ = self.configs
        for name, want, have in (('height', c_['height'], h), ('width', c_['width'], w), ('n_channels', c_['n_channels'], c)):
            if want is not None and int(want) != int(have):
                raise ValueError('MultiResUnet: model_options.%s is %s but the data has %s' % (name, want, have))
        if h % 16 or w % 16:
            raise ValueError('MultiResUnet: H, W (%d, %d) must be multiples of 16' % (h, w))
        self.device_model = device.DeviceModel(self.arch, c, h, w, max_batch or b or 1, self.n_filters_first, 4, bn=True, padding='same',
                                               dtype=self.dtype)
        self.device_model.init_glorot(seed)
        return self.device_model
