"""Test-time augmentation (`predict --tta`, `evaluate --tta`): the modes and the view masks they stand for.

A view is a number k = 4 t + 2 v + h in 0..7 (the dihedral group of the square): flip the rows (v) and the columns (h) of a slice,
then (t) transpose it.  A set of views is a bit mask in 1..255, bit k for view k (include/dnnca.h, dnnca_forward_tta): the network
runs on every selected view, each answer is mapped back and the probabilities are averaged on the device."""

NONE = 'none'
MASKS = {'flips': 0x0F,     # identity, left-right, up-down, both: any H, W
         'd4': 0xFF}        # all eight: the transposed views need H == W
MODES = (NONE,) + tuple(MASKS)


def mask_of(mode, height, width):
    """the view mask of `mode` on slices of height x width; None for 'none'.  ValueError: an unknown mode, d4 on a non-square slice"""
    if mode == NONE:
        return None
    if mode not in MASKS:
        raise ValueError('tta: unknown mode %r (one of %s)' % (mode, ', '.join(MODES)))
    if MASKS[mode] & 0xF0 and int(height) != int(width):
        raise ValueError('tta: mode %r transposes the slices and needs square ones, not %d x %d; the mode that works there is flips'
                         % (mode, height, width))
    return MASKS[mode]
