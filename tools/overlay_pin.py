"""Pin tests/overlay_oracle.py's resize against the library the reference uses: scikit-image 0.13.1 (its requirements.txt).

    python tools/overlay_pin.py [--any-version]

On a machine that has that version installed this calls skimage.transform.resize (its defaults there: order 1, mode 'constant',
cval 0, clip True, preserve_range False) on the seeded arrays of tests/test_overlay_host.py (pin_arrays) and writes
tests/golden/skimage_resize_v1.npz; test_resize_against_scikit_image_pin then holds the oracle to 1e-12 of it.  Until the file
exists that test skips with "resize UNPINNED against scikit-image 0.13.1", and the contract's restatement of the rule stands alone."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    try:
        import skimage
        from skimage.transform import resize
    except ImportError:
        raise SystemExit('overlay_pin: scikit-image is not installed here; run this where scikit-image 0.13.1 is')
    if skimage.__version__ != '0.13.1' and '--any-version' not in sys.argv:
        raise SystemExit('overlay_pin: scikit-image %s found, the reference pins 0.13.1 (--any-version writes the file anyway: later '
                         'versions changed the default mode and anti-aliasing)' % skimage.__version__)
    from test_overlay_host import pin_arrays, PIN
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')               # 0.13.1 announces the coming change of the default mode
        for name, (a, (H, W)) in pin_arrays().items():
            out[name] = np.asarray(resize(a, (H, W)), np.float64)
    np.savez(PIN, **out)
    print('wrote %s (scikit-image %s): %s' % (PIN, skimage.__version__, ', '.join(sorted(out))))


if __name__ == '__main__':
    main()
