"""numpy restatement of ``hesic_homonet_prepare_items`` (include/hesic_homonet_items.h) BY DEFINITION: per item, the crop is sliced out of
the stored HWC array and handed to ``homography_prep_ref.prepare`` as if it were the whole image, and the results are stacked.  "The item
form equals the existing form on the crop" is therefore what the GPU test holds the kernel to."""
import numpy as np

import homography_prep_ref as R


def crop(stored, x0, y0, cw, ch):
    """The (1, 3, ch, cw) uint8 NCHW copy of ``stored[y0:y0+ch, x0:x0+cw]`` (``stored``: (rows, pitch_px, 3) uint8)."""
    assert stored.dtype == np.uint8 and stored.ndim == 3 and stored.shape[2] == 3
    assert 0 <= x0 and x0 + cw <= stored.shape[1] and 0 <= y0 and y0 + ch <= stored.shape[0] and cw >= 1 and ch >= 1
    return np.ascontiguousarray(stored[y0:y0 + ch, x0:x0 + cw].transpose(2, 0, 1))[None]


def prepare_items(lefts, rights, geometry, S, P, mean, std):
    """``lefts`` / ``rights``: per item the stored (rows, pitch_px, 3) uint8 arrays; ``geometry``: per item ``(x0, y0, cw, ch, wx, wy)``.
    Returns the five fp32 outputs, items stacked along the batch axis."""
    outs = [R.prepare(crop(a, x0, y0, cw, ch), crop(b, x0, y0, cw, ch), [(wx, wy)], S, P, mean, std)
            for a, b, (x0, y0, cw, ch, wx, wy) in zip(lefts, rights, geometry)]
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(5))
