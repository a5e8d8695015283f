"""What the host-side pipeline modules (metrics, postprocessing, resampling, augmentation, preprocessing, inference2d) share: the way a caller's numpy array or torch tensor reaches the working device and finds its way back, and the cubic B-spline tap weights of
scipy.ndimage that resampling and inference2d put into their per-axis tables."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L

_KIND_NAMES = {"biuf": "integer, bool or floating", "iuf": "integer or floating"}


def to_working_device(x, who, what, kinds="biuf", plural=False):
    """A detached tensor on the working device.  numpy arrays whose dtype kind is not in ``kinds`` are refused in the name of module ``who``
    (``kinds=None``: no check); unsigned integers wider than a byte, which torch does not have, come as int64."""
    if isinstance(x, torch.Tensor):
        t = x.detach()
    else:
        a = np.asarray(x)
        if kinds is not None and a.dtype.kind not in kinds:
            names = _KIND_NAMES[kinds]
            raise RuntimeError(f"{who}: {what} are {names} arrays, got {a.dtype}" if plural else
                               f"{who}: {what} is an {names} array, got {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a.astype(np.int64) if a.dtype.kind == "u" and a.dtype.itemsize > 1 else a))
    if not L._test_backend and not t.is_cuda and torch.cuda.is_available():
        t = t.cuda()
    return t


def load(x, who, what, kinds="biuf", plural=False):
    """(tensor on the working device, ``back(r, dtype=None)`` that gives a result tensor the container and device the caller expects: a tensor
    on x's device for a tensor, numpy for anything else; in x's dtype, or in the torch ``dtype`` named)."""
    t = to_working_device(x, who, what, kinds, plural)
    if isinstance(x, torch.Tensor):
        def back(r, dtype=None):
            return r.to(device=x.device, dtype=x.dtype if dtype is None else dtype)
    else:
        a_dtype = np.asarray(x).dtype

        def back(r, dtype=None):
            if dtype is None:
                return r.cpu().numpy().astype(a_dtype, copy=False)
            return r.to(dtype).cpu().numpy()
    return t, back


def cubic_bspline_weights(frac):
    """(n, 4) float64: the weights of the four cells floor(c) - 1 .. floor(c) + 2 at the fractional parts ``frac`` = c - floor(c), in the order
    of operations of scipy.ndimage's spline evaluation."""
    y = np.asarray(frac, dtype=np.float64)
    z = 1.0 - y
    w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w0 = z * z * z / 6.0
    return np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2], 1)
