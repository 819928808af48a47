"""Float64 NumPy reference of the resident zoom with a correction mask (the
definition in include/slm_hip.h, "resident zoom"): the masked unit field in
front of the two products of tests/zoom_reference.py. Test infrastructure only:
the package has no CPU path."""
import numpy as np

import zoom_reference as zr


def unit_field(hologram, mask=None, ct2pi=None):
    """u as the device forms it: arg = t - mask, one rounded float64
    subtraction, t = 2 pi level / ct2pi (evaluated as the level table's) or the
    float32 phase widened; its float64 sine and cosine rounded to complex64."""
    if mask is None:
        return zr.unit_field(hologram, ct2pi)
    h = np.asarray(hologram)
    if h.dtype == np.uint8:
        t = (2 * np.pi * np.arange(256, dtype=np.float64) / float(ct2pi))[h]
    else:
        t = h.astype(np.float32).astype(np.float64)
    arg = t - np.asarray(mask, dtype=np.float64)
    return (np.cos(arg).astype(np.float32) + 1j * np.sin(arg).astype(np.float32)).astype(np.complex128)


def zoom(hologram, origin, pitch, size, z=0.0, ain=None, ct2pi=None, mask=None):
    """V [ny][nx] complex128 of one hologram [H][W] with `mask` taken off."""
    u = unit_field(hologram, mask, ct2pi)
    if ain is not None:
        u = np.asarray(ain, np.float32).astype(np.float64) * u
    h, w = u.shape
    dy, dx = (pitch, pitch) if np.ndim(pitch) == 0 else pitch
    py = zr.table(h, origin[0], dy, size[0], z)
    px = zr.table(w, origin[1], dx, size[1], z)
    return np.conj(py).T @ (u @ np.conj(px))
