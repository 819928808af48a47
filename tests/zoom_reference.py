"""Float64 NumPy reference of the zoomed far field (the definition in
include/slm_hip.h, "zoomed far field", and DESIGN.md section 3): two matrix
products with the trap lists' tables (tests/spots_reference.py), the same frac
before the sine, the same rounding of u to complex64. Test infrastructure
only: the package has no CPU path."""
import numpy as np


def unit_field(hologram, ct2pi=None):
    """u as the device forms it: float64 sine and cosine rounded to complex64,
    of a float32 phase or of 2 pi level / ct2pi for a uint8 frame."""
    h = np.asarray(hologram)
    if h.dtype == np.uint8:
        arg = (2 * np.pi * np.arange(256, dtype=np.float64) / float(ct2pi))[h]
    else:
        arg = h.astype(np.float32).astype(np.float64)
    return (np.cos(arg).astype(np.float32) + 1j * np.sin(arg).astype(np.float32)).astype(np.complex128)


def table(n_pix, pos0, pitch, count, z):
    """P[n][s] = exp(i (2 pi frac(n p_s / N) + z (n - N/2)^2)), p_s = pos0 + s pitch."""
    n = np.arange(n_pix, dtype=np.float64)[:, None]
    p = np.float64(pos0) + np.arange(count, dtype=np.float64) * np.float64(pitch)
    return np.exp(1j * (2 * np.pi * ((n * p / n_pix) % 1.0) + z * (n - n_pix / 2) ** 2))


def zoom(hologram, origin, pitch, size, z=0.0, ain=None, ct2pi=None):
    """V [ny][nx] complex128 of one hologram [H][W]; the intensity is |V|^2."""
    u = unit_field(hologram, ct2pi)
    if ain is not None:
        u = np.asarray(ain, np.float32).astype(np.float64) * u
    h, w = u.shape
    dy, dx = (pitch, pitch) if np.ndim(pitch) == 0 else pitch
    py = table(h, origin[0], dy, size[0], z)
    px = table(w, origin[1], dx, size[1], z)
    r = u @ np.conj(px)          # product 1: [H][nx]
    return np.conj(py).T @ r     # product 2: [ny][nx]


def sum_a(shape, ain=None):
    return float(shape[0] * shape[1]) if ain is None else float(np.sum(np.abs(np.asarray(ain, np.float64))))
