"""Float64 NumPy reference of weighted Gerchberg-Saxton (the definition in
DESIGN.md section 3, "Weighted GS") and the trap targets its tests share.
Test infrastructure only: the package has no CPU path."""
import numpy as np


def traps(h, w, nt, seed, gray):
    """nt single-pixel traps at random places, 255 or (gray) 60..255, uint8."""
    rng = np.random.default_rng(seed)
    t = np.zeros((h, w), np.uint8)
    idx = rng.choice(h * w, nt, replace=False)
    t.flat[idx] = rng.integers(60, 256, nt) if gray else 255
    return t


def uniformity(e, t):
    """std / mean of E / T over the support T > 0."""
    sup = np.asarray(t) > 0
    r = np.asarray(e, np.float64)[sup] / np.asarray(t, np.float64)[sup]
    return float(r.std() / r.mean())


def incoming_gauss(h, w):
    """The incoming amplitude the a_in tests share: a wide Gaussian on a 0.2
    pedestal, float32 (0.2 + exp(-(((y - H/2) / 0.35 H)^2 + ((x - W/2) / 0.35 W)^2)))."""
    y = (np.arange(h)[:, None] - h / 2) / (0.35 * h)
    x = (np.arange(w)[None, :] - w / 2) / (0.35 * w)
    return (0.2 + np.exp(-(y ** 2 + x ** 2))).astype(np.float32)


def gsw_reference(target, loops, feedback=1.0, initial_phase=None, initial_weights=None, ain=None, factors=None):
    """(phase, E, error_evolution, g): g normalised to mean 1 over the support,
    1 off it. feedback = 0 is plain GS. The amplitude follows numpy's dtype
    rule as GS does: float16 sqrt for uint8 targets, float32 for float32.
    ain: the incoming amplitude a_in [H][W] of B = a_in exp(i angle(A)); None is
    uniform and computes what this function computed before it took a_in, bit
    for bit. factors: a list that receives (min, max) of every iteration's
    update factor (a_T / |C|)^feedback (an observer; the kernels clamp it to
    [2^-64, 2^64] and the tests assert that the clamp is idle)."""
    t = np.asarray(target)
    a_t = np.sqrt(t).astype(np.float64)
    sup = t > 0
    tf = t.astype(np.float64)
    g = np.ones(t.shape) if initial_weights is None else np.array(initial_weights, np.float64)
    g[~sup] = 1.0
    a = np.fft.ifft2(a_t) if initial_phase is None else np.exp(1j * np.asarray(initial_phase, np.float64))
    errs = []
    for _ in range(loops):
        b = np.exp(1j * np.angle(a))
        c = np.fft.fft2(b if ain is None else np.asarray(ain, np.float64) * b)
        amp = np.abs(c)
        upd = sup & (amp > 0)
        f = (a_t[upd] / amp[upd]) ** feedback
        if factors is not None:
            factors.append((float(f.min()), float(f.max())))
        g[upd] *= f
        g[sup] /= g[sup].mean()
        a = np.fft.ifft2(a_t * g * np.exp(1j * np.angle(c)))
        e = amp ** 2
        errs.append(np.sum((e * (tf.max() / e.max()) - tf) ** 2) / t.size)
    return np.angle(a), e, errs, g
