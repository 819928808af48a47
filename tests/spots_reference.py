"""Float64 NumPy reference of spot-based weighted Gerchberg-Saxton on a trap
list (the definition in include/slm_hip.h, "trap lists", and DESIGN.md section
3) and the trap lists its tests share. The trap phase is separable, so the two
sums are matrix products with the tables Py [H][M] and Px [W][M].
Test infrastructure only: the package has no CPU path."""
import numpy as np

GOLDEN = 0.6180339887498949


def tables(h, w, ys, xs, zs=None):
    """Py [H][M] = exp(i (2 pi k y / H + z (k - H/2)^2)), Px [W][M] likewise."""
    ys, xs = np.asarray(ys, np.float64), np.asarray(xs, np.float64)
    zs = np.zeros_like(ys) if zs is None else np.asarray(zs, np.float64)
    k, l = np.arange(h, dtype=np.float64)[:, None], np.arange(w, dtype=np.float64)[:, None]
    py = np.exp(1j * (2 * np.pi * ((k * ys / h) % 1.0) + zs * (k - h / 2) ** 2))
    px = np.exp(1j * (2 * np.pi * ((l * xs / w) % 1.0) + zs * (l - w / 2) ** 2))
    return py, px


def delta(h, w, y, x, z=0.0):
    """The trap phase D(k, l) of one trap, direct form."""
    k, l = np.arange(h, dtype=np.float64)[:, None], np.arange(w, dtype=np.float64)[None, :]
    return 2 * np.pi * (k * y / h + l * x / w) + z * ((k - h / 2) ** 2 + (l - w / 2) ** 2)


def fields(phase, py, px, ain=None):
    """V_m = sum_kl a exp(i (phase - D_m))."""
    u = np.exp(1j * np.asarray(phase, np.float64))
    if ain is not None:
        u = np.asarray(ain, np.float64) * u
    return np.sum(np.conj(py) * (u @ np.conj(px)), axis=0)


def superpose(c, py, px):
    """angle(sum_m c_m exp(i D_m)), with angle(0) = 0."""
    return np.angle((py * np.asarray(c)) @ px.T)


def start_phase(py, px, intensity):
    m = np.arange(py.shape[1])
    theta = 2 * np.pi * ((m * GOLDEN) % 1.0)
    return superpose(np.sqrt(intensity) * np.exp(1j * theta), py, px)


def statistics(v, intensity, h, w, sum_a2):
    e = np.abs(v) ** 2
    q = e / intensity
    r = q / q.mean()
    return np.array([e.sum() / (h * w * sum_a2), r.std(), r.min(), r.max()])


def spots_reference(shape, ys, xs, zs=None, intensity=None, loops=30, feedback=1.0, ain=None, initial_phase=None,
                    initial_weights=None):
    """(phase [H][W], V [M] of the last iteration, stats [loops][4], w [M] with
    mean 1) of one hologram; feedback = 0 is unweighted spot GS."""
    h, w = shape
    ys = np.asarray(ys, np.float64)
    inten = np.ones_like(ys) if intensity is None else np.asarray(intensity, np.float64)
    a_t = np.sqrt(inten)
    py, px = tables(h, w, ys, xs, zs)
    a = None if ain is None else np.asarray(ain, np.float64)
    sum_a2 = float(h * w) if a is None else float(np.sum(a * a))
    wt = np.ones_like(ys) if initial_weights is None else np.array(initial_weights, np.float64)
    phase = start_phase(py, px, inten) if initial_phase is None else np.asarray(initial_phase, np.float64)
    stats = np.empty((loops, 4))
    v = np.zeros(ys.shape, np.complex128)
    for it in range(loops):
        v = fields(phase, py, px, a)
        amp = np.abs(v)
        stats[it] = statistics(v, inten, h, w, sum_a2)
        ok = amp > 0
        wt[ok] *= np.clip((a_t[ok] / amp[ok]) ** feedback, 2.0 ** -64, 2.0 ** 64)
        wt /= wt.mean()
        unit = np.where(ok, v / np.where(ok, amp, 1.0), 1.0)
        phase = superpose(a_t * wt * unit, py, px)
    return phase, v, stats, wt


def trap_list(h, w, m, seed, zscale=1.0, uniform=False):
    """m traps uniform in the central half of the far field (fractional
    positions, either sign), |z| <= zscale 4 pi / (H^2 + W^2), intensities
    0.5 .. 1 (or ones)."""
    rng = np.random.default_rng(seed)
    ys = rng.uniform(-h / 4, h / 4, m)
    xs = rng.uniform(-w / 4, w / 4, m)
    zs = zscale * rng.uniform(-1, 1, m) * 4 * np.pi / (h * h + w * w)
    inten = np.ones(m) if uniform else rng.uniform(0.5, 1.0, m)
    return ys, xs, zs, inten
