"""Float64 NumPy reference of MRAF, mixed-region amplitude freedom (the
definition in DESIGN.md section 3, "MRAF"), and the drawn-shape target its
tests share. Test infrastructure only: the package has no CPU path."""
import numpy as np


def shapes(h, w):
    """(target, region), both uint8: a filled ellipse of 200 and a rectangle of
    120 in the upper left quarter, inside a rectangular signal region."""
    y, x = np.mgrid[:h, :w]
    cy, cx = h // 4, w // 4
    t = np.zeros((h, w), np.uint8)
    t[((y - cy) / (h / 10)) ** 2 + ((x - cx) / (w / 7)) ** 2 <= 1] = 200
    t[cy + h // 8: cy + h // 8 + h // 12, cx - w // 10: cx + w // 8] = 120
    r = np.zeros((h, w), np.uint8)
    r[cy - h // 6: cy + h // 4 + 2, cx - w // 5: cx + w // 5] = 1
    return t, r


def start_phase(shape):
    """The start phase the tests share."""
    return np.random.default_rng(5).uniform(0, 2 * np.pi, shape)


def amplitude(target):
    """a_T as GS takes it: numpy's sqrt (float16 for uint8 targets, float32 for
    float32 ones), carried in float64."""
    return np.sqrt(np.asarray(target)).astype(np.float64)


def mraf_reference(target, region, loops, mixing=0.4, initial_phase=None, ain=None, a_t=None):
    """(phase, E, error_evolution, efficiency_evolution) after `loops`
    iterations. region: nonzero = signal region sr. The error is GS's error_f
    restricted to sr, the efficiency sum_sr E / P with P = S sum a_in^2. T
    outside sr plays no part except in the cold start ifft2(a_T), which is GS's
    own on the target as given. a_t overrides the amplitude (the comparison
    with the pinned GS oracle feeds both sides the same one)."""
    t = np.asarray(target)
    tf = t.astype(np.float64)
    a_t = amplitude(t) if a_t is None else np.asarray(a_t, np.float64)
    sr = np.asarray(region) > 0
    m = float(mixing)
    a_in = np.ones(t.shape) if ain is None else np.asarray(ain, np.float64)
    power = t.size * np.sum(a_in ** 2)
    kappa = np.sqrt(power / np.sum(a_t[sr] ** 2))
    a = np.fft.ifft2(a_t) if initial_phase is None else np.exp(1j * np.asarray(initial_phase, np.float64))
    norm = tf[sr].max()
    n_sr = np.count_nonzero(sr)
    errs, effs = [], []
    for _ in range(loops):
        b = a_in * np.exp(1j * np.angle(a))
        c = np.fft.fft2(b)
        e = np.abs(c) ** 2
        d = np.where(sr, m * kappa * a_t * np.exp(1j * np.angle(c)), (1.0 - m) * c)
        a = np.fft.ifft2(d)
        errs.append(np.sum((e[sr] * (norm / e[sr].max()) - tf[sr]) ** 2) / n_sr)
        effs.append(np.sum(e[sr]) / power)
    return np.angle(a), e, np.array(errs), np.array(effs)
