"""The weighted-GS reference after it learned an incoming amplitude: without
one it is the function the parity gates were set against, bit for bit, and
with one it computes B = a_in exp(i angle(A))."""
import numpy as np
import pytest

from gsw_reference import gsw_reference, incoming_gauss, traps


def _reference_before_ain(target, loops, feedback=1.0, initial_phase=None, initial_weights=None):
    """gsw_reference as it stood before the a_in argument, kept verbatim."""
    t = np.asarray(target)
    a_t = np.sqrt(t).astype(np.float64)
    sup = t > 0
    tf = t.astype(np.float64)
    g = np.ones(t.shape) if initial_weights is None else np.array(initial_weights, np.float64)
    g[~sup] = 1.0
    a = np.fft.ifft2(a_t) if initial_phase is None else np.exp(1j * np.asarray(initial_phase, np.float64))
    errs = []
    for _ in range(loops):
        c = np.fft.fft2(np.exp(1j * np.angle(a)))
        amp = np.abs(c)
        upd = sup & (amp > 0)
        g[upd] *= (a_t[upd] / amp[upd]) ** feedback
        g[sup] /= g[sup].mean()
        a = np.fft.ifft2(a_t * g * np.exp(1j * np.angle(c)))
        e = amp ** 2
        errs.append(np.sum((e * (tf.max() / e.max()) - tf) ** 2) / t.size)
    return np.angle(a), e, errs, g


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("feedback", [0.0, 0.75, 1.0])
@pytest.mark.parametrize("warm", [False, True])
def test_no_ain_is_bitwise_the_previous_reference(dtype, feedback, warm):
    t = traps(128, 64, 24, 11, True).astype(dtype)
    rng = np.random.default_rng(5)
    kw = {}
    if warm:
        kw = dict(initial_phase=rng.uniform(0, 2 * np.pi, t.shape).astype(np.float32),
                  initial_weights=rng.uniform(0.5, 1.5, t.shape).astype(np.float32))
    want = _reference_before_ain(t, 7, feedback, **kw)
    factors = []
    for got in (gsw_reference(t, 7, feedback, **kw), gsw_reference(t, 7, feedback, ain=None, factors=factors, **kw)):
        for a, b in zip(want, got):
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    assert len(factors) == 7 and all(0 < lo <= hi for lo, hi in factors)


def test_ain_enters_the_forward_transform_only():
    """A uniform a_in of ones is no a_in at all; a power-of-two a_in scales C,
    E by its square, and leaves phase, weights and error where they were (the
    weights are normalised, the error is of E / max E)."""
    t = traps(64, 64, 12, 11, True)
    ph0 = np.random.default_rng(5).uniform(0, 2 * np.pi, t.shape)
    base = gsw_reference(t, 6, 1.0, initial_phase=ph0)
    ones = gsw_reference(t, 6, 1.0, initial_phase=ph0, ain=np.ones(t.shape, np.float32))
    for a, b in zip(base, ones):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    four = gsw_reference(t, 6, 1.0, initial_phase=ph0, ain=np.full(t.shape, 4.0, np.float32))
    np.testing.assert_array_equal(four[1], 16.0 * base[1])
    np.testing.assert_allclose(four[0], base[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(four[3], base[3], rtol=1e-12)
    np.testing.assert_allclose(four[2], base[2], rtol=1e-12)
    # a shaped a_in is B = a_in exp(i angle(A)): one iteration by hand
    ain = incoming_gauss(64, 64)
    assert ain.dtype == np.float32 and 0.2 < ain.min() < ain.max() <= 1.2
    got = gsw_reference(t, 1, 0.0, initial_phase=ph0, ain=ain)
    c = np.fft.fft2(ain.astype(np.float64) * np.exp(1j * np.angle(np.exp(1j * ph0))))
    np.testing.assert_array_equal(got[1], np.abs(c) ** 2)
