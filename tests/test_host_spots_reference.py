"""The float64 reference of spot-based weighted GS (tests/spots_reference.py)
checked against its own definition on the CPU: the separable tables against the
direct sums, the identities that tie it to the rest of the package, and that
the weights do what they are for."""
import numpy as np
import pytest

import spots_reference as sr


def test_separable_form_equals_direct_sums():
    h, w = 12, 20
    ys, xs, zs, inten = sr.trap_list(h, w, 3, 1)
    rng = np.random.default_rng(2)
    phase = rng.uniform(-np.pi, np.pi, (h, w))
    ain = rng.uniform(0.2, 1.0, (h, w))
    py, px = sr.tables(h, w, ys, xs, zs)
    d = [sr.delta(h, w, ys[m], xs[m], zs[m]) for m in range(3)]
    v_direct = np.array([np.sum(ain * np.exp(1j * (phase - d[m]))) for m in range(3)])
    np.testing.assert_allclose(sr.fields(phase, py, px, ain), v_direct, rtol=0, atol=1e-12)
    c = rng.normal(size=3) + 1j * rng.normal(size=3)
    s_direct = sum(c[m] * np.exp(1j * d[m]) for m in range(3))
    diff = np.angle(np.exp(1j * (sr.superpose(c, py, px) - np.angle(s_direct))))
    assert np.max(np.abs(diff)) <= 1e-12


def test_single_integer_trap_is_the_plane_wave():
    h, w = 12, 20
    one_hot = np.zeros((h, w))
    one_hot[5, 7] = 255.0
    phase, _, _, wt = sr.spots_reference((h, w), [5.0], [7.0], loops=3)
    diff = np.angle(np.exp(1j * (phase - np.angle(np.fft.ifft2(one_hot)))))
    assert np.max(np.abs(diff)) <= 2e-13
    assert wt[0] == 1.0


def test_fields_at_integer_traps_are_fft2():
    h, w = 12, 20
    rng = np.random.default_rng(3)
    phase = rng.uniform(-np.pi, np.pi, (h, w))
    ain = rng.uniform(0.2, 1.0, (h, w))
    ys, xs = np.array([0.0, 3.0, 11.0, 6.0]), np.array([0.0, 19.0, 4.0, 10.0])
    py, px = sr.tables(h, w, ys, xs)
    want = np.fft.fft2(ain * np.exp(1j * phase))[ys.astype(int), xs.astype(int)]
    np.testing.assert_allclose(sr.fields(phase, py, px, ain), want, rtol=0, atol=2e-12)


def test_feedback_zero_leaves_the_weights_at_one():
    ys, xs, zs, inten = sr.trap_list(40, 72, 5, 4)
    _, _, _, wt = sr.spots_reference((40, 72), ys, xs, zs, inten, loops=10, feedback=0.0)
    assert np.all(wt == 1.0)


@pytest.mark.parametrize("h,w,m,seed", [(40, 72, 5, 1), (96, 160, 12, 2)])
def test_weights_improve_uniformity(h, w, m, seed):
    ys, xs, zs, inten = sr.trap_list(h, w, m, seed)
    u0 = sr.spots_reference((h, w), ys, xs, zs, inten, loops=30, feedback=0.0)[2][-1, 1]
    u1 = sr.spots_reference((h, w), ys, xs, zs, inten, loops=30, feedback=1.0)[2][-1, 1]
    print(f"[spots reference] {h}x{w} {m} traps, 30 iterations: uniformity p=0 {u0:.3e}, p=1 {u1:.3e}")
    assert u1 <= 0.005 and u1 <= u0 / 5
