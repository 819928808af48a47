"""Spot-based weighted GS on trap lists (slm_spots_*) on the MI355X against the
float64 NumPy reference of its definition (tests/spots_reference.py). The
feature has no counterpart in the reference project.

The two matrix products are tested alone through the one-shot entries, then the
loop from a warm start as tests/test_gpu_gsw.py does: 30 reference iterations,
the phase and the weights rounded to the float32 the handle takes go to both
sides, which then run 20 further iterations. Gates: the project's float32 phase
bar 1e-5 rms, weights within 5e-6, fields within 1e-6 sum(a) per trap (the
f32 MFMA chain's 0.75 .. 1.5e-7 sum|a b| at K <= 1024 plus two table roundings of
6e-8, the row fold being float64: about 3x margin)."""
import numpy as np
import pytest

import spots_reference as sr
from gsw_reference import incoming_gauss
from oracle import gs_gd_oracle as orc

PHASE_RMS_TOL = 1e-5
WEIGHT_TOL = 5e-6
FIELDS_TOL = 1e-6  # times sum(a), per trap
# 10x the largest deviation from the float64 reference the MI355X showed when
# these tests were first run (test_loop_parity's docstring)
INTENSITY_RTOL = 1.77e-6  # measured 1.763e-7 (the issue caps this gate at 1e-5)
STATS_TOL = 1.9e-6        # measured 1.893e-7

ONE_SHOT = [(45, 70, 5), (64, 64, 1), (96, 160, 33), (130, 264, 70), (64, 64, 1024)]
_IDS = [f"{h}x{w}-{m}" for h, w, m in ONE_SHOT]


def _phase(shape, seed):
    return np.random.default_rng(seed).uniform(-np.pi, np.pi, shape).astype(np.float32)


# ---------------------------------------------------------------------------
# 1. the two products alone
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("h,w,m", ONE_SHOT, ids=_IDS)
def test_fields_product(gpu, h, w, m):
    ys, xs, zs, _ = sr.trap_list(h, w, m, 10 + m)
    phase = _phase((h, w), m)
    py, px = sr.tables(h, w, ys, xs, zs)
    for ain in (None, incoming_gauss(h, w)):
        got = gpu.spots_fields(phase, ys, xs, zs, ain)[0]
        want = sr.fields(phase, py, px, ain)
        sum_a = float(h * w) if ain is None else float(ain.astype(np.float64).sum())
        dev = float(np.max(np.abs(got - want))) / sum_a
        print(f"[spots fields] {h}x{w} {m} traps, a_in {'set' if ain is not None else 'ones'}: "
              f"max |V - V_ref| / sum a = {dev:.3e}")
        assert dev <= FIELDS_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,m", ONE_SHOT, ids=_IDS)
def test_superposition_product(gpu, h, w, m):
    ys, xs, zs, _ = sr.trap_list(h, w, m, 20 + m)
    rng = np.random.default_rng(m)
    c = rng.uniform(0.5, 1.0, m) * np.exp(2j * np.pi * rng.uniform(0, 1, m))
    py, px = sr.tables(h, w, ys, xs, zs)
    got = gpu.spots_superpose((h, w), c, ys, xs, zs)[0]
    rms = orc.phase_rms(got, sr.superpose(c, py, px))
    print(f"[spots superpose] {h}x{w} {m} traps: phase rms {rms:.3e}")
    assert got.dtype == np.float32 and got.shape == (h, w)
    assert rms <= PHASE_RMS_TOL


# ---------------------------------------------------------------------------
# 2. the loop from a warm start
# ---------------------------------------------------------------------------
def _run(gpu, shape, lists, loops, feedback=1.0, ain=None, phase=None, weights=None):
    """One run of a fresh handle; lists = [(ys, xs, zs, intensity)] per hologram."""
    h, w = shape
    cols = [np.stack([li[k] for li in lists]) for k in range(4)]
    with gpu.Spots(len(lists), h, w, cols[0].shape[1], ain is not None, loops) as sp:
        sp.set_traps(*cols)
        if ain is not None:
            sp.set_ain(ain)
        sp.set_feedback(feedback)
        sp.set_phase(phase)
        sp.set_weights(weights)
        sp.run(loops)
        return sp.read()


PARITY = [
    # id, shape, trap-list seeds (one per hologram), traps, feedback, a_in
    ("45x70-5", (45, 70), (1,), 5, 1.0, False),
    ("45x70-5-p0.5", (45, 70), (1,), 5, 0.5, False),
    ("96x160-33", (96, 160), (2,), 33, 1.0, False),
    ("96x160-33-p0.5", (96, 160), (2,), 33, 0.5, False),
    ("130x264-70", (130, 264), (3,), 70, 1.0, False),
    ("130x264-70-p0.5", (130, 264), (3,), 70, 0.5, False),
    ("96x160-33-ain", (96, 160), (4,), 33, 1.0, True),
    ("2x96x160-33", (96, 160), (5, 6), 33, 1.0, False),
]
WARM, MORE = 30, 20
_PARITY_RUNS = {}


def _parity_run(gpu, label, shape, seeds, m, feedback, with_ain):
    """Reference and device results of one parity case, computed once."""
    if label in _PARITY_RUNS:
        return _PARITY_RUNS[label]
    h, w = shape
    ain = incoming_gauss(h, w) if with_ain else None
    lists = [sr.trap_list(h, w, m, s) for s in seeds]
    ph0, w0, want = [], [], []
    for li in lists:
        ph, _, _, wt = sr.spots_reference(shape, *li, loops=WARM, feedback=feedback, ain=ain)
        ph0.append(ph.astype(np.float32))
        w0.append(wt.astype(np.float32))
        want.append(sr.spots_reference(shape, *li, loops=MORE, feedback=feedback, ain=ain, initial_phase=ph0[-1],
                                       initial_weights=w0[-1]))
    got = _run(gpu, shape, lists, MORE, feedback, ain, np.stack(ph0), np.stack(w0))
    _PARITY_RUNS[label] = (want, got)
    return _PARITY_RUNS[label]


def _deviations(want, got, k):
    phase, v, stats, wt = got
    rms = orc.phase_rms(phase[k], want[k][0])
    dw = float(np.max(np.abs(wt[k].astype(np.float64) - want[k][3])))
    i_ref = np.abs(want[k][1]) ** 2
    di = float(np.max(np.abs(np.abs(v[k]) ** 2 / i_ref - 1)))
    ds = np.abs(stats[k] - want[k][2])
    ds[:, 0] /= want[k][2][:, 0]  # the efficiency relative, the others (uniformity, min r, max r ~ 1) absolute
    return rms, dw, di, float(ds.max())


@pytest.mark.gpu
@pytest.mark.parametrize("label,shape,seeds,m,feedback,with_ain", PARITY, ids=[c[0] for c in PARITY])
def test_loop_parity(gpu, label, shape, seeds, m, feedback, with_ain):
    """Measured (MI355X) when first run, over these nine holograms: phase rms
    1.6e-7 .. 6.4e-7 of the 1e-5 bar, max |dw| 2.3e-8 .. 1.1e-7 of 5e-6,
    per-trap intensities within 4.9e-8 .. 1.763e-7 relative, the four
    statistics (efficiency relative, the others absolute) within 1.0e-7 ..
    1.893e-7. The last two gates are 10x those largest figures."""
    want, got = _parity_run(gpu, label, shape, seeds, m, feedback, with_ain)
    assert got[2].shape == (len(seeds), MORE, 4)
    for k in range(len(seeds)):
        rms, dw, di, ds = _deviations(want, got, k)
        print(f"[spots parity] {label}[{k}] p={feedback} +{MORE}: phase rms {rms:.3e}, max |dw| {dw:.3e}, "
              f"intensities max rel {di:.3e}, statistics max dev {ds:.3e}")
        assert rms <= PHASE_RMS_TOL
        assert dw <= WEIGHT_TOL
        assert di <= INTENSITY_RTOL
        assert ds <= STATS_TOL


# ---------------------------------------------------------------------------
# 3. cold start: the weights make the traps uniform
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_cold_start_uniformity(gpu):
    shape = (96, 160)
    li = sr.trap_list(96, 160, 12, 2)
    u_w = _run(gpu, shape, [li], 60, 1.0)[2][0, -1, 1]
    u_0 = _run(gpu, shape, [li], 60, 0.0)[2][0, -1, 1]
    print(f"[spots] device 96x160 12 traps, 60 iterations from the default start: uniformity p=0 {u_0:.3e}, "
          f"p=1 {u_w:.3e}")
    assert u_w <= 0.005 and u_w <= u_0 / 5


# ---------------------------------------------------------------------------
# 4. identities on the device
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("y,x", [(7, 11), (-3, 5)])
def test_single_trap_is_update_hologram(gpu, y, x):
    from spatial_light_modulator_module_amd import move_traps as mt

    shape = (45, 70)
    want = mt.update_hologram(np.zeros(shape, np.uint8), [(y, x)], 0)
    got = mt.trap_array_hologram(shape, [float(y)], [float(x)], loops=3)[0]
    diff = np.abs(np.angle(np.exp(1j * (got - want))))
    print(f"[spots] single trap ({y}, {x}) against update_hologram: max |d phase| {diff.max():.3e}")
    assert diff.max() <= 1e-6


@pytest.mark.gpu
def test_fields_at_integer_traps_are_fft2(gpu):
    h, w = 45, 70
    phase = _phase((h, w), 9)
    ain = incoming_gauss(h, w)
    ys, xs = np.array([0.0, 3.0, 44.0, 20.0, 31.0]), np.array([0.0, 69.0, 5.0, 33.0, 1.0])
    field = ain.astype(np.float64) * np.exp(1j * phase.astype(np.float64))
    want = gpu.fft2_c128(field)[ys.astype(int), xs.astype(int)]
    got = gpu.spots_fields(phase, ys, xs, None, ain)[0]
    dev = float(np.max(np.abs(got - want))) / float(ain.astype(np.float64).sum())
    print(f"[spots fields] integer traps against fft2_c128: max |dV| / sum a = {dev:.3e}")
    assert dev <= FIELDS_TOL


@pytest.mark.gpu
def test_feedback_zero_leaves_weights_at_one(gpu):
    li = sr.trap_list(45, 70, 5, 7)
    wt = _run(gpu, (45, 70), [li], 10, 0.0)[3]
    assert np.all(wt == 1.0)


# ---------------------------------------------------------------------------
# 5. state
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_state(gpu):
    shape = (45, 70)
    lists = [sr.trap_list(45, 70, 5, s) for s in (1, 2, 3)]
    cols = [np.stack([li[k] for li in lists]) for k in range(4)]
    ph = _phase((3,) + shape, 4)
    w0 = np.random.default_rng(5).uniform(0.8, 1.2, (3, 5)).astype(np.float32)
    with gpu.Spots(3, 45, 70, 5, False, 12) as sp:
        sp.set_traps(*cols)
        with pytest.raises(gpu.SlmError) as ei:
            sp.read()
        assert ei.value.code == gpu.ERR_STATE
        sp.set_phase(ph)
        sp.set_weights(w0)
        sp.run(12)
        first = sp.read()
        sp.run(12)  # starts from the host-set phase and weights again
        for a, b in zip(first, sp.read()):
            np.testing.assert_array_equal(a, b)
        assert first[3].std() > 1e-4  # the weights did move
        # hologram k of the batch equals the same list run alone, bit for bit
        for k in range(3):
            one = _run(gpu, shape, lists[k:k + 1], 12, 1.0, None, ph[k:k + 1], w0[k:k + 1])
            for a, b in zip(first, one):
                np.testing.assert_array_equal(a[k], b[0])
        # set_weights(None) and set_phase(None) return to the defaults
        sp.set_weights(None)
        sp.set_phase(None)
        sp.run(12)
        fresh = _run(gpu, shape, lists, 12)
        for a, b in zip(sp.read(), fresh):
            np.testing.assert_array_equal(a, b)
        assert not np.array_equal(first[0], fresh[0])
        # set_traps returns the weights to ones
        sp.set_weights(w0)
        sp.set_traps(*cols)
        sp.run(12)
        for a, b in zip(sp.read(), fresh):
            np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(gpu):
    def arg_error(call):
        with pytest.raises(gpu.SlmError) as ei:
            call()
        assert ei.value.code == gpu.ERR_ARG

    for h, w in ((1, 64), (64, 1), (4097, 64), (64, 4097)):
        arg_error(lambda: gpu.Spots(1, h, w, 4))
    arg_error(lambda: gpu.Spots(1, 64, 64, 0))
    arg_error(lambda: gpu.Spots(1, 64, 64, 1025))
    ys, xs, zs, inten = sr.trap_list(64, 64, 4, 1)
    with gpu.Spots(1, 64, 64, 4, False, 5) as sp:
        arg_error(lambda: sp.set_traps([], []))
        arg_error(lambda: sp.set_traps(np.zeros(5), np.zeros(5)))
        for bad in (np.nan, np.inf):
            arg_error(lambda: sp.set_traps(np.array([bad, 1, 2, 3.0]), xs))
            arg_error(lambda: sp.set_traps(ys, xs, np.array([0, bad, 0, 0.0])))
        for bad in (0.0, -1.0, np.nan, np.inf):
            arg_error(lambda: sp.set_traps(ys, xs, zs, np.array([1, 1, bad, 1.0])))
        sp.set_traps(ys, xs, zs, inten)
        for bad in (0.0, -1.0, np.nan, np.inf):
            arg_error(lambda: sp.set_weights(np.array([1, bad, 1, 1.0])))
        for bad in (-0.5, float("nan"), float("inf")):
            arg_error(lambda: sp.set_feedback(bad))
        arg_error(lambda: sp.run(0))
        arg_error(lambda: sp.run(6))
        sp.run(5)  # the handle is still good


# ---------------------------------------------------------------------------
# 7. the Python layer
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_python_layer(gpu):
    from spatial_light_modulator_module_amd import constants
    from spatial_light_modulator_module_amd import move_traps as mt

    shape = (45, 70)
    ys, xs, zs, inten = sr.trap_list(45, 70, 5, 8)
    holo, trap_i, stats, wt = mt.trap_array_hologram(shape, ys, xs, zs, inten, loops=8)
    assert holo.dtype == np.float64 and holo.shape == shape
    assert trap_i.shape == (5,) and stats.shape == (8, 4) and wt.shape == (5,)
    want = sr.spots_reference(shape, ys, xs, zs, inten, loops=8)
    assert orc.phase_rms(holo, want[0]) <= PHASE_RMS_TOL
    lists = [sr.trap_list(45, 70, 5, s) for s in (8, 9)]
    cols = [np.stack([li[k] for li in lists]) for k in range(4)]
    bh, bi, bs, bw = mt.trap_array_hologram(shape, *cols, loops=8)
    assert bh.shape == (2,) + shape and bi.shape == (2, 5) and bs.shape == (2, 8, 4) and bw.shape == (2, 5)
    np.testing.assert_array_equal(bh[0], holo)
    mask = np.random.default_rng(1).uniform(0, 2 * np.pi, shape)
    h2, frame, _, _, _ = mt.trap_array_frame(shape, ys, xs, zs, inten, loops=8, mask=mask, ct2pi=200)
    np.testing.assert_array_equal(h2, holo)
    np.testing.assert_array_equal(frame, mt.hologram_frame(holo, mask, True, 200))
    assert frame.dtype == np.uint8
    f = 0.4
    assert mt.lens_to_z(f) == -np.pi * constants.px_distance ** 2 / (constants.wavelength * f)
    mt.clear_spots()
