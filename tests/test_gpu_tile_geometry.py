"""Forced tile geometries and plan variants of the any-size engine
(csrc/generic.hip, mr_inst.hip, rz_inst.hip, radix_c128.hpp).

The engine takes its tiles and kernel instantiations from heuristics that read
the shape, the batch and the device's CU count, so the other files of the
suite run what those pick at their shapes on one device. Here the overrides
the heuristics honour ($SLM_MR_RPW, $SLM_MR_CW; $SLM_RZ_ROW_PLAN,
$SLM_RZ_COL_PLAN, $SLM_RZ_PLAN, $SLM_RZ_CW, $SLM_RZ_LAYOUT, $SLM_RZ_PANEL)
force the rest of the built code: multi-row tiles with a tail tile, ragged
multi-column tiles (zero-padded columns the statistics must skip), every
column-tile width of the radix-plan kernels, both plan variants per axis and
both state layouts. Every plan asserts through Plan.generic_info() the
geometry it runs -- an override the build does not accept falls back to
another back end without a message -- and nothing is asserted about what the
heuristics would pick.

References: numpy.fft for the transforms, the faithful float64 oracle
(oracle/gs_gd_oracle.py, SURVEY.md 8c warm-start protocol) for GS and GD, at
the bars of the sibling files (test_gpu_generic.py, test_gpu_radix_c128.py,
test_gpu_radix_c64.py). A line's butterflies do not depend on the tile that
holds it, so on the mixed-radix back end transforms and phases are also held
bit for bit to the one-row / one-column geometry; statistics regroup their
partial sums per column tile (rtol 1e-12).
"""
import functools

import numpy as np
import pytest

from oracle import gs_gd_oracle as orc

KNOBS = ("SLM_MR_RPW", "SLM_MR_CW", "SLM_RZ_PLAN", "SLM_RZ_ROW_PLAN", "SLM_RZ_COL_PLAN", "SLM_RZ_CW",
         "SLM_RZ_LAYOUT", "SLM_RZ_PANEL", "SLM_ENGINE", "SLM_GENERIC_ENGINE", "SLM_PRECISION")

# plan keys (csrc/plans.hpp kPlans indices) of the (length, variant) pairs used here:
# variant 0 wide, 1 narrow, 2 the 4096-point E = 8 plan, 3 / 4 the panel plans
KEY = {(64, "wide"): 0, (256, "wide"): 2, (256, "narrow"): 8, (512, "wide"): 3, (512, "narrow"): 9,
       (4096, "narrow"): 13, (4096, "e8"): 14, (600, "main"): 15, (1920, "main"): 23, (1920, "alt"): 24}


@pytest.fixture
def knobs(monkeypatch):
    """set(**env) sets or (None) unsets the engine's overrides, read at plan creation."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)

    def set_(**env):
        for k, v in env.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))

    yield set_
    from spatial_light_modulator_module_amd import algorithms as alg

    alg.clear_plans()  # the drop-in's plans and slm_fft2_c128's engines


def _target(shape, u8, seed):
    rng = np.random.default_rng(seed)
    if u8:
        return rng.integers(0, 256, shape).astype(np.uint8)
    return rng.uniform(0, 255, shape).astype(np.float32)


def _ain(shape):
    a = np.sqrt(np.random.default_rng(12).uniform(0.25, 2.0, shape)).astype(np.float32)
    return a, a.astype(np.float64) ** 2  # a_in; the oracle takes the intensity


def _x(shape, dtype, seed=2):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((2,) + shape) + 1j * rng.standard_normal((2,) + shape)).astype(dtype)


@functools.lru_cache(maxsize=None)
def _fft_ref(shape, dtype, inverse):
    x = _x(shape, dtype).astype(np.complex128)
    want = np.fft.ifft2(x) * (shape[0] * shape[1]) if inverse else np.fft.fft2(x)
    want.setflags(write=False)
    return want


def _max_err(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


@functools.lru_cache(maxsize=None)
def _gs_warm_ref(shape, u8, with_ain, loops, seed):
    """the oracle's phase after 30 cold iterations, then `loops` more."""
    t = _target(shape, u8, seed)
    ain, inten = _ain(shape) if with_ain else (None, None)
    phi30, _, _ = orc.gerchberg_saxton_faithful(t, 30, incoming_intensity=inten)
    phi30 = phi30.astype(np.float32)
    ref, ref_e, ref_err = orc.gerchberg_saxton_faithful(t, loops, incoming_intensity=inten, initial_phase=phi30)
    for a in (phi30, ref, ref_e):
        a.setflags(write=False)
    return t, ain, phi30, ref, ref_e, np.array(ref_err)


@functools.lru_cache(maxsize=None)
def _gd_ref(shape, u8, with_ain, loops, seed):
    """GD from the host-set random guess (seed 42)."""
    from spatial_light_modulator_module_amd import algorithms as alg

    t = _target(shape, u8, seed)
    ain, inten = _ain(shape) if with_ain else (None, None)
    x0 = alg.make_initial_guess("random", None if inten is None else inten ** 0.5, t, 42)
    ref, _, ref_err, _ = orc.gradient_descent_faithful(t, loops, 0.005, 1.0, 0, incoming_intensity=inten,
                                                       initial_field=x0)
    return t, ain, x0, ref, np.array(ref_err)


@functools.lru_cache(maxsize=None)
def _gd_fourier_ref(shape, loops, seed):
    t = _target(shape, False, seed)
    ref1, _, _, _ = orc.gradient_descent_faithful(t, 1, 0.005, 1.0, 0, initial_guess="fourier")
    _, _, ref_err, _ = orc.gradient_descent_faithful(t, loops, 0.005, 1.0, 0, initial_guess="fourier")
    return t, ref1, np.array(ref_err)


def _check_info(gi, expect):
    for k, v in expect.items():
        assert gi[k] == v, (k, gi, expect)


def _run(lib, algo, t, loops, expect, phase=None, field=None, ain=None, tol=0.0, checked=False):
    """One plan: asserts the geometry it was created with, runs, reads back."""
    b, h, w = t.shape
    tt = lib.TGT_U8 if t.dtype == np.uint8 else lib.TGT_F32
    with lib.Plan(algo, b, h, w, tt, ain is not None, loops) as p:
        gi = p.generic_info()
        _check_info(gi, expect)
        p.set_target(t)
        if ain is not None:
            p.set_ain(ain)
        if algo == lib.ALGO_GS:
            p.set_phase(phase)
            p.run(loops, tol, checked)
        else:
            p.set_field(field)
            p.set_lr(np.full(loops, 0.005, np.float32))
            p.run(loops, tol, checked, white_attention=1.0)
        ph, e, stats, iters = p.read()
    return ph, e, stats, iters, gi


def _probe(lib, batch, shape, expect, f64=False, algo=None):
    """The geometry a transform entry's engine gets under the current overrides:
    slm_fft2 builds a float32-target GS plan, slm_fft2_c128 a float64 GS engine
    of the same shape and batch, both through the plan's own selection."""
    with lib.Plan(lib.ALGO_GS if algo is None else algo, batch, shape[0], shape[1], lib.TGT_F32, False, 1) as p:
        if f64:
            p.set_precision(lib.PRECISION_F64)
        gi = p.generic_info()
    _check_info(gi, expect)
    return gi


def _expected_out(e, t, stats, loops):
    return e.astype(np.float64) * (float(np.max(t)) / stats[loops - 1, 0])


# ---------------------------------------------------------------------------
# mixed-radix tiles
# ---------------------------------------------------------------------------
# (45, 77) = 3^2 5 x 7 11: the kernels built with the odd radices 7, 11, 13;
# (50, 54) = 2 5^2 x 2 3^3: the small-radix kernels. Both widths are ragged for
# 4-, 8- and 16-column tiles (77 for 2 as well), both heights leave a tail row
# tile for 4 and 7 rows; the largest tile, H x W, is 3465 elements (kTileElems 4608).
MR_SHAPES = [(45, 77), (50, 54)]
RPWS = (1, 2, 4, 7, "H")
CWS = (1, 2, 4, 8, 16)
RAGGED = [(2, 2), (4, 8), (7, 16), ("H", 4)]


def _mr_force(knobs, shape, rpw, cw):
    rpw = shape[0] if rpw == "H" else rpw
    knobs(SLM_GENERIC_ENGINE="mr", SLM_MR_RPW=rpw, SLM_MR_CW=cw)
    return {"engine": "mixed-radix", "precision": "f64", "rows_per_tile": rpw, "cols_per_tile": cw,
            "col_workgroups": -(-shape[1] // cw)}


@pytest.mark.gpu
@pytest.mark.parametrize("rpw", RPWS)
@pytest.mark.parametrize("shape", MR_SHAPES)
def test_mr_tiles_transforms(gpu, knobs, shape, rpw):
    """slm_fft2_c128 and slm_fft2, forward and inverse, two holograms, on every
    rows-per-tile x columns-per-tile geometry: numpy.fft at 1e-13 (complex128)
    and 1e-6 (the complex64 entry), and bit for bit the one-row / one-column
    geometry's result."""
    xz, xc = _x(shape, np.complex128), _x(shape, np.complex64)
    _mr_force(knobs, shape, 1, 1)
    base = {(f, inv): f(x, inverse=inv) for f, x in ((gpu.fft2_c128, xz), (gpu.fft2, xc)) for inv in (False, True)}
    worst = 0.0
    for cw in CWS:
        expect = _mr_force(knobs, shape, rpw, cw)
        _probe(gpu, 2, shape, expect)
        for (f, inv), ref in base.items():
            z = f is gpu.fft2_c128
            got = f(xz if z else xc, inverse=inv)
            err = _max_err(got, _fft_ref(shape, np.complex128 if z else np.complex64, inv))
            assert err < (1e-13 if z else 1e-6), (shape, rpw, cw, z, inv, err)
            worst = max(worst, float(np.max(np.abs(got - ref))))
            np.testing.assert_array_equal(got, ref, err_msg=f"{shape} rpw {rpw} cw {cw} c128 {z} inverse {inv}")
    print(f"[geometry] mixed-radix transforms {shape} rpw {rpw}: largest difference to (1, 1) {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("with_ain", [False, True])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("shape", MR_SHAPES)
def test_mr_tiles_gs_warm_start(gpu, knobs, shape, u8, with_ain):
    """GS warm start (30 + 40) on multi-row tiles with a tail and ragged
    multi-column tiles, with and without a non-uniform a_in (the row passes
    read it at pix0 + e of the tile), at the float64 engines' bars; phases bit
    for bit the (1, 1) geometry's, errors at rtol 1e-12 (the partial sums
    regroup per column tile)."""
    loops = 40
    t, ain, phi30, ref, ref_e, ref_err = _gs_warm_ref(shape, u8, with_ain, loops, 1)
    ph1, e1, st1, _, _ = _run(gpu, gpu.ALGO_GS, t[None], loops, _mr_force(knobs, shape, 1, 1), phase=phi30[None],
                              ain=ain)
    worst_rms = worst_curve = 0.0
    for rpw, cw in RAGGED:
        ph, e, st, iters, _ = _run(gpu, gpu.ALGO_GS, t[None], loops, _mr_force(knobs, shape, rpw, cw),
                                   phase=phi30[None], ain=ain)
        rms = orc.phase_rms(ph[0], ref)
        curve = float(np.max(np.abs(st[0, :loops, 3] / ref_err - 1)))
        worst_rms, worst_curve = max(worst_rms, rms), max(worst_curve, curve)
        assert rms < 1e-6, (rpw, cw, rms)
        np.testing.assert_allclose(st[0, :loops, 3], ref_err, rtol=1e-6)
        np.testing.assert_allclose(_expected_out(e[0], t, st[0], loops), ref_e, rtol=1e-6,
                                   atol=1e-6 * float(np.max(ref_e)))
        assert (iters == -1).all()
        np.testing.assert_array_equal(ph, ph1, err_msg=f"rpw {rpw} cw {cw}")
        np.testing.assert_array_equal(e, e1, err_msg=f"rpw {rpw} cw {cw}")
        np.testing.assert_allclose(st[..., 3], st1[..., 3], rtol=1e-12)
    print(f"[geometry] mixed-radix GS warm {shape} {'u8' if u8 else 'f32'} a_in {with_ain}: worst phase rms "
          f"{worst_rms:.3e}, curve {worst_curve:.3e}; phases bitwise equal to (1, 1)")


@pytest.mark.gpu
@pytest.mark.parametrize("with_ain", [False, True])
@pytest.mark.parametrize("shape", MR_SHAPES)
def test_mr_tiles_gs_cold_start(gpu, knobs, shape, with_ain):
    """The cold start (CO_AMP_INV on a ragged column tile, RO_COLD on a tail
    row tile): the first three errors pointwise at rtol 1e-6 as
    test_generic_gs_cold_start (chaotic at rounding level later),
    the whole run bit for bit the (1, 1) geometry's.

    With a non-uniform a_in the start is no longer symmetric and rounding
    grows from the first iteration: the oracle itself, started from another
    float32 or a float64 transform of sqrt(T), moves its first error by
    <= 4e-8 but its second and third by up to 9.5e-7 at these shapes (CPU
    check; 4.6e-6 at 120 x 90). Those two are held at 1e-5, ten times that --
    a misplaced a_in would show at order one."""
    t = _target(shape, True, 3)
    ain, inten = _ain(shape) if with_ain else (None, None)
    _, _, ref_err = orc.gerchberg_saxton_faithful(t, 40, incoming_intensity=inten)
    ph1, _, st1, _, _ = _run(gpu, gpu.ALGO_GS, t[None], 40, _mr_force(knobs, shape, 1, 1), ain=ain)
    ph, _, st, _, _ = _run(gpu, gpu.ALGO_GS, t[None], 40, _mr_force(knobs, shape, 4, 8), ain=ain)
    print(f"[geometry] mixed-radix GS cold {shape} a_in {with_ain} (4, 8): first errors "
          f"{np.abs(st[0, :3, 3] / ref_err[:3] - 1)}")
    np.testing.assert_allclose(st[0, :1, 3], ref_err[:1], rtol=1e-6)
    np.testing.assert_allclose(st[0, 1:3, 3], ref_err[1:3], rtol=1e-5 if with_ain else 1e-6)
    np.testing.assert_array_equal(ph, ph1)
    np.testing.assert_allclose(st[..., 3], st1[..., 3], rtol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["field", "field-ain", "u8"])
@pytest.mark.parametrize("shape", MR_SHAPES)
def test_mr_tiles_gd(gpu, knobs, shape, case):
    """GD, 40 iterations from the host-set field (float32 target without and
    with a_in, uint8 target) at two ragged geometries: the bars of a complex64
    field crossing the C-ABI; phases bit for bit the (1, 1) geometry's (the
    normalisation uses the maximum, which regrouping leaves exact)."""
    loops = 40
    t, ain, x0, ref, ref_err = _gd_ref(shape, case == "u8", case == "field-ain", loops, 5)
    ph1, _, st1, _, _ = _run(gpu, gpu.ALGO_GD, t[None], loops, _mr_force(knobs, shape, 1, 1), field=x0[None],
                             ain=ain)
    for rpw, cw in [(4, 8), (7, 16)]:
        ph, _, st, _, _ = _run(gpu, gpu.ALGO_GD, t[None], loops, _mr_force(knobs, shape, rpw, cw), field=x0[None],
                               ain=ain)
        rms = orc.phase_rms(ph[0], ref)
        print(f"[geometry] mixed-radix GD {shape} {case} ({rpw}, {cw}): phase rms {rms:.3e}, curve "
              f"{float(np.max(np.abs(st[0, :loops, 3] / ref_err - 1))):.3e}")
        assert rms < 1e-5
        np.testing.assert_allclose(st[0, :loops, 3], ref_err, rtol=1e-5)
        np.testing.assert_array_equal(ph, ph1, err_msg=f"rpw {rpw} cw {cw}")
        np.testing.assert_allclose(st[..., 3], st1[..., 3], rtol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MR_SHAPES)
def test_mr_tiles_gd_fourier_guess(gpu, knobs, shape):
    """GD from the device-formed "fourier" guess (CO_AMP_INV + RO_GD_FOURIER)
    at two ragged geometries. That start is Hermitian-symmetric and the run
    chaotic at rounding level (test_gd_fourier_guess_on_the_complex128_engines):
    the oracle itself, started from a float64 instead of scipy's float32
    transform of sqrt(T), ends 40 iterations 0.04 rad (45 x 77) and 0.36 rad
    (50 x 54) rms away and moves its own phase after one iteration by 5.6e-7
    and 2.0e-6 (CPU check; the device forms the guess from its float64
    transform). So the phase is held pointwise after one iteration, at GD's
    1e-5 bar, the first errors at rtol 1e-6, the last error in a band -- and
    all 40 iterations bit for bit to the (1, 1) geometry."""
    loops = 40
    t, ref1, ref_err = _gd_fourier_ref(shape, loops, 5)
    ph1, _, st1, _, _ = _run(gpu, gpu.ALGO_GD, t[None], loops, _mr_force(knobs, shape, 1, 1))
    for rpw, cw in [(4, 8), (7, 16)]:
        expect = _mr_force(knobs, shape, rpw, cw)
        first, _, _, _, _ = _run(gpu, gpu.ALGO_GD, t[None], 1, expect)
        rms1 = orc.phase_rms(first[0], ref1)
        ph, _, st, _, _ = _run(gpu, gpu.ALGO_GD, t[None], loops, expect)
        print(f"[geometry] mixed-radix GD {shape} fourier ({rpw}, {cw}): phase rms {rms1:.3e} after 1 iteration, "
              f"first errors {float(np.max(np.abs(st[0, :3, 3] / ref_err[:3] - 1))):.3e}")
        assert rms1 < 1e-5
        np.testing.assert_allclose(st[0, :3, 3], ref_err[:3], rtol=1e-6)
        assert 0.5 < st[0, loops - 1, 3] / ref_err[-1] < 2.0
        np.testing.assert_array_equal(ph, ph1, err_msg=f"rpw {rpw} cw {cw}")
        np.testing.assert_allclose(st[..., 3], st1[..., 3], rtol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MR_SHAPES)
def test_mr_tiles_batch(gpu, knobs, shape):
    """Different targets in one plan at a ragged geometry (tile id -> hologram
    id / tiles, tile id % tiles): every hologram equals its single-hologram
    run bit for bit, GS (warm start, with a_in) and GD."""
    seeds = (1, 7, 8)
    expect = _mr_force(knobs, shape, 7, 16)
    refs = [_gs_warm_ref(shape, False, True, 40, s) for s in seeds]
    ain = refs[0][1]
    t, phi = np.stack([r[0] for r in refs]), np.stack([r[2] for r in refs])
    ph, e, st, _, _ = _run(gpu, gpu.ALGO_GS, t, 40, expect, phase=phi, ain=ain)
    for k in range(len(seeds)):
        ph_k, e_k, st_k, _, _ = _run(gpu, gpu.ALGO_GS, t[k:k + 1], 40, expect, phase=phi[k:k + 1], ain=ain)
        np.testing.assert_array_equal(ph[k], ph_k[0])
        np.testing.assert_array_equal(e[k], e_k[0])
        np.testing.assert_array_equal(st[k], st_k[0])
        assert orc.phase_rms(ph[k], refs[k][3]) < 1e-6
    gd = [_gd_ref(shape, False, False, 40, s) for s in (5, 6, 9)]
    t, x0 = np.stack([r[0] for r in gd]), np.stack([r[2] for r in gd])
    ph, e, st, _, _ = _run(gpu, gpu.ALGO_GD, t, 40, expect, field=x0)
    for k in range(len(gd)):
        ph_k, e_k, st_k, _, _ = _run(gpu, gpu.ALGO_GD, t[k:k + 1], 40, expect, field=x0[k:k + 1])
        np.testing.assert_array_equal(ph[k], ph_k[0])
        np.testing.assert_array_equal(e[k], e_k[0])
        np.testing.assert_array_equal(st[k], st_k[0])
        assert orc.phase_rms(ph[k], gd[k][3]) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MR_SHAPES)
def test_mr_tiles_tolerance_stop(gpu, knobs, shape):
    """test_generic_tolerance_stop at a ragged geometry: of two holograms the
    first (a dim target: its errors are a tenth of the other's) stops early;
    its iteration count, frozen phase and expected output equal an unchecked
    run of that many iterations (the same kernels on the same inputs: bit for
    bit), its statistics at rtol 1e-10; the oracle stops at the same
    iteration. The runs start from a random phase: the cold start's error
    curve stays on a plateau for the first iterations."""
    expect = _mr_force(knobs, shape, 4, 8)
    t = np.stack([_target(shape, False, 7) * np.float32(0.3), _target(shape, False, 8)])
    phi = np.random.default_rng(3).uniform(-np.pi, np.pi, t.shape).astype(np.float32)
    loops = 20
    _, _, full, _, _ = _run(gpu, gpu.ALGO_GS, t, loops, expect, phase=phi)
    tol = float(np.sqrt(full[0, 7, 3] * full[0, 8, 3]))
    stop0 = int(np.argmax(~(full[0, :loops, 3] > tol)))
    assert stop0 == 8 and (full[1, :loops, 3] > tol).all()  # hologram 1 keeps going
    ph, e, st, it, _ = _run(gpu, gpu.ALGO_GS, t, loops, expect, phase=phi, tol=tol, checked=True)
    assert it[0] == stop0 + 1 and it[1] in (-1, loops)
    ph0, e0, st0, _, _ = _run(gpu, gpu.ALGO_GS, t[:1], stop0 + 1, expect, phase=phi[:1])
    np.testing.assert_array_equal(ph[0], ph0[0])
    np.testing.assert_array_equal(e[0], e0[0])
    np.testing.assert_allclose(st[0, :stop0 + 1], st0[0, :stop0 + 1], rtol=1e-10)
    np.testing.assert_allclose(st[1, :loops], full[1, :loops], rtol=1e-10)
    _, _, ref_err = orc.gerchberg_saxton_faithful(t[0], loops, tolerance=tol, initial_phase=phi[0])
    assert len(ref_err) == stop0 + 1
    np.testing.assert_allclose(st[0, :stop0 + 1, 3], ref_err, rtol=1e-6)


# ---------------------------------------------------------------------------
# slm_fft2_c128's engine cache
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_fft2_c128_cache_honours_the_engine_overrides(gpu, knobs):
    """One shape through slm_fft2_c128 on the chirp-z line transforms, then on
    the mixed radix with the first engine still cached: each call runs the
    back end its environment asks for. Both match numpy.fft -- the direct
    transform at 1e-13; chirp-z (two transforms of a length M <= 160 and three
    point-wise products per line, the table of FFT(b) summed over M terms on
    the host: <= ~M eps = 2e-14 per line in the worst case) at 1e-12 -- and
    round differently, so a reused engine would show as bitwise-equal results."""
    shape = (45, 77)
    x = _x(shape, np.complex128)
    want = _fft_ref(shape, np.complex128, False)
    knobs(SLM_GENERIC_ENGINE="bluestein")
    _probe(gpu, 2, shape, {"engine": "bluestein"})
    cz = gpu.fft2_c128(x)
    knobs(SLM_GENERIC_ENGINE="mr")
    _probe(gpu, 2, shape, {"engine": "mixed-radix"})
    mr = gpu.fft2_c128(x)
    print(f"[geometry] fft2_c128 {shape}: chirp-z error {_max_err(cz, want):.3e}, mixed radix {_max_err(mr, want):.3e}")
    assert _max_err(cz, want) < 1e-12
    assert _max_err(mr, want) < 1e-13
    assert not np.array_equal(cz, mr)
    # and back: the first engine's entry is found again, not the newer one
    knobs(SLM_GENERIC_ENGINE="bluestein")
    np.testing.assert_array_equal(gpu.fft2_c128(x), cz)


# ---------------------------------------------------------------------------
# radix-plan back end
# ---------------------------------------------------------------------------
def _rz_expect(shape, row, col, cw, layout, engine="radix-c128"):
    return {"engine": engine, "precision": "f64" if engine == "radix-c128" else "f32",
            "row_plan": KEY[(shape[1], row)], "col_plan": KEY[(shape[0], col)], "cols_per_tile": cw,
            "layout": layout, "col_workgroups": shape[1] // cw}


# column tiles the build accepts at 256-point columns (rz_col_ok: 64 .. 1024
# threads per tile): 16-thread wide lines in tiles of 4 and 8, 32-thread narrow
# lines in tiles of 2, 4 and 8; no single-column tile
C128_COLS = [("wide", 4), ("wide", 8), ("narrow", 2), ("narrow", 4), ("narrow", 8)]
# covering subset for the GS / GD runs: every row variant, column variant,
# tile width and layout occurs under both
C128_COVER = [("wide", "wide", 4, "b2"), ("wide", "wide", 8, "rm"), ("narrow", "narrow", 2, "b2"),
              ("narrow", "narrow", 4, "rm"), ("wide", "narrow", 8, "b2"), ("narrow", "wide", 4, "rm"),
              ("wide", "narrow", 2, "rm"), ("narrow", "wide", 8, "b2")]
C128_SHAPE = (256, 512)


def _rz_force(knobs, row, col, cw, layout):
    knobs(SLM_RZ_ROW_PLAN=row, SLM_RZ_COL_PLAN=col, SLM_RZ_CW=cw, SLM_RZ_LAYOUT=layout)


@pytest.mark.gpu
@pytest.mark.parametrize("col", ["wide", "narrow"])
@pytest.mark.parametrize("row", ["wide", "narrow"])
def test_rz_c128_variants_transforms(gpu, knobs, row, col):
    """slm_fft2_c128 at 256 x 512 under $SLM_ENGINE=float64 on each row plan x
    column plan x accepted column-tile width x state layout."""
    knobs(SLM_ENGINE="float64")
    x = _x(C128_SHAPE, np.complex128)
    worst = 0.0
    for c, cw in C128_COLS:
        if c != col:
            continue
        for layout in ("rm", "b2"):
            _rz_force(knobs, row, col, cw, layout)
            _probe(gpu, 2, C128_SHAPE, _rz_expect(C128_SHAPE, row, col, cw, layout))
            for inverse in (False, True):
                err = _max_err(gpu.fft2_c128(x, inverse=inverse), _fft_ref(C128_SHAPE, np.complex128, inverse))
                worst = max(worst, err)
                assert err < 1e-13, (row, col, cw, layout, inverse, err)
    print(f"[geometry] radix-c128 fft2_c128 {C128_SHAPE} rows {row} columns {col}: worst error {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("row,col,cw,layout", C128_COVER)
def test_rz_c128_variants_gs(gpu, knobs, row, col, cw, layout):
    """GS warm start (30 + 40), uint8 and float32 targets, with and without
    a_in, on the covering subset, at test_gpu_radix_c128.py's bars."""
    knobs(SLM_ENGINE="float64")
    _rz_force(knobs, row, col, cw, layout)
    expect = _rz_expect(C128_SHAPE, row, col, cw, layout)
    loops = 40
    for u8 in (False, True):
        for with_ain in (False, True):
            t, ain, phi30, ref, ref_e, ref_err = _gs_warm_ref(C128_SHAPE, u8, with_ain, loops, 256)
            ph, e, st, iters, _ = _run(gpu, gpu.ALGO_GS, t[None], loops, expect, phase=phi30[None], ain=ain)
            rms = orc.phase_rms(ph[0], ref)
            print(f"[geometry] radix-c128 GS {C128_SHAPE} {row}/{col}/{cw}/{layout} {'u8' if u8 else 'f32'} a_in "
                  f"{with_ain}: phase rms {rms:.3e}, curve {float(np.max(np.abs(st[0, :loops, 3] / ref_err - 1))):.3e}")
            assert rms < 1e-6
            np.testing.assert_allclose(st[0, :loops, 3], ref_err, rtol=1e-6)
            np.testing.assert_allclose(_expected_out(e[0], t, st[0], loops), ref_e, rtol=1e-6,
                                       atol=1e-6 * float(np.max(ref_e)))
            assert (iters == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("row,col,cw,layout", C128_COVER)
def test_rz_c128_variants_gd(gpu, knobs, row, col, cw, layout):
    """GD, 40 iterations from the host-set random guess (float32 target; uint8
    target with a_in), on the covering subset, at test_gpu_radix_c128.py's bars."""
    knobs(SLM_ENGINE="float64")
    _rz_force(knobs, row, col, cw, layout)
    expect = _rz_expect(C128_SHAPE, row, col, cw, layout)
    loops = 40
    for u8, with_ain in ((False, False), (True, True)):
        t, ain, x0, ref, ref_err = _gd_ref(C128_SHAPE, u8, with_ain, loops, 5)
        ph, _, st, _, _ = _run(gpu, gpu.ALGO_GD, t[None], loops, expect, field=x0[None], ain=ain)
        rms = orc.phase_rms(ph[0], ref)
        print(f"[geometry] radix-c128 GD {C128_SHAPE} {row}/{col}/{cw}/{layout} {'u8' if u8 else 'f32'} a_in "
              f"{with_ain}: phase rms {rms:.3e}, curve {float(np.max(np.abs(st[0, :loops, 3] / ref_err - 1))):.3e}")
        assert rms < 1e-5  # the field crosses the C-ABI as complex64
        np.testing.assert_allclose(st[0, :loops, 3], ref_err, rtol=1e-5)


def _gs_c128_case(gpu, shape, expect, loops, tag, seed=4096):
    t, _, phi30, ref, ref_e, ref_err = _gs_warm_ref(shape, False, False, loops, seed)
    ph, e, st, _, _ = _run(gpu, gpu.ALGO_GS, t[None], loops, expect, phase=phi30[None])
    rms = orc.phase_rms(ph[0], ref)
    print(f"[geometry] {tag}: phase rms {rms:.3e}, curve {float(np.max(np.abs(st[0, :loops, 3] / ref_err - 1))):.3e}")
    assert rms < 1e-6
    np.testing.assert_allclose(st[0, :loops, 3], ref_err, rtol=1e-6)
    np.testing.assert_allclose(_expected_out(e[0], t, st[0], loops), ref_e, rtol=1e-6, atol=1e-6 * float(np.max(ref_e)))


@pytest.mark.gpu
@pytest.mark.parametrize("col", ["e8", "narrow"])
def test_rz_4096_point_columns(gpu, knobs, col):
    """4096-point columns (4096 x 64) on the E = 8 plan the engine always
    picks there and on the narrow one, in one- and two-column tiles (all the
    build accepts: four columns exceed a workgroup); GS plans with a
    4096-point side default to the row-major state. Transforms on each, one
    GS warm start (30 + 20) per column plan."""
    shape = (4096, 64)
    knobs(SLM_ENGINE="float64", SLM_RZ_COL_PLAN=col)
    x = _x(shape, np.complex128)[:1]
    for cw in (1, 2):
        knobs(SLM_RZ_CW=cw)
        expect = _rz_expect(shape, "wide", col, cw, "rm")
        _probe(gpu, 1, shape, expect)
        for inverse in (False, True):
            err = _max_err(gpu.fft2_c128(x, inverse=inverse), _fft_ref(shape, np.complex128, inverse)[:1])
            print(f"[geometry] radix-c128 fft2_c128 {shape} columns {col} cw {cw} inverse {inverse}: error {err:.3e}")
            assert err < 1e-13, (col, cw, inverse, err)
    _gs_c128_case(gpu, shape, expect, 20, f"radix-c128 GS {shape} columns {col} cw 2 warm 30+20")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["rm", "b2"])
def test_rz_4096_point_rows(gpu, knobs, layout):
    """4096-point rows (64 x 4096) on both state layouts: transforms."""
    shape = (64, 4096)
    knobs(SLM_ENGINE="float64", SLM_RZ_LAYOUT=layout)
    expect = _rz_expect(shape, "narrow", "wide", 8, layout)
    _probe(gpu, 1, shape, expect)
    x = _x(shape, np.complex128)[:1]
    for inverse in (False, True):
        err = _max_err(gpu.fft2_c128(x, inverse=inverse), _fft_ref(shape, np.complex128, inverse)[:1])
        print(f"[geometry] radix-c128 fft2_c128 {shape} layout {layout} inverse {inverse}: error {err:.3e}")
        assert err < 1e-13, (layout, inverse, err)


# complex64 kernels (float32 GS by default where one side is a 13-smooth panel
# length): the 2^k side's variant and the column-tile width. Three of the eight
# combinations have no kernel and fall back to the float64 mixed radix, which
# generic_info shows: 16-thread wide 256-point columns in tiles of 2 are half a
# wave (rz_col_ok wants 64 threads), and wide 256-point rows come 16 to a
# workgroup, which does not divide 600 rows.
C64_CASES = [((256, 600), "wide", 2, False), ((256, 600), "wide", 4, True), ((256, 600), "narrow", 2, True),
             ((256, 600), "narrow", 4, True), ((600, 256), "wide", 2, False), ((600, 256), "wide", 4, False),
             ((600, 256), "narrow", 2, True), ((600, 256), "narrow", 4, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,plan,cw,built", C64_CASES)
def test_rz_c64_variants(gpu, knobs, shape, plan, cw, built):
    """slm_fft2 and a GS warm start (30 + 40) at test_gpu_radix_c64.py's bars
    on each variant of the 2^k side and column-tile width."""
    knobs(SLM_RZ_PLAN=plan, SLM_RZ_CW=cw)
    if built:
        expect = _rz_expect(shape, plan if shape[1] == 256 else "main", plan if shape[0] == 256 else "main", cw,
                            "b2", engine="radix-c64")
    else:
        expect = {"engine": "mixed-radix", "precision": "f64"}
    _probe(gpu, 2, shape, expect)
    x = _x(shape, np.complex64)
    for inverse in (False, True):
        got, want = gpu.fft2(x, inverse=inverse), _fft_ref(shape, np.complex64, inverse)
        err = float(np.sqrt(np.mean(np.abs(got - want) ** 2) / np.mean(np.abs(want) ** 2)))
        print(f"[geometry] {expect['engine']} fft2 {shape} {plan} cw {cw} inverse {inverse}: rel rms {err:.3e}, "
              f"max {_max_err(got, want):.3e}")
        assert err < 1e-6, (shape, plan, cw, inverse, err)
    loops = 40
    t, _, phi30, ref, ref_e, ref_err = _gs_warm_ref(shape, False, False, loops, 600)
    ph, e, st, _, _ = _run(gpu, gpu.ALGO_GS, t[None], loops, expect, phase=phi30[None])
    rms = orc.phase_rms(ph[0], ref)
    print(f"[geometry] {expect['engine']} GS {shape} {plan} cw {cw} warm 30+40: phase rms {rms:.3e}, curve "
          f"{float(np.max(np.abs(st[0, :loops, 3] / ref_err - 1))):.3e}")
    assert rms < 1e-5
    np.testing.assert_allclose(st[0, :loops, 3], ref_err, rtol=1e-4)
    np.testing.assert_allclose(_expected_out(e[0], t, st[0], loops), ref_e, rtol=1e-3, atol=1e-4 * float(np.max(ref_e)))


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("shape", [(64, 1920), (1920, 64)])
def test_rz_panel_plans(gpu, knobs, shape, f64):
    """Both 1920-point plans ($SLM_RZ_PANEL=main: 15.16.8, alt: 8.16.15) on
    rows (64 x 1920) and on columns (1920 x 64), at float32 (float32 target)
    and at float64 (uint8 target): a transform and a GS warm start (30 + 40)
    each; the plan key of the 1920-point axis differs between the two.
    64-point columns have 8 threads, below the complex64 kernels' 2- and
    4-column tiles: 64 x 1920 runs the complex128 kernels at either precision."""
    rows = shape[1] == 1920
    c64 = not f64 and not rows
    loops = 40
    keys = {}
    for panel in ("main", "alt"):
        knobs(SLM_RZ_PANEL=panel)
        expect = _rz_expect(shape, panel if rows else "wide", "wide" if rows else panel, 8 if rows else 2, "b2",
                            engine="radix-c64" if c64 else "radix-c128")
        t, _, phi30, ref, ref_e, ref_err = _gs_warm_ref(shape, f64, False, loops, 1920)
        ph, e, st, _, gi = _run(gpu, gpu.ALGO_GS, t[None], loops, expect, phase=phi30[None])
        keys[panel] = gi["row_plan" if rows else "col_plan"]
        rms = orc.phase_rms(ph[0], ref)
        print(f"[geometry] {gi['engine']} GS {shape} panel {panel} {'u8' if f64 else 'f32'} warm 30+40: phase rms "
              f"{rms:.3e}, curve {float(np.max(np.abs(st[0, :loops, 3] / ref_err - 1))):.3e}")
        # the bars of the precision the plan reports
        assert rms < (1e-5 if c64 else 1e-6)
        np.testing.assert_allclose(st[0, :loops, 3], ref_err, rtol=1e-4 if c64 else 1e-6)
        np.testing.assert_allclose(_expected_out(e[0], t, st[0], loops), ref_e, rtol=1e-3 if c64 else 1e-6,
                                   atol=(1e-4 if c64 else 1e-6) * float(np.max(ref_e)))
        for inverse in (False, True):
            if f64:
                _probe(gpu, 2, shape, dict(expect, engine="radix-c128", precision="f64"), f64=True)
                err = _max_err(gpu.fft2_c128(_x(shape, np.complex128), inverse=inverse),
                               _fft_ref(shape, np.complex128, inverse))
                assert err < 1e-13, (shape, panel, inverse, err)
            else:
                _probe(gpu, 2, shape, expect)
                got, want = gpu.fft2(_x(shape, np.complex64), inverse=inverse), _fft_ref(shape, np.complex64, inverse)
                err = float(np.sqrt(np.mean(np.abs(got - want) ** 2) / np.mean(np.abs(want) ** 2)))
                assert err < 1e-6, (shape, panel, inverse, err)
            print(f"[geometry] {gi['engine']} transform {shape} panel {panel} inverse {inverse}: error {err:.3e}")
    assert keys["main"] != keys["alt"], keys


# ---------------------------------------------------------------------------
# chirp-z length limit
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_chirp_z_longest_line(gpu, knobs):
    """4093 (prime) transforms by chirp-z over M = 8192 points: exactly one
    workgroup's 128 KiB of LDS, the longest line the engine takes."""
    shape = (4093, 2)
    with gpu.Plan(gpu.ALGO_GS, 1, shape[0], shape[1], gpu.TGT_F32, False, 1) as p:
        assert p.generic_info()["engine"] == "bluestein"
    xc, xz = _x(shape, np.complex64), _x(shape, np.complex128)
    for inverse in (False, True):
        err = _max_err(gpu.fft2(xc, inverse=inverse), _fft_ref(shape, np.complex64, inverse))
        errz = _max_err(gpu.fft2_c128(xz, inverse=inverse), _fft_ref(shape, np.complex128, inverse))
        print(f"[geometry] chirp-z {shape} inverse {inverse}: fft2 error {err:.3e}, fft2_c128 error {errz:.3e}")
        assert err < 1e-6, (inverse, err)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4099, 2), (2, 8200)])
def test_sides_past_the_chirp_z_limit_are_refused(gpu, knobs, shape):
    """A side over 4096 with a prime factor above 13 (4099 is prime), or any
    side over 8192, does not fit a workgroup's line: refused with the limit
    in the message, by the library and by the drop-in's shape check."""
    from spatial_light_modulator_module_amd import algorithms as alg

    for call in (lambda: gpu.fft2(np.zeros(shape, np.complex64)), lambda: gpu.fft2_c128(np.zeros(shape, np.complex128)),
                 lambda: gpu.Plan(gpu.ALGO_GS, 1, shape[0], shape[1], gpu.TGT_F32, False, 1)):
        with pytest.raises(gpu.SlmError, match=r"over 4096 with a prime factor above 13.*over\s+8192"):
            call()
    with pytest.raises(ValueError, match=r"over 4096 with a prime factor above 13.*over 8192"):
        alg._check_shape(np.zeros(shape))


@pytest.mark.gpu
def test_generic_info_refuses_a_fused_engine_plan(gpu, knobs):
    """slm_plan_generic_info describes any-size plans only; slm_plan_info keeps
    its values for them (0 / 1 / -1: bench.py and the tools read those)."""
    with gpu.Plan(gpu.ALGO_GS, 1, 64, 128, gpu.TGT_F32, False, 1) as p:
        assert p.engine()[0] in ("stockham", "shuffle")
        with pytest.raises(gpu.SlmError, match="not an any-size plan"):
            p.generic_info()
    knobs(SLM_GENERIC_ENGINE="mr", SLM_MR_RPW=4, SLM_MR_CW=8)
    with gpu.Plan(gpu.ALGO_GS, 1, 45, 77, gpu.TGT_F32, False, 1) as p:
        info = p.info()
        assert (info["col_cw"], info["rows_per_workgroup"], info["row_plan"], info["col_plan"]) == (0, 1, -1, -1)
        assert p.generic_info()["rows_per_tile"] == 4 and p.generic_info()["cols_per_tile"] == 8
