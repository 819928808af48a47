"""Early-stop paths, the one-shot C-ABI entry points and asynchronous reruns.

* ``while error > tolerance`` stopping at an odd iteration (GD keeps X of
  iteration i in buffer i % 2: the expected-output kernel then reads the
  ping-pong partner, kernels.hpp COL_EXPECTED) — src/algorithms.py:83;
* a GS batch whose holograms stop at different iterations under one
  tolerance: per-hologram stop flags must not leak between holograms
  (src/generate_hologram_sequence.py runs each frame with the same -tol);
* slm_gs / slm_gd called exactly as INTEGRATION.md binds them;
* slm_plan_run issued back to back with different loop counts and no read in
  between (the cached graph is re-captured while a replay may be queued).
"""
import argparse
import ctypes

import numpy as np
import pytest

from oracle import goldens
from oracle import gs_gd_oracle as orc


def gd_args(**kw):
    base = dict(incomming_intensity="uniform", tolerance=0.0, max_loops=12, gif=False, print_info=False,
                plot_error=False, learning_rate=0.005, white_attention=1.0, unsettle=0, initial_guess="random",
                random_seed=5)
    base.update(kw)
    return argparse.Namespace(**base)


def _tol_between(err, s):
    """A tolerance with err[i] > tol for i < s and err[s] <= tol (geometric midpoint)."""
    err = np.asarray(err)
    assert np.all(np.diff(err[: s + 1]) < 0), "error curve must decrease up to the stop"
    return float(np.sqrt(err[s - 1] * err[s]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 1024])
def test_gd_tolerance_stop_at_odd_iteration(gpu, n):
    """n = 1024: the configs[2] plan (narrow layout pair; a checked run takes
    the two-launch column side, an unchecked one the fused side)."""
    from spatial_light_modulator_module_amd.algorithms import gradient_descent

    rng = np.random.default_rng(21)
    t = rng.uniform(0, 255, (n, n)).astype(np.float32)
    _, _, err_full, _ = orc.gradient_descent_faithful(t, 12, 0.005, 1.0, 0, random_seed=5)
    tol = _tol_between(err_full, 5)  # stops after iteration index 5 (odd): 6 iterations
    ph_o, out_o, err_o, _ = orc.gradient_descent_faithful(t, 12, 0.005, 1.0, 0, tolerance=tol, random_seed=5)
    assert len(err_o) == 6
    holo, out, err = gradient_descent(t, gd_args(tolerance=tol))
    assert len(err) == 6
    np.testing.assert_allclose(err, err_o, rtol=1e-4)
    assert orc.phase_rms(holo, ph_o) < 1e-5
    np.testing.assert_allclose(out, out_o, rtol=1e-3, atol=1e-3 * float(t.max()))


@pytest.mark.gpu
def test_gs_4096_batch_with_different_stop_iterations(gpu):
    """The float32 4096 row kernels carry two rows per thread (r04): a checked
    run whose two holograms stop after 3 and 5 iterations (tiles of a stopped
    hologram leave before their exchanges) against the threaded float64
    restatement with the same tolerance."""
    from oracle import fast_f64
    from spatial_light_modulator_module_amd import algorithms as alg

    n = 4096
    rng = np.random.default_rng(34)
    base = rng.uniform(0, 255, (n, n))
    phi0 = rng.uniform(-np.pi, np.pi, base.shape).astype(np.float32)
    _, _, err_base = fast_f64.gerchberg_saxton_f64(base.astype(np.float32), 8, initial_phase=phi0)
    tol = 1000.0
    stops = (2, 4)
    scales = [np.sqrt(tol / _tol_between(err_base, s)) for s in stops]
    t = np.stack([(c * base).astype(np.float32) for c in scales])
    ph, _, errs, _, _ = alg.run_gs(t, 8, tol=tol, initial_phase=np.stack([phi0] * 2))
    for k, s in enumerate(stops):
        ref_ph, _, ref_err = fast_f64.gerchberg_saxton_f64(t[k], 8, initial_phase=phi0, tolerance=tol)
        assert len(errs[k]) == len(ref_err) == s + 1, (k, len(errs[k]), len(ref_err))
        np.testing.assert_allclose(errs[k], ref_err, rtol=1e-4)
        rms = orc.phase_rms(ph[k], ref_ph)
        print(f"[parity] GS 4096^2 checked batch, hologram {k} stops after {s + 1}: phase rms {rms:.3e}")
        assert rms < 1e-5
    alg.clear_plans()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [128, 1024])
def test_gs_batch_with_different_stop_iterations(gpu, n):
    """One tolerance, three holograms scaled so that each stops at a different
    iteration (2, 3 and 5): GS is scale free in the target, the error scales
    with its square. n = 1024 runs the checked (early-exit) wave-shuffle
    kernels: whole workgroups leave before the pair's barriers."""
    from spatial_light_modulator_module_amd import algorithms as alg

    rng = np.random.default_rng(33)
    base = rng.uniform(0, 255, (n, n))
    phi0 = rng.uniform(-np.pi, np.pi, base.shape).astype(np.float32)
    _, _, err_base = orc.gerchberg_saxton_faithful(base.astype(np.float32), 12, initial_phase=phi0)
    tol = 1000.0
    stops = (2, 3, 5)
    scales = [np.sqrt(tol / _tol_between(err_base, s)) for s in stops]
    t = np.stack([(c * base).astype(np.float32) for c in scales])
    phis = np.stack([phi0] * 3)
    ph, _, errs, _, _ = alg.run_gs(t, 12, tol=tol, initial_phase=phis)
    for k, s in enumerate(stops):
        ref_ph, _, ref_err = orc.gerchberg_saxton_faithful(t[k], 12, tolerance=tol, initial_phase=phi0)
        assert len(errs[k]) == len(ref_err) == s + 1, (k, len(errs[k]), len(ref_err))
        np.testing.assert_allclose(errs[k], ref_err, rtol=1e-4)
        assert orc.phase_rms(ph[k], ref_ph) < 1e-5
        p1, _, e1, _, _ = alg.run_gs(t[k:k + 1], 12, tol=tol, initial_phase=phis[k:k + 1])
        np.testing.assert_array_equal(p1[0], ph[k])
        assert e1[0] == errs[k]


# --- INTEGRATION.md section 2, verbatim apart from the library path -----------
def _integration_binding(path):
    _lib = ctypes.CDLL(path)
    _vp, _i, _d, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float
    _lib.slm_init.argtypes = [_i]
    _lib.slm_last_error.restype = ctypes.c_char_p
    _lib.slm_gs.argtypes = [_vp, _i, _vp, _i, _i, _i, _i, _d, _vp, _vp, _vp, _vp, _vp]
    _lib.slm_gd.argtypes = [_vp, _i, _vp, _i, _i, _i, _i, _d, _vp, _vp, _f, _vp, _vp, _vp, _vp]
    SLM_TGT_U8, SLM_TGT_F32 = 0, 1

    def _p(a):
        return None if a is None else a.ctypes.data

    def gerchberg_saxton_hip(demanded_output, max_loops, tolerance=0.0, incoming_amplitude=None, device=0):
        if _lib.slm_init(device) != 0:
            raise RuntimeError(_lib.slm_last_error().decode())
        t = np.ascontiguousarray(demanded_output)
        tt = SLM_TGT_U8 if t.dtype == np.uint8 else SLM_TGT_F32
        if tt == SLM_TGT_F32:
            t = t.astype(np.float32)
        h, w = t.shape
        ain = None if incoming_amplitude is None else np.ascontiguousarray(incoming_amplitude, np.float32)
        phase = np.empty((h, w), np.float32)
        expected = np.empty((h, w), np.float32)
        stats = np.empty((1, max_loops, 4), np.float64)
        iters = np.empty(1, np.int32)
        rc = _lib.slm_gs(_p(t), tt, _p(ain), 1, h, w, max_loops, tolerance, None,
                         _p(phase), _p(expected), _p(stats), _p(iters))
        if rc != 0:
            raise RuntimeError(_lib.slm_last_error().decode())
        n = max_loops if iters[0] < 0 else int(iters[0])
        return phase.astype(np.float64), expected, list(stats[0, :n, 3])

    def gradient_descent_hip(demanded_output, max_loops, learning_rates, white_attention, init_field,
                             tolerance=0.0, device=0):
        if _lib.slm_init(device) != 0:
            raise RuntimeError(_lib.slm_last_error().decode())
        t = np.ascontiguousarray(demanded_output)
        tt = SLM_TGT_U8 if t.dtype == np.uint8 else SLM_TGT_F32
        if tt == SLM_TGT_F32:
            t = t.astype(np.float32)
        h, w = t.shape
        x0 = None if init_field is None else np.ascontiguousarray(init_field, np.complex64).view(np.float32)
        lr = np.ascontiguousarray(learning_rates, np.float32)
        phase = np.empty((h, w), np.float32)
        expected = np.empty((h, w), np.float32)
        stats = np.empty((1, max_loops, 4), np.float64)
        iters = np.empty(1, np.int32)
        rc = _lib.slm_gd(_p(t), tt, None, 1, h, w, max_loops, tolerance, _p(x0), _p(lr), white_attention,
                         _p(phase), _p(expected), _p(stats), _p(iters))
        if rc != 0:
            raise RuntimeError(_lib.slm_last_error().decode())
        n = max_loops if iters[0] < 0 else int(iters[0])
        return phase.astype(np.float64), expected, list(stats[0, :n, 3])

    return gerchberg_saxton_hip, gradient_descent_hip


@pytest.mark.gpu
def test_one_shot_entry_points_as_integration_binds_them(gpu, golden_dir):
    from spatial_light_modulator_module_amd import _lib
    from spatial_light_modulator_module_amd import algorithms as alg

    gs_hip, gd_hip = _integration_binding(_lib.LIB_PATH)
    g = goldens.load(f"{golden_dir}/g1_gs_u8_256.npz")
    t = g["target"]
    # cold start: chaotic at rounding level, so the first errors are
    # compared with the reference and the rest with the plan API bit for bit
    phase, expected, err = gs_hip(t, 30)
    np.testing.assert_allclose(err[:3], g["err30"][:3], rtol=1e-4)
    ph_p, e_p, err_p, _, _ = alg.run_gs(t[None], 30)
    np.testing.assert_array_equal(phase, ph_p[0].astype(np.float64))
    np.testing.assert_array_equal(expected, e_p[0])
    assert err == err_p[0]
    g4 = goldens.load(f"{golden_dir}/g4_gd_f32_256.npz")
    t4 = g4["target"]
    x0 = alg.make_initial_guess("random", None, t4, 42)
    ph, _, err = gd_hip(t4, 100, np.full(100, 0.005), 1.0, x0)
    assert orc.phase_rms(ph, g4["phi100"]) < 1e-5
    np.testing.assert_allclose(err, g4["err100"], rtol=1e-4)
    tol = _tol_between(g4["err100"], 5)
    _, _, err_tol = gd_hip(t4, 100, np.full(100, 0.005), 1.0, x0, tolerance=tol)
    assert len(err_tol) == 6


@pytest.mark.gpu
def test_back_to_back_runs_without_reads(gpu):
    """run(5); run(9); run(5) with no synchronisation in between, then one read:
    the same bits as a fresh plan's run(5) (the cached graph exec is
    destroyed and re-captured while replays may still be queued)."""
    lib = gpu
    rng = np.random.default_rng(17)
    t = rng.uniform(0, 255, (2, 256, 256)).astype(np.float32)
    phi = rng.uniform(-np.pi, np.pi, t.shape).astype(np.float32)
    with lib.Plan(lib.ALGO_GS, 2, 256, 256, lib.TGT_F32, False, 16) as p:
        p.set_target(t)
        p.set_phase(phi)
        for loops in (5, 9, 5, 9, 5):
            p.run(loops)
        ph, e, stats, _ = p.read()
    with lib.Plan(lib.ALGO_GS, 2, 256, 256, lib.TGT_F32, False, 16) as q:
        q.set_target(t)
        q.set_phase(phi)
        q.run(5)
        ph1, e1, stats1, _ = q.read()
    np.testing.assert_array_equal(ph, ph1)
    np.testing.assert_array_equal(e, e1)
    np.testing.assert_array_equal(stats[:, :5], stats1[:, :5])
