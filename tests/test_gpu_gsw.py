"""Weighted Gerchberg-Saxton (SLM_ALGO_GSW) on the MI355X against the float64
NumPy reference of its definition (tests/gsw_reference.py). GSW has no
counterpart in the reference project; feedback = 0 must be plain GS bit for bit.

Parity runs from a warm start (30 reference iterations, 10 for the two large
shapes) as the GS parity tests do: the reference's phase and weights, rounded to
the float32 the plan takes, go to both sides, which then run the same further
iterations. Gates: the project's float32 phase bar 1e-5 rms, weights within
5e-6 on the support, error curve rtol 1e-4."""
import argparse
import os

import numpy as np
import pytest
from PIL import Image

from gsw_reference import gsw_reference, traps, uniformity
from oracle import gs_gd_oracle as orc

PHASE_RMS_TOL = 1e-5
WEIGHT_TOL = 5e-6
ERR_RTOL = 1e-4


def _phi0(shape, seed=5):
    return np.random.default_rng(seed).uniform(0, 2 * np.pi, shape)


def _gsw_plan(gpu, t, loops, feedback=1.0, phase=None, weights=None, prec=None):
    """A GSW plan with its inputs set; t [B][H][W] uint8 or float32."""
    tt = gpu.TGT_U8 if t.dtype == np.uint8 else gpu.TGT_F32
    p = gpu.Plan(gpu.ALGO_GSW, t.shape[0], t.shape[1], t.shape[2], tt, False, loops)
    if prec is not None:
        p.set_precision(prec)
    p.set_target(t)
    p.set_feedback(feedback)
    p.set_phase(phase)
    p.set_weights(weights)
    return p


# ---------------------------------------------------------------------------
# 3. feedback = 0 is GS
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype", [((64, 64), np.uint8), ((1024, 1024), np.float32)])
def test_feedback_zero_is_gs(gpu, shape, dtype):
    rng = np.random.default_rng(3)
    t = (rng.integers(0, 256, shape, dtype=np.uint8) if dtype == np.uint8
         else rng.uniform(0, 255, shape).astype(np.float32))[None]
    tt = gpu.TGT_U8 if dtype == np.uint8 else gpu.TGT_F32
    with gpu.Plan(gpu.ALGO_GS, 1, shape[0], shape[1], tt, False, 20) as gs, _gsw_plan(gpu, t, 20, 0.0) as gsw:
        gs.set_target(t)
        gs.run(20)
        gsw.run(20)
        want, got = gs.read(), gsw.read()
        if shape[0] == 1024:
            assert gsw.engine() == ("shuffle", "shuffle") and gsw.info() == gs.info()
        for a, b in zip(want, got):
            np.testing.assert_array_equal(a, b)
        assert np.all(gsw.read_weights() == 1.0)
        assert gsw.kernel_bytes(gpu.KERNEL_COL_MAIN) == gs.kernel_bytes(gpu.KERNEL_COL_MAIN) + 8 * t.size


# ---------------------------------------------------------------------------
# 4. parity with the reference, warm start
# ---------------------------------------------------------------------------
PARITY = [
    # id, shape, traps, dtype, feedback, warm + further iterations
    ("64", (64, 64), 12, np.uint8, 1.0, 30, 20),
    ("64-p0.5", (64, 64), 12, np.uint8, 0.5, 30, 20),
    ("128x256", (128, 256), 24, np.uint8, 1.0, 30, 20),
    ("2048x64-table-twiddles", (2048, 64), 24, np.uint8, 1.0, 30, 20),
    ("4096x64-two-lines", (4096, 64), 24, np.uint8, 1.0, 30, 20),
    ("1024-f32-shuffle", (1024, 1024), 40, np.float32, 1.0, 10, 10),
    ("768x1024-u8", (768, 1024), 40, np.uint8, 1.0, 10, 10),
]


_PARITY_RUNS = {}


def _parity_run(gpu, label, ts, feedback, warm, more):
    """Reference and device results of one parity case, computed once and
    shared by the tests that gate them. ts: targets of one shape and dtype."""
    if label in _PARITY_RUNS:
        return _PARITY_RUNS[label]
    ph0, w0, want = [], [], []
    for t in ts:
        ph, _, _, g = gsw_reference(t, warm, feedback, initial_phase=_phi0(t.shape))
        ph0.append(ph.astype(np.float32))
        w0.append(g.astype(np.float32))
        want.append(gsw_reference(t, more, feedback, initial_phase=ph0[-1], initial_weights=w0[-1]))
    with _gsw_plan(gpu, np.stack(ts), more, feedback, np.stack(ph0), np.stack(w0)) as p:
        p.run(more)
        phase, _, stats, _ = p.read()
        g = p.read_weights()
        prec = p.info()["precision"]
    for k, t in enumerate(ts):
        sup = t > 0
        rms = orc.phase_rms(phase[k], want[k][0])
        dg = float(np.max(np.abs(g[k][sup].astype(np.float64) - want[k][3][sup])))
        derr = float(np.max(np.abs(stats[k, :more, 3] / np.array(want[k][2]) - 1)))
        print(f"[gsw parity] {label}[{k}] p={feedback} {prec} +{more}: phase rms {rms:.3e}, max |dg| {dg:.3e}, "
              f"error curve max rel {derr:.3e}, g in [{g[k][sup].min():.4f}, {g[k][sup].max():.4f}]")
    _PARITY_RUNS[label] = (ts, want, phase, g, stats[:, :more, 3])
    return _PARITY_RUNS[label]


def _case_run(gpu, label, shape, nt, dtype, feedback, warm, more):
    return _parity_run(gpu, label, [traps(shape[0], shape[1], nt, 11, True).astype(dtype)], feedback, warm, more)


def _batch_run(gpu):
    """eight different 256 x 256 targets in one plan (512 waves: still the narrow
    plans, keys 8 / 8; the wide keys run in test_gpu_gsw_variants.py)"""
    return _parity_run(gpu, "8x256x256", [traps(256, 256, 24, seed, True) for seed in range(8)], 1.0, 30, 20)


def _check_phase_and_weights(run):
    ts, want, phase, g, _ = run
    for k, t in enumerate(ts):
        sup = t > 0
        assert orc.phase_rms(phase[k], want[k][0]) <= PHASE_RMS_TOL
        assert np.max(np.abs(g[k][sup].astype(np.float64) - want[k][3][sup])) <= WEIGHT_TOL
        assert np.all(g[k][~sup] == 1.0)


def _check_error_curve(run):
    ts, want, _, _, err = run
    for k in range(len(ts)):
        np.testing.assert_allclose(err[k], want[k][2], rtol=ERR_RTOL)


_PARITY_IDS = [c[0] for c in PARITY]


@pytest.mark.gpu
@pytest.mark.parametrize("label,shape,nt,dtype,feedback,warm,more", PARITY, ids=_PARITY_IDS)
def test_parity_warm_start(gpu, label, shape, nt, dtype, feedback, warm, more):
    """Measured (MI355X): phase rms 1.2e-7 .. 4.2e-7 of the 1e-5 bar (the float32
    1024^2 shuffle pair 4.2e-7), max |dg| 0.8e-7 .. 1.7e-7 of 5e-6."""
    _check_phase_and_weights(_case_run(gpu, label, shape, nt, dtype, feedback, warm, more))


@pytest.mark.gpu
def test_parity_warm_start_batch(gpu):
    _check_phase_and_weights(_batch_run(gpu))


@pytest.mark.gpu
@pytest.mark.parametrize("label,shape,nt,dtype,feedback,warm,more", PARITY, ids=_PARITY_IDS)
def test_parity_error_curve(gpu, label, shape, nt, dtype, feedback, warm, more):
    """The error curve against the reference at the GS tests' rtol of 1e-4.
    Weighted GS makes E proportional to T on these targets, so the error is
    ~1e-4 of sum T^2 / S and its expansion cancels by 1e3 .. 3e4: the gate holds
    because the column pass sums E^2 and E T in float64 against the exact T when
    p > 0 (GS's float32 partials measured 1.1e-4 .. 8.3e-4 here)."""
    _check_error_curve(_case_run(gpu, label, shape, nt, dtype, feedback, warm, more))


@pytest.mark.gpu
def test_parity_error_curve_batch(gpu):
    """See test_parity_error_curve."""
    _check_error_curve(_batch_run(gpu))


# ---------------------------------------------------------------------------
# 5. uniformity on the device
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
@pytest.mark.parametrize("h,w,nt,seed", [(128, 128, 16, 7), (256, 256, 40, 8)])
def test_uniformity_on_device(gpu, h, w, nt, seed, dtype):
    t = traps(h, w, nt, seed, False).astype(dtype)
    phi0 = np.random.default_rng(0).uniform(0, 2 * np.pi, (1, h, w)).astype(np.float32)
    tt = gpu.TGT_U8 if dtype == np.uint8 else gpu.TGT_F32
    with gpu.Plan(gpu.ALGO_GS, 1, h, w, tt, False, 60) as gs, _gsw_plan(gpu, t[None], 60, 1.0, phi0) as gsw:
        gs.set_target(t[None])
        gs.set_phase(phi0)
        gs.run(60)
        gsw.run(60)
        u_gs = uniformity(gs.read()[1][0], t)
        u_w = uniformity(gsw.read()[1][0], t)
    print(f"[gsw] device {h}x{w} {nt} traps {np.dtype(dtype).name}, 60 iterations: u GS {u_gs:.3e}, GSW {u_w:.3e}")
    assert u_w <= 0.005 and u_w <= u_gs / 5


# ---------------------------------------------------------------------------
# 6. state
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_rerun_is_bitwise_and_null_weights_return_to_ones(gpu):
    t = traps(128, 256, 24, 2, True)[None]
    ph, _, _, g = gsw_reference(t[0], 5, 1.0, initial_phase=_phi0(t[0].shape))
    ph, g = ph.astype(np.float32)[None], g.astype(np.float32)[None]
    with _gsw_plan(gpu, t, 12, 1.0, ph, g) as p, _gsw_plan(gpu, t, 12, 1.0, ph, None) as fresh:
        np.testing.assert_allclose(p.read_weights(), g, rtol=3e-7)  # before any run: the weights just set
        p.run(12)
        first = p.read() + (p.read_weights(),)
        p.run(12)  # the captured graph replayed: the run starts from the host-set weights again
        again = p.read() + (p.read_weights(),)
        for a, b in zip(first, again):
            np.testing.assert_array_equal(a, b)
        assert first[4][t > 0].std() > 1e-4  # the weights did move
        p.set_weights(None)
        assert np.all(p.read_weights() == 1.0)
        p.run(12)
        fresh.run(12)
        for a, b in zip(p.read() + (p.read_weights(),), fresh.read() + (fresh.read_weights(),)):
            np.testing.assert_array_equal(a, b)
        assert not np.array_equal(first[0], fresh.read()[0])


@pytest.mark.gpu
def test_batch_equals_single_runs(gpu):
    ts = np.stack([traps(64, 64, 12, s, True) for s in (1, 2, 3)])
    ph = _phi0(ts.shape).astype(np.float32)
    with _gsw_plan(gpu, ts, 15, 1.0, ph) as p:
        p.run(15)
        batch = p.read() + (p.read_weights(),)
    for k in range(3):
        with _gsw_plan(gpu, ts[k:k + 1], 15, 1.0, ph[k:k + 1]) as p:
            p.run(15)
            one = p.read() + (p.read_weights(),)
        for a, b in zip(batch, one):
            np.testing.assert_array_equal(a[k], b[0])


@pytest.mark.gpu
def test_stopped_hologram_keeps_its_weights(gpu):
    ts = np.stack([traps(64, 64, 12, s, True) for s in (4, 5)])
    ph = _phi0(ts.shape).astype(np.float32)
    loops = 12
    with _gsw_plan(gpu, ts, loops, 1.0, ph) as p:
        p.run(loops)
        err = p.read()[2][0, :, 3]
        # the first iteration k >= 1 whose error is a new minimum: a tolerance between
        # it and the earlier minimum stops hologram 0 right there
        k = next(i for i in range(1, loops) if err[i] < err[:i].min())
        tol = 0.5 * (err[k] + err[:k].min())
        p.run(loops, tol, True)
        phase, _, _, iters = p.read()
        g = p.read_weights()
    assert iters[0] == k + 1 < loops
    with _gsw_plan(gpu, ts[:1], k + 1, 1.0, ph[:1]) as q:
        q.run(k + 1)
        np.testing.assert_array_equal(q.read_weights()[0], g[0])
        np.testing.assert_array_equal(q.read()[0][0], phase[0])


# ---------------------------------------------------------------------------
# 7. robustness
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_dense_target_keeps_weights_finite(gpu):
    t = np.random.default_rng(6).uniform(0, 255, (1, 64, 64)).astype(np.float32)
    with _gsw_plan(gpu, t, 200, 1.0) as p:
        p.run(200)
        phase = p.read()[0]
        g = p.read_weights()
    print(f"[gsw] dense 64x64 p=1 200 iterations: g in [{g.min():.3e}, {g.max():.3e}]")
    assert np.all(np.isfinite(g)) and np.all(g > 0) and np.all(np.isfinite(phase))


@pytest.mark.gpu
def test_long_run_on_traps(gpu):
    t = traps(64, 64, 12, 9, True)
    with _gsw_plan(gpu, t[None], 1000, 1.0, _phi0((1, 64, 64)).astype(np.float32)) as p:
        p.run(1000)
        e = p.read()[1][0]
        g = p.read_weights()[0]
    u = uniformity(e, t)
    print(f"[gsw] traps 64x64 1000 iterations: g in [{g[t > 0].min():.4f}, {g[t > 0].max():.4f}], u {u:.3e}")
    assert g[t > 0].min() >= 0.5 and g[t > 0].max() <= 2.0 and u <= 0.005


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(gpu, monkeypatch):
    from spatial_light_modulator_module_amd import algorithms as alg

    def refused(h, w):
        with pytest.raises(gpu.SlmError) as ei:
            gpu.Plan(gpu.ALGO_GSW, 1, h, w, gpu.TGT_U8, False, 5)
        assert ei.value.code == gpu.ERR_UNSUPPORTED
        for word in ("64", "4096", "768", "powers of two"):
            assert word in str(ei.value)

    refused(1080, 1920)
    refused(97, 101)
    with pytest.raises(ValueError, match="4096.*768"):
        alg.run_gsw(np.zeros((1, 1080, 1920), np.uint8), 5)
    with monkeypatch.context() as m:
        m.setenv("SLM_ENGINE", "float64")
        refused(64, 64)
        with pytest.raises(ValueError, match="SLM_ENGINE=float64"):
            alg.run_gsw(np.zeros((1, 64, 64), np.uint8), 5)
    with gpu.Plan(gpu.ALGO_GS, 1, 64, 64, gpu.TGT_U8, False, 5) as gs:
        for call in (lambda: gs.set_weights(np.ones((1, 64, 64))), lambda: gs.set_weights(None), gs.read_weights,
                     lambda: gs.set_feedback(1.0)):
            with pytest.raises(gpu.SlmError) as ei:
                call()
            assert ei.value.code == gpu.ERR_STATE
    t = traps(64, 64, 12, 1, True)[None]
    with _gsw_plan(gpu, t, 5) as p:
        for bad in (-0.5, float("nan"), float("inf")):
            with pytest.raises(gpu.SlmError) as ei:
                p.set_feedback(bad)
            assert ei.value.code == gpu.ERR_ARG
        for v in (0.0, -1.0, np.nan, np.inf):
            w = np.ones(t.shape, np.float32)
            w[t > 0] = [v] + [1.0] * (np.count_nonzero(t) - 1)
            with pytest.raises(gpu.SlmError) as ei:
                p.set_weights(w)
            assert ei.value.code == gpu.ERR_ARG
        w = np.ones(t.shape, np.float32)
        w[t == 0] = -3.0  # off the support anything goes
        p.set_weights(w)
        p.run(5)
        assert np.all(p.read_weights()[t == 0] == 1.0)
        with pytest.raises(ValueError, match="feedback"):
            alg.run_gsw(t, 5, feedback=-1.0)


# ---------------------------------------------------------------------------
# 9. CLI, and the one-shot entry
# ---------------------------------------------------------------------------
def _ns(**kw):
    base = dict(incomming_intensity="uniform", tolerance=0.0, max_loops=5, gif=False, print_info=False,
                plot_error=False)
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.gpu
def test_one_shot_equals_plan(gpu):
    from spatial_light_modulator_module_amd import algorithms as alg

    t = traps(128, 128, 16, 3, True)[None]
    ph = _phi0(t.shape).astype(np.float32)
    phase, e, stats, iters, g = gpu.gsw(t, 9, 0.5, initial_phase=ph)
    out = alg.run_gsw(t, 9, 0.5, initial_phase=ph, return_weights=True)
    np.testing.assert_array_equal(phase, out[0])
    np.testing.assert_array_equal(e, out[1])
    np.testing.assert_array_equal(stats[0, :, 3], out[2][0])
    np.testing.assert_array_equal(g, out[5])
    assert iters[0] == -1


@pytest.mark.gpu
def test_generate_hologram_cli(gpu, tmp_path, monkeypatch):
    from spatial_light_modulator_module_amd import algorithms as alg
    from spatial_light_modulator_module_amd import generate_hologram as gh

    monkeypatch.chdir(tmp_path)
    os.makedirs("images")
    Image.fromarray(traps(768, 1024, 40, 4, True)).save("images/traps.png")
    path = gh.cli(["traps.png", "-alg", "weighted_gerchberg_saxton", "--feedback", "0.5", "-l", "6", "-dest_dir",
                   "holos"])
    assert "_weighted_gerchberg_saxton" in path and path.endswith(".npy")
    h = np.load(path)
    assert h.shape == (768, 1024) and h.dtype == np.float64
    target = gh.prepare_target("traps.png", gh.build_parser().parse_args(["traps.png"]))
    phase = alg.run_gsw(target[None], 6, 0.5)[0]
    np.testing.assert_array_equal(h, alg.hologram_from(phase[0]))
    gs_phase = alg.run_gs(target[None], 6)[0]
    assert not np.array_equal(phase, gs_phase)


@pytest.mark.gpu
def test_sequence_cli(gpu, tmp_path, monkeypatch):
    from spatial_light_modulator_module_amd import generate_hologram_sequence as ghs
    from spatial_light_modulator_module_amd.algorithms import weighted_gerchberg_saxton

    frames = [traps(256, 512, 20, s, True) for s in (1, 2, 3)]
    for root in ("one", "multi"):
        d = tmp_path / root / "images" / "moving_traps" / "walk"
        d.mkdir(parents=True)
        for i, f in enumerate(frames):
            Image.fromarray(f).save(d / f"{i}.png")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SLM_GPUS"):
        monkeypatch.delenv(k, raising=False)
    argv = ["walk", "-v", "a", "-ct2pi", "255", "-loops", "5", "-alg", "weighted_gerchberg_saxton"]
    monkeypatch.chdir(tmp_path / "one")
    errors = ghs.cli(argv, plot=False)
    assert sorted(errors) == [0, 1, 2]
    for i, f in enumerate(frames):
        h = np.load(tmp_path / "one" / "holograms" / "walk_a_holograms" / f"{i}.npy")
        holo, _, err = weighted_gerchberg_saxton(f, _ns(max_loops=5, feedback=1.0))  # one frame at a time
        np.testing.assert_array_equal(h, holo)
        assert errors[i] == err
    # the one-process shard path ($SLM_GPUS: one GPU listed twice) writes the same files
    monkeypatch.chdir(tmp_path / "multi")
    monkeypatch.setenv("SLM_GPUS", "0,0")
    assert ghs.cli(argv, plot=False) == errors
    for i in range(3):
        np.testing.assert_array_equal(np.load(tmp_path / "multi" / "holograms" / "walk_a_holograms" / f"{i}.npy"),
                                      np.load(tmp_path / "one" / "holograms" / "walk_a_holograms" / f"{i}.npy"))
