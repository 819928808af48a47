"""MRAF (SLM_ALGO_MRAF, COL_MRAF_MAIN) on the MI355X against the float64
reference of tests/mraf_reference.py.

Protocol: the reference runs `warm` iterations from start_phase; its phase
rounded to float32 goes to both sides, which run `more` further iterations.
Gates: phase within 1e-5 rms, error curve rtol 1e-4, efficiency curve within
1e-5 absolute. (A float32 NumPy run of the same cases sits at 2.5e-7 .. 1.25e-6,
9e-7 .. 2.1e-5 and 1e-9 .. 5e-8 against them.) Targets are shapes(h, w), uint8
or cast to float32. Every reference run is computed once and shared.

Measured on the MI355X over the ten cases of test_warm_start_parity at the
plan's default precision (every case prints its own figures; the table is in
DESIGN.md section 5, "MRAF"):
    uint8 targets (float64 butterflies): phase rms 7.1e-08 .. 2.3e-07, error curve
        2.0e-07 .. 6.0e-06 relative, efficiency 4.1e-09 .. 2.1e-08 absolute;
    float32 targets (float32 butterflies): phase rms 6.6e-07 .. 7.4e-07, error
        curve 4.5e-06 .. 1.0e-05 relative, efficiency 4.9e-08 .. 7.5e-08 absolute.
Forced to float32 butterflies the uint8 64 x 64 and 128 x 256 cases give 6.5e-7
and 8.6e-7 rms (error curve 1.3e-5 and 6.1e-6 relative)."""
import os

import numpy as np
import pytest
from PIL import Image

from gsw_reference import incoming_gauss, uniformity
from mraf_reference import mraf_reference, shapes, start_phase
from oracle import gs_gd_oracle as orc

PHASE_RMS_TOL = 1e-5
ERR_RTOL = 1e-4
EFF_ATOL = 1e-5

PREC = {"f32": 0, "f64": 1}


class env:
    """Plan-picker overrides, set around plan creation and set_precision."""

    def __init__(self, **kw):
        self.kw = {k: v for k, v in kw.items() if v is not None}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update({k: str(v) for k, v in self.kw.items()})

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_REFS = {}


def _reference(h, w, dtype=np.uint8, m=0.4, warm=10, more=20, gauss=False, roll=(0, 0)):
    """Target, region, a_in, the float32 warm start and the reference's
    (phase, E, errors, efficiencies) after `more` further iterations."""
    k = (h, w, np.dtype(dtype).name, m, warm, more, gauss, roll)
    if k not in _REFS:
        t, r = shapes(h, w)
        t, r = np.roll(t, roll, (0, 1)).astype(dtype), np.roll(r, roll, (0, 1))
        a = incoming_gauss(h, w) if gauss else None
        ph0 = mraf_reference(t, r, warm, m, initial_phase=start_phase(t.shape), ain=a)[0].astype(np.float32)
        want = mraf_reference(t, r, more, m, initial_phase=ph0, ain=a)
        for arr in (t, r, ph0) + tuple(want) + (() if a is None else (a,)):
            arr.flags.writeable = False
        _REFS[k] = dict(t=t, r=r, ain=a, ph0=ph0, want=want, m=m, more=more)
    return _REFS[k]


def _plan(gpu, refs, loops=None, prec=None, overrides=None, expect=None, phase=True):
    """An MRAF plan of the holograms `refs` with every input set."""
    t = np.stack([x["t"] for x in refs])
    tt = gpu.TGT_U8 if t.dtype == np.uint8 else gpu.TGT_F32
    ain = refs[0]["ain"]
    with env(**(overrides or {})):
        plan = gpu.Plan(gpu.ALGO_MRAF, t.shape[0], t.shape[1], t.shape[2], tt, ain is not None,
                        loops or refs[0]["more"])
        if prec is not None:
            plan.set_precision(PREC[prec])
        info = plan.info()
    try:
        for name, value in (expect or {}).items():
            assert info[name] == value, (name, value, info)
        plan.set_target(t)
        plan.set_region(np.stack([x["r"] for x in refs]))
        if ain is not None:
            plan.set_ain(ain)
        plan.set_mixing(refs[0]["m"])
        plan.set_phase(np.stack([x["ph0"] for x in refs]) if phase else None)
    except BaseException:
        plan.close()
        raise
    return plan


def _everything(plan):
    """phase, E, statistics, iterations and efficiencies of the last run."""
    return plan.read() + (plan.read_efficiency(),)


def _assert_bitwise(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def _gate(label, refs, got, info):
    """The three gates on a batch of holograms; prints the figures first."""
    phase, _, stats, _, eff = got
    fig = []
    for k, x in enumerate(refs):
        want, more = x["want"], x["more"]
        fig.append((orc.phase_rms(phase[k], want[0]), float(np.max(np.abs(stats[k, :more, 3] / want[2] - 1))),
                    float(np.max(np.abs(eff[k, :more] - want[3])))))
    worst = np.max(np.array(fig), axis=0)
    print(f"[mraf] {label}: key {info['col_plan']} cw {info['col_cw']} threads {info['col_threads']} "
          f"{info['precision']} layout {info['layout']} m={refs[0]['m']}: phase rms {worst[0]:.3e}, "
          f"error curve max rel {worst[1]:.3e}, efficiency max abs {worst[2]:.3e}")
    for k, x in enumerate(refs):
        want, more = x["want"], x["more"]
        assert fig[k][0] <= PHASE_RMS_TOL
        np.testing.assert_allclose(stats[k, :more, 3], want[2], rtol=ERR_RTOL)
        np.testing.assert_allclose(eff[k, :more], want[3], rtol=0, atol=EFF_ATOL)


def _parity(gpu, label, refs, prec=None, overrides=None, expect=None, repeats=1):
    with _plan(gpu, refs, prec=prec, overrides=overrides, expect=expect) as plan:
        info = plan.info()
        plan.run(refs[0]["more"])
        first = _everything(plan)
        for _ in range(repeats - 1):
            plan.run(refs[0]["more"])
            _assert_bitwise(first, _everything(plan))
    _gate(label, refs, first, info)
    return first


# ---------------------------------------------------------------------------
# warm-start parity
# ---------------------------------------------------------------------------
CASES = [
    (64, 64, 0.4, 10, 20, np.uint8, False),
    (64, 64, 0.7, 30, 20, np.uint8, False),
    (64, 64, 1.0, 30, 20, np.uint8, False),
    (128, 256, 0.4, 10, 20, np.uint8, True),
    (128, 256, 0.7, 30, 20, np.uint8, False),
    (2048, 64, 0.4, 10, 20, np.uint8, False),
    (4096, 64, 0.4, 10, 20, np.uint8, False),
    (64, 768, 0.4, 10, 20, np.float32, False),
    (768, 1024, 0.4, 10, 10, np.uint8, False),
    (1024, 1024, 0.4, 10, 10, np.float32, True),
]


def _case_id(c):
    h, w, m, warm, more, dtype, gauss = c
    return f"{h}x{w}-m{m}-{warm}+{more}-{np.dtype(dtype).name}" + ("-gauss" if gauss else "")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_warm_start_parity(gpu, case):
    h, w, m, warm, more, dtype, gauss = case
    _parity(gpu, f"parity {_case_id(case)}", [_reference(h, w, dtype, m, warm, more, gauss)])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[_case_id(CASES[0]), _case_id(CASES[3])])
def test_both_precisions(gpu, case, prec):
    h, w, m, warm, more, dtype, gauss = case
    _parity(gpu, f"precision {prec} {_case_id(case)}", [_reference(h, w, dtype, m, warm, more, gauss)], prec=prec,
            expect=dict(precision=prec))


@pytest.mark.gpu
def test_batch_equals_solo_runs(gpu):
    """Eight rolled copies of shapes(256, 256) in one plan: each equals its
    solo run bit for bit and passes the parity gates."""
    rolls = [(0, 0), (17, 3), (100, 40), (5, 130), (128, 128), (31, 77), (90, 9), (60, 150)]
    refs = [_reference(256, 256, roll=r) for r in rolls]
    got = _parity(gpu, "batch of 8 256x256", refs)
    for k, x in enumerate(refs):
        with _plan(gpu, [x]) as plan:
            plan.run(x["more"])
            solo = _everything(plan)
        _assert_bitwise([a[k:k + 1] for a in got], solo)


@pytest.mark.gpu
def test_reruns_repeat_bitwise(gpu):
    """A rerun (a graph replay), and a rerun after set_mixing to another value
    and back, repeat bit for bit; the other value does not."""
    x = _reference(128, 256, gauss=True)
    with _plan(gpu, [x]) as plan:
        plan.run(x["more"])
        first = _everything(plan)
        plan.run(x["more"])
        _assert_bitwise(first, _everything(plan))
        plan.set_mixing(0.7)
        plan.run(x["more"])
        other = _everything(plan)
        assert not np.array_equal(other[0], first[0])
        plan.set_mixing(x["m"])
        plan.run(x["more"])
        _assert_bitwise(first, _everything(plan))


# ---------------------------------------------------------------------------
# every column kernel: plan keys (plans.hpp, kPlans) and their valid tiles, as
# tests/test_gpu_gsw_variants.py tabulates them (ColCfg<K, cw>::kValid)
# ---------------------------------------------------------------------------
KEYS = {
    0: (64, "wide"), 1: (128, "wide"), 2: (256, "wide"), 3: (512, "wide"), 4: (768, "wide"), 5: (1024, "wide"),
    6: (2048, "wide"), 7: (4096, "wide"), 8: (256, "narrow"), 9: (512, "narrow"), 10: (768, "narrow"),
    11: (1024, "narrow"), 12: (2048, "narrow"), 13: (4096, "narrow"),
}
TILES = {
    (0, 8): 64, (0, 16): 128,
    (1, 8): 64, (1, 16): 128,
    (2, 4): 64, (2, 8): 128, (2, 16): 256,
    (3, 2): 64, (3, 4): 128, (3, 8): 256, (3, 16): 512,
    (4, 2): 64, (4, 4): 128, (4, 8): 256, (4, 16): 512,
    (5, 1): 64, (5, 2): 128, (5, 4): 256, (5, 8): 512, (5, 16): 1024,
    (6, 1): 128, (6, 2): 256, (6, 4): 512, (6, 8): 1024,
    (7, 1): 128, (7, 2): 256, (7, 4): 512,
    (8, 2): 64, (8, 4): 128, (8, 8): 256, (8, 16): 512,
    (9, 1): 64, (9, 2): 128, (9, 4): 256, (9, 8): 512, (9, 16): 1024,
    (10, 1): 64, (10, 2): 128, (10, 4): 256, (10, 8): 512, (10, 16): 1024,
    (11, 1): 128, (11, 2): 256, (11, 4): 512, (11, 8): 1024,
    (12, 1): 256, (12, 2): 512, (12, 4): 1024,
    (13, 1): 256, (13, 2): 256, (13, 4): 512,
}


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("key,cw", sorted(TILES), ids=[f"key{k}-{KEYS[k][0]}{KEYS[k][1]}-cw{c}"
                                                       for k, c in sorted(TILES)])
def test_every_tile(gpu, key, cw, prec):
    """Every valid (column key, tile width), forced with SLM_COL_PLAN /
    SLM_COL_CW on the smallest shape that selects it (n x 64), at both
    precisions: parity, and a rerun equal bit for bit. info() must report the
    forced geometry, so an ignored override fails the case."""
    n, variant = KEYS[key]
    _parity(gpu, f"tile key{key} {n}{variant} cw{cw}", [_reference(n, 64)], prec=prec,
            overrides=dict(SLM_COL_PLAN=variant, SLM_COL_CW=cw),
            expect=dict(col_plan=key, col_cw=cw, col_threads=TILES[(key, cw)], precision=prec), repeats=2)


@pytest.mark.gpu
def test_narrow_layout_pair(gpu):
    """A single 1024 x 1024 image runs the 8-wide X / 2-wide Y layout pair
    (the CASES entry of that shape must not run the default one unnoticed)."""
    x = _reference(1024, 1024, np.float32, 0.4, 10, 10, True)
    with _plan(gpu, [x]) as plan:
        assert plan.info()["layout"] == (8, 2), plan.info()


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _ns(**kw):
    import argparse

    base = dict(incomming_intensity="uniform", tolerance=0.0, max_loops=5, gif=False, print_info=False,
                plot_error=False)
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.gpu
def test_mraf_smooths_what_gs_speckles(gpu):
    """256 x 256, cold from the start phase, 60 iterations through
    algorithms.mraf with the default margin region, beside a GS plan."""
    from spatial_light_modulator_module_amd import algorithms as alg

    t, _ = shapes(256, 256)
    ph0 = start_phase(t.shape).astype(np.float32)
    region = alg.signal_region(t, 8)
    phase, e, errs, norm, emax, effs = alg.run_mraf(t[None], region[None], 60, 0.4, initial_phase=ph0[None],
                                                    return_efficiency=True)
    e_gs = alg.run_gs(t[None], 60, initial_phase=ph0[None])[1]
    u_m, u_gs = uniformity(e[0], t), uniformity(e_gs[0], t)
    print(f"[mraf] 256x256 cold, 60 iterations: u GS {u_gs:.3e}, MRAF {u_m:.3e}, efficiency {effs[0][-1]:.4f}")
    assert u_m <= 0.01
    assert u_gs >= 0.1
    assert len(errs[0]) == len(effs[0]) == 60 and norm[0] == 200
    # the drop-in shaped entry point: the same run from GS's own cold start
    holo, expected, evolution = alg.mraf(t, _ns(max_loops=60))
    cold = alg.run_mraf(t[None], region[None], 60, 0.4)
    np.testing.assert_array_equal(holo, alg.hologram_from(cold[0][0]))
    assert evolution == cold[2][0] and expected.shape == t.shape and expected.dtype == np.float64
    assert abs(expected[region > 0].max() - 200) < 1e-9


@pytest.mark.gpu
def test_generate_hologram_cli(gpu, tmp_path, monkeypatch):
    from spatial_light_modulator_module_amd import algorithms as alg
    from spatial_light_modulator_module_amd import generate_hologram as gh

    monkeypatch.chdir(tmp_path)
    os.makedirs("images")
    t, r = shapes(96, 128)
    Image.fromarray(t).save("images/disc.png")
    Image.fromarray(r * 255).save("images/disc_region.png")
    path = gh.cli(["disc.png", "-alg", "mraf", "--mixing", "0.5", "-l", "6", "-dest_dir", "holos"])
    assert "_mraf" in path and path.endswith(".npy")
    h = np.load(path)
    assert h.shape == (768, 1024) and h.dtype == np.float64
    args = gh.build_parser().parse_args(["disc.png"])
    target = gh.prepare_target("disc.png", args)
    holo = alg.mraf(target, _ns(max_loops=6, mixing=0.5))[0]
    np.testing.assert_array_equal(h, holo)
    # with a region image: through the target's geometric preparation, nonzero = signal
    path = gh.cli(["disc.png", "-alg", "mraf", "--mixing", "0.5", "--region", "disc_region.png", "-l", "6",
                   "-dest_dir", "holos"])
    region = gh.prepare_target("disc_region.png", args)
    assert region.shape == (768, 1024) and 0 < np.count_nonzero(region) < region.size
    holo_r = alg.mraf(target, _ns(max_loops=6, mixing=0.5, signal_region=region))[0]
    np.testing.assert_array_equal(np.load(path), holo_r)
    assert not np.array_equal(holo_r, holo)


# ---------------------------------------------------------------------------
# tolerance stop
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_tolerance_stop_on_the_region_error(gpu):
    """tol = the geometric mean of two neighbouring values of the reference
    error curve that differ by more than 1 %: the checked run stops where the
    reference does, and the passes launched after the stop leave the phase, the
    expected output and the efficiency rows untouched."""
    a = _reference(256, 256)
    err = a["want"][2]
    k = next(i for i in range(2, len(err) - 2) if err[i] < 0.99 * err[i - 1] and err[:i].min() == err[i - 1])
    tol = float(np.sqrt(err[k] * err[k - 1]))
    loops = a["more"]
    with _plan(gpu, [a]) as plan:
        plan.run(loops)
        full = _everything(plan)
        plan.run(loops, tol, True)
        phase, e, stats, iters, eff = _everything(plan)
        # what the stopped hologram must hold: its state after k + 1 iterations
        plan.run(k + 1)
        short = _everything(plan)
    print(f"[mraf] tolerance stop: tol {tol:.6e} between error[{k - 1}] {err[k - 1]:.6e} and error[{k}] "
          f"{err[k]:.6e}; stopped after {iters[0]} of {loops}")
    assert iters[0] == k + 1
    np.testing.assert_allclose(stats[0, :k + 1, 3], err[:k + 1], rtol=ERR_RTOL)
    np.testing.assert_allclose(eff[0, :k + 1], a["want"][3][:k + 1], rtol=0, atol=EFF_ATOL)
    np.testing.assert_array_equal(phase, short[0])
    np.testing.assert_array_equal(e, short[1])
    np.testing.assert_array_equal(stats[0, :k + 1], short[2][0, :k + 1])
    np.testing.assert_array_equal(eff[0, :k + 1], short[4][0, :k + 1])
    assert not np.array_equal(phase, full[0])
    # rows past the stop: left as the earlier run wrote them, as the statistics rows are
    np.testing.assert_array_equal(stats[0, k + 1:loops], full[2][0, k + 1:loops])
    np.testing.assert_array_equal(eff[0, k + 1:loops], full[4][0, k + 1:loops])


# ---------------------------------------------------------------------------
# refusals, states, bytes
# ---------------------------------------------------------------------------
def _code(gpu, fn, *a):
    with pytest.raises(gpu.SlmError) as e:
        fn(*a)
    return e.value.code, str(e.value)


@pytest.mark.gpu
def test_refusals_and_states(gpu):
    t, r = shapes(64, 64)
    for algo in (gpu.ALGO_GS, gpu.ALGO_GSW, gpu.ALGO_GD):
        with gpu.Plan(algo, 1, 64, 64, gpu.TGT_U8, False, 4) as p:
            assert _code(gpu, p.set_region, r[None])[0] == gpu.ERR_STATE
            assert _code(gpu, p.set_mixing, 0.5)[0] == gpu.ERR_STATE
            assert _code(gpu, p.read_efficiency)[0] == gpu.ERR_STATE
    for shape in ((97, 101), (1080, 1920)):
        code, msg = _code(gpu, gpu.Plan, gpu.ALGO_MRAF, 1, shape[0], shape[1], gpu.TGT_U8, False, 4)
        assert code == gpu.ERR_UNSUPPORTED and "fused engine only" in msg and f"{shape[0]} x {shape[1]}" in msg
    with env(SLM_ENGINE="float64"):
        code, msg = _code(gpu, gpu.Plan, gpu.ALGO_MRAF, 1, 64, 64, gpu.TGT_U8, False, 4)
        assert code == gpu.ERR_UNSUPPORTED and "SLM_ENGINE=float64" in msg
        # the weighted-GS refusal is what it was
        code, msg = _code(gpu, gpu.Plan, gpu.ALGO_GSW, 1, 64, 64, gpu.TGT_U8, False, 4)
        assert code == gpu.ERR_UNSUPPORTED and msg.split(": ", 1)[1].startswith("weighted GS (SLM_ALGO_GSW) runs")
    with gpu.Plan(gpu.ALGO_MRAF, 2, 64, 64, gpu.TGT_U8, False, 4) as p:
        for m in (0.0, -0.5, 1.5, float("nan"), float("inf")):
            assert _code(gpu, p.set_mixing, m)[0] == gpu.ERR_ARG
        p.set_mixing(1.0)
        p.set_mixing(0.4)
        p.set_target(np.stack([t, t]))
        code, msg = _code(gpu, p.run, 4)  # no region yet
        assert code == gpu.ERR_STATE and "region" in msg
        away = np.zeros_like(r)
        away[50:60, 50:60] = 1
        code, msg = _code(gpu, p.set_region, np.stack([r, away]))
        assert code == gpu.ERR_ARG and "hologram 1" in msg
        assert _code(gpu, p.run, 4)[0] == gpu.ERR_STATE  # the refused region is not in force
        p.set_region(np.stack([r, r]))
        p.run(4)
        eff = p.read_efficiency()
        assert eff.shape == (2, 4) and np.all((eff > 0) & (eff < 1)) and np.array_equal(eff[0], eff[1])
        # a new target the region no longer fits: the run names the hologram
        p.set_target(np.stack([t, np.roll(t, (40, 40), (0, 1))]))
        code, msg = _code(gpu, p.run, 4)
        assert code == gpu.ERR_ARG and "hologram 1" in msg
        p.set_region(np.stack([r, np.roll(r, (40, 40), (0, 1))]))
        p.run(4)
        np.testing.assert_array_equal(p.read_efficiency()[0], eff[0])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_kernel_bytes(gpu, dtype):
    tt = gpu.TGT_U8 if dtype == np.uint8 else gpu.TGT_F32
    with gpu.Plan(gpu.ALGO_MRAF, 2, 256, 128, tt, False, 4) as p, gpu.Plan(gpu.ALGO_GS, 2, 256, 128, tt, False, 4) as g:
        assert p.kernel_bytes(gpu.KERNEL_COL_MAIN) == g.kernel_bytes(gpu.KERNEL_COL_MAIN) + 2 * 256 * 128
        assert p.kernel_bytes(gpu.KERNEL_ROW_MAIN) == g.kernel_bytes(gpu.KERNEL_ROW_MAIN)
