"""Weighted Gerchberg-Saxton (COL_GSW_MAIN) on every column kernel it is built
for: all 14 column plan keys, every valid tile width, both precisions for both
target types, the general exponent (powf / pow), an incoming amplitude, and
the bitwise invariances (layout pair, store mode, precision switch, stop in a
batch, shards) plus the GIF chunk hand-off.

Protocol and gates are test_gpu_gsw.py's: the float64 reference
(tests/gsw_reference.py) runs 30 iterations from _phi0, its phase and weights
rounded to float32 go to both sides, both run 20 more; phase within 1e-5 rms,
weights within 5e-6 on the support and exactly 1 off it, error curve rtol 1e-4.
Targets are traps(H, 64, 24, 11, True) (12 traps at 64 x 64), uint8 or cast to
float32. Every plan asserts through info() the column plan key, tile width,
thread count, precision and layout pair the case claims to run: an override
the library ignores fails the case.

Every reference run is computed once per (shape, dtype, p, a_in) and shared."""
import argparse
import os

import numpy as np
import pytest

from gsw_reference import gsw_reference, incoming_gauss, traps
from oracle import gs_gd_oracle as orc

PHASE_RMS_TOL = 1e-5
WEIGHT_TOL = 5e-6
ERR_RTOL = 1e-4

W = 64  # one row plan (key 0); the smallest supported row length


class env:
    """Plan-picker overrides, set around plan creation and set_precision (both
    read them) and restored afterwards."""

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


# ---------------------------------------------------------------------------
# the column kernels: plan keys (plans.hpp, kPlans) and their valid tiles
# ---------------------------------------------------------------------------
# key: (column length, variant, threads per column T = n / e)
KEYS = {
    0: (64, "wide", 8), 1: (128, "wide", 8), 2: (256, "wide", 16), 3: (512, "wide", 32), 4: (768, "wide", 32),
    5: (1024, "wide", 64), 6: (2048, "wide", 128), 7: (4096, "wide", 128),
    8: (256, "narrow", 32), 9: (512, "narrow", 64), 10: (768, "narrow", 64), 11: (1024, "narrow", 128),
    12: (2048, "narrow", 256), 13: (4096, "narrow", 256),
}
# (key, cw): threads of the tile. ColCfg<K, cw>::kValid: 64 <= threads <= 1024,
# threads = (cw / L) T, and lds_line(n) cw 8 <= 160 KiB with lds_line(n) =
# n + n / 16. L = 2 columns per thread only at key 13 (4096 narrow) with an
# even cw. Left out by the thread bounds: every pair below the first / above
# the last of its key's row. Left out by LDS: 4096 at cw 8 and 16
# (4352 x 8 x 8 = 272 KiB; cw 4 is 136 KiB), wide and narrow alike -- so the
# L == 2 tiles of 4096 narrow are cw 2 and 4, next to the L == 1 tile cw 1.
TILES = {
    (0, 8): 64, (0, 16): 128,  # 64-thread single-wave tile: (0, 8)
    (1, 8): 64, (1, 16): 128,
    (2, 4): 64, (2, 8): 128, (2, 16): 256,
    (3, 2): 64, (3, 4): 128, (3, 8): 256, (3, 16): 512,
    (4, 2): 64, (4, 4): 128, (4, 8): 256, (4, 16): 512,
    (5, 1): 64, (5, 2): 128, (5, 4): 256, (5, 8): 512, (5, 16): 1024,  # 1024-thread table-twiddle tile: (5, 16)
    (6, 1): 128, (6, 2): 256, (6, 4): 512, (6, 8): 1024,
    (7, 1): 128, (7, 2): 256, (7, 4): 512,
    (8, 2): 64, (8, 4): 128, (8, 8): 256, (8, 16): 512,  # wave-local multi-column tile: (8, 2)
    (9, 1): 64, (9, 2): 128, (9, 4): 256, (9, 8): 512, (9, 16): 1024,
    (10, 1): 64, (10, 2): 128, (10, 4): 256, (10, 8): 512, (10, 16): 1024,
    (11, 1): 128, (11, 2): 256, (11, 4): 512, (11, 8): 1024,
    (12, 1): 256, (12, 2): 512, (12, 4): 1024,
    (13, 1): 256, (13, 2): 256, (13, 4): 512,  # L == 1 at cw 1; L == 2 at cw 2 and 4
}
# pick_cw without an override: 2-column tiles on the narrow plans; on the wide
# ones the first valid of 4, 8, 16 (64- and 128-point columns start at 8)
DEFAULT_CW = {0: 8, 1: 8, 2: 4, 3: 4, 4: 4, 5: 4, 6: 4, 7: 4, 8: 2, 9: 2, 10: 2, 11: 2, 12: 2, 13: 2}
DEFAULT_LAYOUT = (4, 4)  # the narrow pair (8, 2) needs 1024-point rows and columns


def test_tile_table_is_consistent():
    """The literal table against the rule it was derived from (host only)."""
    want = {}
    for key, (n, variant, t) in KEYS.items():
        for cw in (1, 2, 4, 8, 16):
            lines = 2 if (key == 13 and cw % 2 == 0) else 1
            threads = cw // lines * t
            if 64 <= threads <= 1024 and (n + n // 16) * cw * 8 <= 160 * 1024:
                want[(key, cw)] = threads
    assert want == TILES
    assert all((k, cw) in TILES for k, cw in DEFAULT_CW.items())
    assert sorted(KEYS) == list(range(14))


def _key_id(key):
    n, variant, _ = KEYS[key]
    return f"key{key}-{n}{variant}"


# ---------------------------------------------------------------------------
# reference runs, cached
# ---------------------------------------------------------------------------
def _phi0(shape, seed=5):
    return np.random.default_rng(seed).uniform(0, 2 * np.pi, shape)


def _target(h, w, dtype, seed=11, nt=None):
    if nt is None:
        nt = 12 if (h, w) == (64, 64) else 24
    return traps(h, w, nt, seed, True).astype(dtype)


_REFS = {}


def _reference(h, w, dtype, p=1.0, ain=None, seed=11, warm=30, more=20, nt=None):
    """The warm start and the expected result of one target: ph0, w0 (float32,
    what both sides start from), want = (phase, E, errors, g) after `more`
    further iterations, and the range of the update factor over all of them.
    ain: None, or a scale s for s * incoming_gauss(h, w)."""
    k = (h, w, np.dtype(dtype).name, p, ain, seed, warm, more, nt)
    if k not in _REFS:
        t = _target(h, w, dtype, seed, nt)
        a = None if ain is None else (np.float32(ain) * incoming_gauss(h, w)).astype(np.float32)
        fac = []
        ph, _, _, g = gsw_reference(t, warm, p, initial_phase=_phi0(t.shape), ain=a, factors=fac)
        ph0, w0 = ph.astype(np.float32), g.astype(np.float32)
        want = gsw_reference(t, more, p, initial_phase=ph0, initial_weights=w0, ain=a, factors=fac)
        for arr in (t, ph0, w0) + tuple(np.asarray(x) for x in want) + (() if a is None else (a,)):
            arr.flags.writeable = False
        _REFS[k] = dict(t=t, ain=a, ph0=ph0, w0=w0, want=want, more=more, p=p,
                        factors=(min(f[0] for f in fac), max(f[1] for f in fac)))
    return _REFS[k]


# ---------------------------------------------------------------------------
# device runs
# ---------------------------------------------------------------------------
PREC = {"f32": 0, "f64": 1}


def _plan(gpu, t, loops, p=1.0, phase=None, weights=None, prec=None, ain=None, overrides=None, expect=None,
          algo=None):
    """A weighted-GS plan with its inputs set, created (and its precision set)
    under `overrides`; info() must report `expect`."""
    tt = gpu.TGT_U8 if t.dtype == np.uint8 else gpu.TGT_F32
    algo = gpu.ALGO_GSW if algo is None else algo
    with env(**(overrides or {})):
        plan = gpu.Plan(algo, t.shape[0], t.shape[1], t.shape[2], tt, ain is not None, loops)
        if prec is not None:
            plan.set_precision(PREC[prec])
        info = plan.info()
    try:
        for name, value in (expect or {}).items():
            assert info[name] == value, (name, value, info)
        plan.set_target(t)
        if ain is not None:
            plan.set_ain(ain)
        if algo == gpu.ALGO_GSW:
            plan.set_feedback(p)
            plan.set_weights(weights)
        plan.set_phase(phase)
    except BaseException:
        plan.close()
        raise
    return plan


def _everything(plan):
    """phase, E, statistics, iterations and weights of the last run."""
    return plan.read() + (plan.read_weights(),)


def _assert_bitwise(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def _geometry(key, cw, prec, layout=DEFAULT_LAYOUT):
    return dict(col_plan=key, col_cw=cw, col_threads=TILES[(key, cw)], precision=prec, layout=layout)


def _gate(label, refs, phase, g, stats, info):
    """The three gates on a batch of holograms; prints geometry and deviations first."""
    worst = [0.0, 0.0, 0.0]
    for k, r in enumerate(refs):
        sup = r["t"] > 0
        want, more = r["want"], r["more"]
        rms = orc.phase_rms(phase[k], want[0])
        dg = float(np.max(np.abs(g[k][sup].astype(np.float64) - want[3][sup])))
        derr = float(np.max(np.abs(stats[k, :more, 3] / np.array(want[2]) - 1)))
        worst = [max(a, b) for a, b in zip(worst, (rms, dg, derr))]
    print(f"[gsw variants] {label}: key {info['col_plan']} cw {info['col_cw']} threads {info['col_threads']} "
          f"{info['precision']} layout {info['layout']} p={refs[0]['p']}: phase rms {worst[0]:.3e}, "
          f"max |dg| {worst[1]:.3e}, error curve max rel {worst[2]:.3e}")
    for k, r in enumerate(refs):
        sup = r["t"] > 0
        lo, hi = r["factors"]
        # the kernels clamp the update factor to [2^-64, 2^64]: idle on these inputs
        assert 2.0 ** -64 < lo <= hi < 2.0 ** 64, (lo, hi)
        assert orc.phase_rms(phase[k], r["want"][0]) <= PHASE_RMS_TOL
        assert np.max(np.abs(g[k][sup].astype(np.float64) - r["want"][3][sup])) <= WEIGHT_TOL
        assert np.all(g[k][~sup] == 1.0)
        np.testing.assert_allclose(stats[k, :r["more"], 3], r["want"][2], rtol=ERR_RTOL)


def _parity(gpu, label, refs, prec, overrides, expect, repeats=1):
    """Run the warm-started plan of `refs` (one hologram each) and gate it;
    with repeats > 1 the further runs of the same plan must repeat the first
    bit for bit (where an LDS exchange race shows)."""
    t = np.stack([r["t"] for r in refs])
    ph0 = np.stack([r["ph0"] for r in refs])
    w0 = np.stack([r["w0"] for r in refs])
    more, p, ain = refs[0]["more"], refs[0]["p"], refs[0]["ain"]
    with _plan(gpu, t, more, p, ph0, w0, prec, ain, overrides, expect) as plan:
        info = plan.info()
        plan.run(more)
        first = _everything(plan)
        for _ in range(repeats - 1):
            plan.run(more)
            _assert_bitwise(first, _everything(plan))
    _gate(label, refs, first[0], first[4], first[2], info)
    return first


# dtype with its default precision first, then the other one
COMBOS = [(np.uint8, "f64"), (np.float32, "f32"), (np.uint8, "f32"), (np.float32, "f64")]
_COMBO_IDS = [f"{np.dtype(d).name}-{p}" for d, p in COMBOS]


# ---------------------------------------------------------------------------
# 1. every column plan key
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,prec", COMBOS, ids=_COMBO_IDS)
@pytest.mark.parametrize("key", sorted(KEYS), ids=_key_id)
def test_every_plan_key(gpu, key, dtype, prec):
    """Each of the 14 column keys of kPlans at its default tile width, forced
    with SLM_COL_PLAN where the length has two variants, at both precisions
    for both target types."""
    n, variant, _ = KEYS[key]
    _parity(gpu, f"plan {_key_id(key)} {np.dtype(dtype).name}", [_reference(n, W, dtype)], prec,
            dict(SLM_COL_PLAN=variant), _geometry(key, DEFAULT_CW[key], prec))


@pytest.mark.gpu
@pytest.mark.parametrize("key,dtype,prec", [(3, np.uint8, "f64"), (9, np.float32, "f32")],
                         ids=["key3-512wide-uint8-f64", "key9-512narrow-float32-f32"])
def test_plan_key_batch_of_three(gpu, key, dtype, prec):
    """Three different targets in one plan, one case per variant."""
    n, variant, _ = KEYS[key]
    refs = [_reference(n, W, dtype, seed=s) for s in (11, 12, 13)]
    _parity(gpu, f"batch 3 {_key_id(key)} {np.dtype(dtype).name}", refs, prec, dict(SLM_COL_PLAN=variant),
            _geometry(key, DEFAULT_CW[key], prec))


# ---------------------------------------------------------------------------
# 2. every tile width
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,prec", COMBOS[:2], ids=_COMBO_IDS[:2])
@pytest.mark.parametrize("key,cw", sorted(TILES), ids=[f"{_key_id(k)}-cw{c}-{TILES[(k, c)]}threads"
                                                       for k, c in sorted(TILES)])
def test_every_tile_width(gpu, key, cw, dtype, prec):
    """Every valid (key, cw) tile, forced with SLM_COL_CW: parity, and three
    runs of one plan equal bit for bit (phase, E, statistics, weights) -- the
    weighted pass adds a shared scale, a second workgroup fold and two barriers
    around the exchange LDS, on wave-local, 64-thread, 1024-thread and
    two-column-per-thread tiles alike."""
    n, variant, _ = KEYS[key]
    _parity(gpu, f"tile {_key_id(key)} {np.dtype(dtype).name}", [_reference(n, W, dtype)], prec,
            dict(SLM_COL_PLAN=variant, SLM_COL_CW=cw), _geometry(key, cw, prec), repeats=3)


@pytest.mark.gpu
def test_invalid_tile_width_is_not_taken(gpu):
    """A width without a kernel (4096 at cw 8: 272 KiB of LDS) falls back to
    the default tile, which info() shows: the assertion every case above
    relies on to notice an ignored override."""
    t = _target(4096, W, np.uint8)[None]
    with _plan(gpu, t, 2, overrides=dict(SLM_COL_PLAN="narrow", SLM_COL_CW=8)) as plan:
        info = plan.info()
    assert (info["col_plan"], info["col_cw"], info["col_threads"]) == (13, 2, 256), info


# ---------------------------------------------------------------------------
# 3. exponents
# ---------------------------------------------------------------------------
EXPONENTS = [0.3, 0.75, 1.25, 1.5]
_EXP_CASES = (
    [(64, np.uint8, prec, p) for p in EXPONENTS for prec in ("f32", "f64")] +
    [(512, np.float32, prec, p) for p in EXPONENTS for prec in ("f32", "f64")] +
    [(4096, np.uint8, "f64", 0.3), (4096, np.float32, "f32", 0.75), (4096, np.uint8, "f64", 1.25),
     (4096, np.float32, "f32", 1.5)])


@pytest.mark.gpu
@pytest.mark.parametrize("h,dtype,prec,p", _EXP_CASES,
                         ids=[f"{h}x64-{np.dtype(d).name}-{prec}-p{p}" for h, d, prec, p in _EXP_CASES])
def test_general_exponent(gpu, h, dtype, prec, p):
    """Exponents off the special-cased 0, 0.5 and 1: powf at f32, pow at f64.
    The reference asserts (in _gate) that the update factor stays inside the
    kernel's [2^-64, 2^64] clamp, so the clamp cannot bind unnoticed."""
    key = {64: 0, 512: 9, 4096: 13}[h]
    ref = _reference(h, W, dtype, p)
    lo, hi = ref["factors"]
    print(f"[gsw variants] p={p} {h}x64 {np.dtype(dtype).name}: update factor in [2^{np.log2(lo):.1f}, "
          f"2^{np.log2(hi):.1f}]")
    _parity(gpu, f"exponent {h}x64 {np.dtype(dtype).name}", [ref], prec, None,
            _geometry(key, DEFAULT_CW[key], prec))


@pytest.mark.gpu
@pytest.mark.parametrize("p", [2.0, 4.0])
@pytest.mark.parametrize("h", [64, 512])
def test_large_exponent_stays_finite(gpu, h, p):
    """p = 2 is no parity case: in the float64 reference itself a 1e-7
    perturbation of the warm start grows by 5e2 .. 2e7 over 20 iterations on
    these targets (p <= 1.5 shrinks it to 0.02 .. 0.08), so two correct
    implementations part ways. What must hold: phase and weights stay finite,
    weights positive."""
    t = _target(h, W, np.uint8)[None]
    with _plan(gpu, t, 50, p, _phi0(t.shape).astype(np.float32)) as plan:
        plan.run(50)
        phase = plan.read()[0]
        g = plan.read_weights()
    sup = t > 0
    print(f"[gsw variants] p={p} {h}x64 50 iterations: g in [{g[sup].min():.3e}, {g[sup].max():.3e}]")
    assert np.all(np.isfinite(phase)) and np.all(np.isfinite(g)) and np.all(g > 0)


# ---------------------------------------------------------------------------
# 4. incoming amplitude
# ---------------------------------------------------------------------------
# h, w, dtype, precision, p, column key, cw, layout, warm + further iterations, traps
_AIN_CASES = [
    (64, 64, np.uint8, "f64", 1.0, 0, 8, (4, 4), 30, 20, None),
    (512, 64, np.float32, "f32", 1.0, 9, 2, (4, 4), 30, 20, None),
    (512, 64, np.float32, "f32", 0.75, 9, 2, (4, 4), 30, 20, None),
    (4096, 64, np.uint8, "f64", 1.0, 13, 2, (4, 4), 30, 20, None),
    # the shuffle pair: 10 + 10 iterations and 40 traps, as the megapixel cases of test_gpu_gsw.py
    (1024, 1024, np.float32, "f32", 1.0, 11, 2, (8, 2), 10, 10, 40),
]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,dtype,prec,p,key,cw,layout,warm,more,nt", _AIN_CASES,
                         ids=[f"{c[0]}x{c[1]}-{np.dtype(c[2]).name}-{c[3]}-p{c[4]}" for c in _AIN_CASES])
def test_incoming_amplitude(gpu, h, w, dtype, prec, p, key, cw, layout, warm, more, nt):
    """has_ain plans against the reference's B = a_in exp(i angle(A)), at each
    plan's default precision and geometry."""
    ref = _reference(h, w, dtype, p, ain=1.0, warm=warm, more=more, nt=nt)
    expect = _geometry(key, cw, prec, layout)
    if (h, w) == (1024, 1024):
        expect["engine"] = ("shuffle", "shuffle")
    _parity(gpu, f"a_in {h}x{w} {np.dtype(dtype).name}", [ref], None, None, expect)


@pytest.mark.gpu
def test_incoming_amplitude_scaled_by_255(gpu):
    """a_in times 255 scales C by 255 and E by 255^2 (the statistics' stat_k
    scaling path); the normalised weights and the phase do not move."""
    ref = _reference(512, W, np.float32, 1.0, ain=1.0)
    lo, hi = ref["factors"]
    assert 2.0 ** -64 < lo / 255 and hi < 2.0 ** 64  # the scaled run's update factor, p = 1
    t, ph0, w0 = ref["t"][None], ref["ph0"][None], ref["w0"][None]
    out = []
    for scale in (1.0, 255.0):
        a = (np.float32(scale) * ref["ain"]).astype(np.float32)
        with _plan(gpu, t, 20, 1.0, ph0, w0, None, a, None, _geometry(9, 2, "f32")) as plan:
            plan.run(20)
            out.append(_everything(plan))
    rms = orc.phase_rms(out[1][0][0], out[0][0][0])
    rms_ref = orc.phase_rms(out[1][0][0], ref["want"][0])
    sup = t > 0
    dg = float(np.max(np.abs(out[1][4][sup].astype(np.float64) - out[0][4][sup])))
    print(f"[gsw variants] a_in x 255, 512x64 f32: phase rms {rms:.3e} against the unscaled run, {rms_ref:.3e} "
          f"against the reference; max |dg| {dg:.3e}")
    assert rms <= PHASE_RMS_TOL and rms_ref <= PHASE_RMS_TOL
    assert dg <= WEIGHT_TOL
    np.testing.assert_allclose(out[1][2][0, :20, 3], ref["want"][2], rtol=ERR_RTOL)


@pytest.mark.gpu
def test_feedback_zero_with_ain_is_gs(gpu):
    """feedback = 0 with an incoming amplitude is the GS plan with the same
    amplitude, bit for bit."""
    t = _target(512, W, np.uint8)[None]
    a = incoming_gauss(512, W)
    ph = _phi0(t.shape).astype(np.float32)
    with _plan(gpu, t, 20, phase=ph, ain=a, algo=gpu.ALGO_GS) as gs, _plan(gpu, t, 20, 0.0, ph, ain=a) as gsw:
        assert gs.info() == gsw.info()
        gs.run(20)
        gsw.run(20)
        _assert_bitwise(gs.read(), gsw.read())
        assert np.all(gsw.read_weights() == 1.0)


@pytest.mark.gpu
def test_run_gsw_with_ain_equals_plan(gpu):
    """The Python layer's run_gsw(t, loops, ain=a) is the has_ain plan's run."""
    from spatial_light_modulator_module_amd import algorithms as alg

    t = traps(128, 128, 16, 3, True)[None]
    a = incoming_gauss(128, 128)
    phase, e, errs, _, _, g = alg.run_gsw(t, 9, ain=a, return_weights=True)
    with _plan(gpu, t, 9, 1.0, ain=a) as plan:
        plan.run(9)
        want = _everything(plan)
    np.testing.assert_array_equal(phase, want[0])
    np.testing.assert_array_equal(e, want[1])
    np.testing.assert_array_equal(errs[0], want[2][0, :, 3])
    np.testing.assert_array_equal(g, want[4])
    # and the amplitude is in use: the uniform run differs
    assert not np.array_equal(phase, alg.run_gsw(t, 9)[0])


# ---------------------------------------------------------------------------
# 5. bitwise invariances
# ---------------------------------------------------------------------------
def _random_start(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-np.pi, np.pi, shape).astype(np.float32), rng.uniform(0.5, 1.5, shape).astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,prec", COMBOS, ids=_COMBO_IDS)
def test_layout_pairs_bitwise(gpu, dtype, prec):
    """The narrow layout pair of a single 1024^2 hologram against the default
    pair: the weights live in layout X, whose panel width changes from 4 to 8;
    addresses move, arithmetic does not."""
    t = traps(1024, 1024, 40, 11, True).astype(dtype)[None]
    ph, w0 = _random_start(t.shape, 7)
    res = {}
    for lay, pair in (("narrow", (8, 2)), ("default", (4, 4))):
        with _plan(gpu, t, 10, 1.0, ph, w0, prec, None, dict(SLM_LAYOUT=lay), _geometry(11, 2, prec, pair)) as plan:
            plan.run(10)
            res[lay] = _everything(plan)
    _assert_bitwise(res["narrow"], res["default"])
    assert res["narrow"][4][t > 0].std() > 1e-4  # the weights did move


@pytest.mark.gpu
@pytest.mark.parametrize("h,key", [(256, 8), (2048, 12)])
def test_store_mode_bitwise(gpu, h, key):
    """Write-through against write-back field stores (SLM_WT; the default
    changes at 2048-point columns): the same values either way. info() does not
    report the store mode, so only the rest of the geometry is asserted."""
    t = _target(h, W, np.float32)[None]
    ph, w0 = _random_start(t.shape, h)
    res = []
    for wt in (0, 1):
        with _plan(gpu, t, 15, 1.0, ph, w0, "f32", None, dict(SLM_WT=wt), _geometry(key, 2, "f32")) as plan:
            plan.run(15)
            res.append(_everything(plan))
    _assert_bitwise(res[0], res[1])


@pytest.mark.gpu
@pytest.mark.parametrize("h,dtype", [(512, np.float32), (4096, np.uint8)])
def test_precision_change_on_live_plan(gpu, h, dtype):
    """set_precision on a weighted-GS plan that holds host-set phase and
    weights: every run equals a fresh plan of that precision, and going back
    gives the first result again (the weights plane survives the switch)."""
    t = _target(h, W, dtype)[None]
    ph, w0 = _random_start(t.shape, 3)
    fresh = {}
    for prec in ("f32", "f64"):
        with _plan(gpu, t, 12, 1.0, ph, w0, prec, expect=dict(precision=prec)) as plan:
            plan.run(12)
            fresh[prec] = (plan.info(),) + _everything(plan)
    with _plan(gpu, t, 12, 1.0, ph, w0, "f32") as plan:
        seen = []
        for prec in ("f32", "f64", "f32"):
            plan.set_precision(PREC[prec])
            assert plan.info() == fresh[prec][0]
            plan.run(12)
            seen.append(_everything(plan))
            _assert_bitwise(seen[-1], fresh[prec][1:])
    _assert_bitwise(seen[0], seen[2])
    assert not np.array_equal(seen[0][0], seen[1][0])  # the two precisions are two kernels


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,dtype,key,layout", [(1024, 1024, np.float32, 11, (8, 2)), (4096, 64, np.uint8, 13, (4, 4))],
                         ids=["2x1024x1024-float32", "2x4096x64-uint8"])
def test_stop_in_batch(gpu, h, w, dtype, key, layout):
    """test_stopped_hologram_keeps_its_weights's construction on the shuffle
    pair and on two-column-per-thread tiles: a tolerance stops one hologram of
    two at iteration k; its phase and weights are a solo run's of k + 1
    iterations, the other hologram's those of the unchecked run."""
    prec = "f32" if dtype == np.float32 else "f64"
    expect = _geometry(key, 2, prec, layout)
    # the second hologram is a dense target: no phase hologram gets near it, so its
    # error stays far above the tolerance that stops the trap hologram
    ts = np.stack([traps(h, w, 24, 4, True),
                   np.random.default_rng(5).integers(0, 256, (h, w), dtype=np.uint8)]).astype(dtype)
    ph = _phi0(ts.shape).astype(np.float32)
    loops = 12
    with _plan(gpu, ts, loops, 1.0, ph, expect=expect) as plan:
        plan.run(loops)
        free = _everything(plan)
        err = free[2][:, :, 3]
        # the first iteration k >= 1 whose error is a new minimum: a tolerance between
        # it and the earlier minimum stops hologram 0 right there
        # (the first such k whose tolerance also lies below every error of hologram 1)
        k, tol = next((i, 0.5 * (err[0, i] + err[0, :i].min())) for i in range(1, loops - 1)
                      if err[0, i] < err[0, :i].min() and 0.5 * (err[0, i] + err[0, :i].min()) < err[1].min())
        assert not np.any(err[1] <= tol), (k, tol, err)
        plan.run(loops, tol, True)
        phase, _, _, iters, g = _everything(plan)
    print(f"[gsw variants] stop in batch {ts.shape} {prec}: hologram 0 stopped after {iters[0]} of {loops}, "
          f"hologram 1 reports {iters[1]}")
    assert iters[0] == k + 1 and iters[1] == -1
    np.testing.assert_array_equal(phase[1], free[0][1])
    np.testing.assert_array_equal(g[1], free[4][1])
    with _plan(gpu, ts[:1], k + 1, 1.0, ph[:1], expect=expect) as solo:
        solo.run(k + 1)
        np.testing.assert_array_equal(solo.read()[0][0], phase[0])
        np.testing.assert_array_equal(solo.read_weights()[0], g[0])


@pytest.mark.gpu
def test_shards_equal_one_batch(gpu):
    """gs_multi with a feedback exponent (three shards on one device) against
    one five-hologram plan."""
    ts = np.stack([traps(128, W, 24, s, True) for s in range(5)])
    loops = 15
    phase, e, stats, _ = gpu.gs_multi(ts, loops, [0, 0, 0], feedback=1.0)
    with _plan(gpu, ts, loops, 1.0) as plan:
        plan.run(loops)
        want = plan.read()
    np.testing.assert_array_equal(phase, want[0])
    np.testing.assert_array_equal(e, want[1])
    np.testing.assert_array_equal(stats, want[2])
    assert not np.array_equal(phase, gpu.gs_multi(ts, loops, [0, 0, 0])[0])  # and it is not plain GS


# ---------------------------------------------------------------------------
# 6. GIF hand-off
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gif_chunks_hand_over_weights(gpu, tmp_path):
    """weighted_gerchberg_saxton with gif=True runs warm-started chunks that
    hand over float32 phase and mean-1 weights (not bitwise the one run): the
    hologram within the phase gate, the error curve within rtol 1e-4."""
    from spatial_light_modulator_module_amd.algorithms import weighted_gerchberg_saxton

    def args(gif):
        return argparse.Namespace(
            incomming_intensity="uniform", tolerance=0.0, max_loops=9, gif=gif, print_info=False, plot_error=False,
            learning_rate=0.005, white_attention=1.0, unsettle=0, initial_guess="random", random_seed=42,
            gif_type="h", gif_skip=4, gif_source_dir=str(tmp_path), correspond_to2pi=256, feedback=1.0)

    t = traps(128, 128, 16, 3, True)
    holo_gif, _, err_gif = weighted_gerchberg_saxton(t, args(True))
    assert sorted(os.listdir(tmp_path)) == ["0.png", "1.png", "2.png"]  # iterations 0, 4, 8
    holo, _, err = weighted_gerchberg_saxton(t, args(False))
    rms = orc.phase_rms(holo_gif, holo)
    derr = float(np.max(np.abs(np.array(err_gif) / np.array(err) - 1))) if len(err) == len(err_gif) else np.inf
    print(f"[gsw variants] GIF chunks 128x128, 9 loops, skip 4: phase rms {rms:.3e}, error curve max rel {derr:.3e}, "
          f"{len(err_gif)} and {len(err)} errors")
    assert len(err_gif) == len(err) == 9
    assert rms <= PHASE_RMS_TOL
    np.testing.assert_allclose(err_gif, err, rtol=ERR_RTOL)
