"""GD on the three any-size implementations -- the line engine (generic.hip:
k_gd_u, k_gd_stats, k_gd_grad, k_gd_update), the float64 mixed radix
(mr_inst.hip: RO_GD*, CO_GD_*) and the complex128 radix plans
(radix_c128.hpp) -- with every input that can be indexed or scheduled wrongly:
the protocol of test_gpu_gd_inputs.py (B = 2 targets, one non-uniform a_in,
white_attention 2, a learning rate that changes every iteration, "random"
fields of seeds 42 and 43), each hologram held to its own float64 oracle run
(oracle.fast_f64.gradient_descent_f64).

These engines compute in the oracle's own types (complex128 state, float64
arithmetic), so the oracle is fed exactly what the device receives -- the
field rounded to complex64 (it crosses the C-ABI in that type), the rates
rounded to float32, the float32 a_in -- and the gates are those of the
complex128 engines' GS tests, not the 1e-5 of a complex64 field start:

1. phase rms < 1e-6 (float32 phase output: its rounding is ~1e-7);
2. error curve rtol 1e-6;
3. expected output rtol 1e-6, atol 1e-6 * norm;
4. the field x per pixel, max|x_gpu - x_ref| / max|x_ref|, at most 4 x the same
   metric of x_ref.astype(complex64) against x_ref: the oracle's own rounding
   to the type read_field returns (3-5e-8); the factor covers the tail of a
   maximum over pixels. Computed from the oracle alone.

test_inputs_discriminate_any_size (no GPU) keeps the inputs honest at these
shapes: every wrong index or scalar moves the oracle by >= 1e-3 rad rms.

Every run asserts the engine, precision (and state layout) of its plan before
it runs, so that no case can pass on another back end.
"""
import argparse
import types

import numpy as np
import pytest
import scipy.fft as sfft

from oracle import fast_f64
from oracle import gs_gd_oracle as orc
from test_gpu_gd_inputs import LOOPS, RATES, WA, field_err, make_inputs

PHASE_RMS_TOL = 1e-6  # test_gpu_generic.py: complex128 engines, float32 phase output
CURVE_RTOL = 1e-6
ROUNDING_FACTOR = 4.0
# the tolerance-stop runs: the protocol's six rates, then two more
STOP_LOOPS = 8
STOP_RATES = 0.005 * np.array([1, 2, 0.5, 3, 1.5, 0.75, 1, 2])

KNOBS = ("SLM_MR_RPW", "SLM_MR_CW", "SLM_RZ_PLAN", "SLM_RZ_ROW_PLAN", "SLM_RZ_COL_PLAN", "SLM_RZ_CW",
         "SLM_RZ_LAYOUT", "SLM_RZ_PANEL", "SLM_ENGINE", "SLM_GENERIC_ENGINE", "SLM_PRECISION")

# back end -> (environment that selects it, engine name of the plan, state layout or None)
BACK_ENDS = {
    "mixed-radix": ({"SLM_GENERIC_ENGINE": "mr"}, "mixed-radix", None),
    "chirp-z": ({"SLM_GENERIC_ENGINE": "bluestein"}, "bluestein", None),  # chirp-z on both sides
    "lines": ({}, "bluestein", None),  # default selection: chirp-z on the prime side, direct on the other
    "radix-c128-b2": ({"SLM_ENGINE": "float64"}, "radix-c128", "b2"),
    "radix-c128-rm": ({"SLM_ENGINE": "float64", "SLM_RZ_LAYOUT": "rm"}, "radix-c128", "rm"),
    "radix-c128-panel": ({}, "radix-c128", "b2"),  # mixed plans on a panel: what GD picks by default
}
# (45, 77) = 3^2 5 x 7 11 and (26, 48) = 2 13 x 2^4 3: every radix of the mixed-radix kernels;
# 31 is prime; (600, 800) is the smallest SLM panel
CASES = [("mixed-radix", (45, 77)), ("mixed-radix", (26, 48)), ("chirp-z", (45, 77)), ("lines", (31, 44)),
         ("radix-c128-b2", (64, 128)), ("radix-c128-b2", (128, 64)), ("radix-c128-rm", (64, 128)),
         ("radix-c128-rm", (128, 64)), ("radix-c128-panel", (600, 800))]
ONE_EACH = [("mixed-radix", (45, 77)), ("chirp-z", (45, 77)), ("lines", (31, 44)), ("radix-c128-b2", (64, 128)),
            ("radix-c128-rm", (128, 64)), ("radix-c128-panel", (600, 800))]


def _ids(cases):
    return [f"{b}-{h}x{w}" for b, (h, w) in cases]


def _dtype(u8):
    return "u8" if u8 else "f32"


@pytest.fixture
def select(monkeypatch):
    """select(back_end) clears the engine's overrides and sets the ones that
    choose the back end (read at plan creation); returns (engine, layout)."""

    def set_(back_end):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        env, engine, layout = BACK_ENDS[back_end]
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        return engine, layout

    yield set_
    from spatial_light_modulator_module_amd import algorithms as alg

    alg.clear_plans()  # the drop-in's cached plans keep the engine they were created on


# ---------------------------------------------------------------------------
# inputs and references: computed once for the module, read-only
# ---------------------------------------------------------------------------
def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


def device_rates(rates):
    """The rates as the kernels read them: float32 (slm_plan_set_lr), widened."""
    return np.asarray(rates, np.float32).astype(np.float64)


def oracle_run(t, x0, ain, loops=LOOPS, rates=RATES, wa=WA, tolerance=0.0):
    """(phase, output, errors, x) of the float64 oracle for one hologram, fed
    what the device receives: x0 as complex64, the rates as float32, and the
    float32 a_in (the oracle takes its square, exact in float64, and the root
    of an exact square is exact)."""
    ph, out, err, x = fast_f64.gradient_descent_f64(t, loops, device_rates(rates), wa,
                                                    initial_field=np.asarray(x0).astype(np.complex64),
                                                    incoming_intensity=ain.astype(np.float64) ** 2,
                                                    tolerance=tolerance)
    return ph, out.copy(), np.asarray(err), x


_CASES = {}


def case(h, w, u8=False, seed=None, loops=LOOPS, rates=RATES):
    """Inputs of the common protocol at one shape, the oracle run of each
    hologram and the bound of gate 4."""
    key = (h, w, u8, seed, loops)
    if key not in _CASES:
        t, ain, x0 = make_inputs(h, w, u8, seed)
        ref, bound = [], []
        for k in range(2):
            r = oracle_run(t[k], x0[k], ain, loops, rates)
            ref.append(tuple(_frozen(a) for a in r))
            bound.append(ROUNDING_FACTOR * field_err(r[3].astype(np.complex64), r[3]))
        _CASES[key] = types.SimpleNamespace(h=h, w=w, u8=u8, t=_frozen(t), ain=_frozen(ain), x0=_frozen(x0), ref=ref,
                                            bound=bound, loops=loops, rates=_frozen(np.array(rates)))
    return _CASES[key]


def gd_run(lib, c, engine, layout, holograms=(0, 1), loops=None, rates=None, wa=WA, tol=0.0, checked=False,
           guess=True, max_loops=None):
    """One plan, one run of the holograms `holograms` of case c on the back end
    the environment selects -- asserted before anything runs."""
    sel = list(holograms)
    loops = c.loops if loops is None else loops
    max_loops = c.loops if max_loops is None else max_loops
    rates = c.rates if rates is None else rates
    with lib.Plan(lib.ALGO_GD, len(sel), c.h, c.w, lib.TGT_U8 if c.u8 else lib.TGT_F32, True, max_loops) as p:
        gi = p.generic_info()
        assert p.engine() == (engine, engine) and gi["engine"] == engine and gi["precision"] == "f64", (p.engine(), gi)
        assert layout is None or gi["layout"] == layout, gi
        p.set_target(np.ascontiguousarray(c.t[sel]))
        p.set_ain(c.ain)
        p.set_field(np.ascontiguousarray(c.x0[sel]) if guess else None)
        p.set_lr(np.asarray(rates, np.float32))
        p.run(loops, tol, checked, wa)
        ph, e, stats, iters = p.read()
        x = p.read_field()
        norm, _ = p.target_stats()
        return types.SimpleNamespace(ph=ph, e=e, stats=stats, iters=iters, x=x, norm=norm, gi=gi)


def check_hologram(label, c, k, r, j):
    """Gates 1-4 of hologram k of case c, which is hologram j of run r."""
    from spatial_light_modulator_module_amd import algorithms as alg

    ref_ph, ref_out, ref_err, ref_x = c.ref[k]
    n = c.loops
    rms = orc.phase_rms(r.ph[j], ref_ph)
    ferr = field_err(r.x[j], ref_x)
    curve = float(np.max(np.abs(r.stats[j, :n, 3] / ref_err - 1)))
    out = alg.expected_from(r.e[j], r.norm[j], r.stats[j, n - 1, 0])
    out_err = float(np.max(np.abs(out - ref_out) / (1e-6 * float(r.norm[j]) + 1e-6 * np.abs(ref_out))))
    print(f"[parity] GD a_in/wa/rates {label} {c.h}x{c.w} {_dtype(c.u8)} hologram {k}: phase rms {rms:.3e}, curve "
          f"{curve:.3e}, output {out_err:.3f} of its tolerance, field max err {ferr:.3e} (bound {c.bound[k]:.3e})")
    problems = []
    if not rms < PHASE_RMS_TOL:
        problems.append(f"phase rms {rms:.3e}")
    if not ferr <= c.bound[k]:
        problems.append(f"field max err {ferr:.3e} > {c.bound[k]:.3e}")
    assert not problems, f"{label} hologram {k}: " + "; ".join(problems)
    np.testing.assert_allclose(r.stats[j, :n, 3], ref_err, rtol=CURVE_RTOL)
    np.testing.assert_allclose(out, ref_out, rtol=1e-6, atol=1e-6 * float(r.norm[j]))


# ---------------------------------------------------------------------------
# host only: the inputs must discriminate
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True], ids=_dtype)
@pytest.mark.parametrize("shape", [(45, 77), (31, 44), (26, 48), (64, 128)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_inputs_discriminate_any_size(shape, u8):
    """Each mistake the GPU tests are meant to catch -- a_in indexed one row or
    one column off, the mask with white_attention 1 or 0, the rate of a
    neighbouring iteration or a constant one, another hologram's target or
    field -- moves the float64 oracle's phase by at least 1e-3 rad rms, 1000 x
    gate 1, after the six iterations of the protocol; feeding the oracle the
    unrounded field and rates instead moves it by less than a quarter of gate
    1 (6e-8 - 8e-8 measured)."""
    c = case(*shape, u8=u8)
    mutations = {
        "a_in rolled one row": dict(ain=np.roll(c.ain, 1, axis=0)),
        "a_in rolled one column": dict(ain=np.roll(c.ain, 1, axis=1)),
        "white_attention 1": dict(wa=1.0),
        "white_attention 0": dict(wa=0.0),
        "rates one iteration late": dict(rates=np.roll(RATES, 1)),
        "rates one iteration early": dict(rates=np.roll(RATES, -1)),
        "rates constant": dict(rates=np.full(LOOPS, RATES[0])),
        "targets exchanged": dict(other_t=True),
        "initial fields exchanged": dict(other_x=True),
    }
    for name, m in mutations.items():
        for k in range(2):
            t = c.t[1 - k] if m.get("other_t") else c.t[k]
            x0 = c.x0[1 - k] if m.get("other_x") else c.x0[k]
            ph, _, _, _ = oracle_run(t, x0, m.get("ain", c.ain), rates=m.get("rates", RATES), wa=m.get("wa", WA))
            moved = orc.phase_rms(ph, c.ref[k][0])
            print(f"[inputs] {shape[0]}x{shape[1]} {_dtype(u8)} hologram {k}, {name}: {moved:.3e} rad rms")
            assert moved >= 1e-3, f"{name} moves hologram {k} by only {moved:.3e} rad rms"
    for k in range(2):
        ph, _, _, _ = fast_f64.gradient_descent_f64(c.t[k], LOOPS, RATES, WA, initial_field=c.x0[k],
                                                    incoming_intensity=c.ain.astype(np.float64) ** 2)
        moved = orc.phase_rms(ph, c.ref[k][0])
        print(f"[inputs] {shape[0]}x{shape[1]} {_dtype(u8)} hologram {k}, unrounded field and rates: {moved:.3e} "
              f"rad rms")
        assert moved < 0.25 * PHASE_RMS_TOL


# ---------------------------------------------------------------------------
# 1: every back end against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("u8", [False, True], ids=_dtype)
@pytest.mark.parametrize("back_end,shape", CASES, ids=_ids(CASES))
def test_gd_inputs_any_size(gpu, select, back_end, shape, u8):
    """Gates 1-4 for both holograms; uint8 targets take the float64 mask
    1 + wa T / 255, float32 targets numpy's float32 one."""
    engine, layout = select(back_end)
    c = case(*shape, u8=u8)
    r = gd_run(gpu, c, engine, layout)
    assert (r.iters == -1).all() or (r.iters == LOOPS).all(), r.iters
    for k in range(2):
        check_hologram(back_end, c, k, r, k)


# ---------------------------------------------------------------------------
# 2: batch equals single
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("u8", [False, True], ids=_dtype)
@pytest.mark.parametrize("back_end,shape", ONE_EACH, ids=_ids(ONE_EACH))
def test_gd_batch_equals_single_any_size(gpu, select, back_end, shape, u8):
    """Hologram k of the B = 2 run against the same hologram alone, on the
    same tiles and plan keys: phases, field, |F|^2 and the statistics bit for
    bit -- the batch offsets of field, target, norm[b], statistics rows and
    stop flags, and a_in read modulo the hologram, against no offsets at all."""
    engine, layout = select(back_end)
    c = case(*shape, u8=u8)
    both = gd_run(gpu, c, engine, layout)
    for k in range(2):
        one = gd_run(gpu, c, engine, layout, holograms=(k,))
        assert one.gi == both.gi, (one.gi, both.gi)
        np.testing.assert_array_equal(both.ph[k], one.ph[0])
        np.testing.assert_array_equal(both.x[k], one.x[0])
        np.testing.assert_array_equal(both.e[k], one.e[0])
        np.testing.assert_array_equal(both.stats[k], one.stats[0])
        check_hologram(f"{back_end} single", c, k, one, 0)


# ---------------------------------------------------------------------------
# 3: tolerance stop
# ---------------------------------------------------------------------------
# (seed, stop iteration of each hologram), chosen on the CPU: among seeds 0..199 the
# widest gap between {errors still above} and {first errors below} with one stop on
# an odd and one on an even iteration count (7 and 6 of 8), both before the last
# loop. The curves are not monotone (iteration 4 rises), so the stops sit late.
STOP_CASES = [("mixed-radix", (45, 77), 88, (6, 5)), ("chirp-z", (45, 77), 88, (6, 5)),
              ("radix-c128-b2", (64, 128), 125, (6, 5)), ("radix-c128-rm", (64, 128), 125, (6, 5))]


@pytest.mark.gpu
@pytest.mark.parametrize("back_end,shape,seed,stops", STOP_CASES, ids=_ids([s[:2] for s in STOP_CASES]))
def test_gd_tolerance_stop_any_size(gpu, select, back_end, shape, seed, stops):
    """One tolerance, two holograms that stop after different counts. The
    tolerance is the midpoint of the gap the two oracle curves leave between
    {every error before the stop} and {the errors at the stops}; each of those
    is more than 1 % away from it (the statistics agree with the oracle to
    1e-6), asserted here. The stopped hologram is frozen while the other goes
    on: iteration counts as the oracle stopped by the same tolerance, phase
    and field bit for bit those of an unchecked run of exactly that many
    iterations (the update of the stopping iteration itself still applies,
    src/algorithms.py:83-92), gates 1 and 2 against the stopped oracle."""
    engine, layout = select(back_end)
    c = case(*shape, seed=seed, loops=STOP_LOOPS, rates=STOP_RATES)
    err = [c.ref[k][2] for k in range(2)]
    above = min(float(err[k][:stops[k]].min()) for k in range(2))
    below = max(float(err[k][stops[k]]) for k in range(2))
    tol = 0.5 * (above + below)
    assert below < 0.99 * tol and above > 1.01 * tol, (below, tol, above)
    counts = [s + 1 for s in stops]
    assert counts[0] % 2 != counts[1] % 2 and max(counts) < STOP_LOOPS, counts
    r = gd_run(gpu, c, engine, layout, tol=tol, checked=True)
    for k, n in enumerate(counts):
        assert r.iters[k] == n, (k, r.iters)
        ref = oracle_run(c.t[k], c.x0[k], c.ain, STOP_LOOPS, STOP_RATES, tolerance=tol)
        assert len(ref[2]) == n
        np.testing.assert_array_equal(ref[2], err[k][:n])  # the stopped oracle run is the prefix of the full one
        free = gd_run(gpu, c, engine, layout, loops=n)  # unchecked, exactly n iterations
        np.testing.assert_array_equal(r.ph[k], free.ph[k])
        np.testing.assert_array_equal(r.x[k], free.x[k])
        rms = orc.phase_rms(r.ph[k], ref[0])
        ferr = field_err(r.x[k], ref[3])
        curve = float(np.max(np.abs(r.stats[k, :n, 3] / ref[2] - 1)))
        print(f"[parity] GD a_in/wa/rates {back_end} checked run {shape[0]}x{shape[1]} hologram {k} stops after {n}: "
              f"phase rms {rms:.3e}, curve {curve:.3e}, field max err {ferr:.3e}")
        assert rms < PHASE_RMS_TOL
        np.testing.assert_allclose(r.stats[k, :n, 3], ref[2], rtol=CURVE_RTOL)


# ---------------------------------------------------------------------------
# 4: the device-side "fourier" guess with a_in
# ---------------------------------------------------------------------------
def fourier_guess_f64(t, ain):
    """a_in exp(i angle(ifft2(sqrt T))) in float64 on the amplitude the
    reference transforms: numpy's sqrt(T), float32 for a float32 target and
    float16 for a uint8 one (src/algorithms.py:153-155; generic.hip g_amp),
    widened before anything else happens to it."""
    amp = np.sqrt(t).astype(np.float64)
    return ain.astype(np.float64) * np.exp(1j * np.angle(sfft.ifft2(amp)))


@pytest.mark.gpu
@pytest.mark.parametrize("u8", [False, True], ids=_dtype)
@pytest.mark.parametrize("back_end,shape", ONE_EACH, ids=_ids(ONE_EACH))
def test_gd_fourier_guess_with_ain_any_size(gpu, select, back_end, shape, u8):
    """set_field(None): the engine forms a_in exp(i angle(ifft2(sqrt T))) on
    the device (k_fourier, RO_GD_FOURIER). One iteration at rate 0 leaves that
    guess in the field (x -= 0 * dEdX), so read_field returns it: relative l2
    norm against the float64 formula at most 4 x that of the formula's own
    rounding to complex64, and the first error with the oracle's from the
    float64 guess at rtol 1e-6.

    The formula takes sqrt(T) in numpy's type for T, as the reference and the
    kernels do. With a float64 root instead the formula itself moves by
    1.0e-7 - 2.5e-7 (float32 targets) and 0.8e-3 - 1.5e-3 (uint8: a float16
    root) in this norm at these shapes (CPU check), as much as or more than
    the bound: the root's type belongs to the operation, not to its rounding."""
    engine, layout = select(back_end)
    c = case(*shape, u8=u8)
    r = gd_run(gpu, c, engine, layout, loops=1, rates=[0.0], guess=False, max_loops=1)
    for k in range(2):
        ref = fourier_guess_f64(c.t[k], c.ain)
        scale = np.linalg.norm(ref)
        got = np.linalg.norm(r.x[k] - ref) / scale
        bound = ROUNDING_FACTOR * np.linalg.norm(ref.astype(np.complex64) - ref) / scale
        _, _, err, _ = fast_f64.gradient_descent_f64(c.t[k], 1, [0.0], WA, initial_field=ref,
                                                     incoming_intensity=c.ain.astype(np.float64) ** 2)
        first = abs(r.stats[k, 0, 3] / err[0] - 1)
        print(f"[parity] GD fourier guess with a_in {back_end} {shape[0]}x{shape[1]} {_dtype(u8)} hologram {k}: field "
              f"rel l2 {got:.3e} (bound {bound:.3e}), first error {first:.3e}")
        assert got <= bound
        np.testing.assert_allclose(r.stats[k, 0, 3], err[0], rtol=CURVE_RTOL)


# ---------------------------------------------------------------------------
# 5: the drop-in entry point
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("back_end", ["mixed-radix", "chirp-z"])
def test_gradient_descent_entry_any_size_unsettle_and_tolerance(gpu, select, back_end):
    """gradient_descent(t, args) at 45 x 77 with white_attention 0.5, unsettle 2
    over 12 loops (the rate doubles after iterations 4, 8 and 12) and a
    tolerance the error curve crosses at its fifth iteration -- the first at
    the doubled rate -- so the run goes with device checks and stops there,
    against the faithful restatement on the same arguments. The float64 field
    of the guess crosses the C-ABI as complex64: the gates are those of
    test_generic_gd_vs_oracle, and the faithful restatement started from the
    rounded field stays within a tenth of them (asserted)."""
    from spatial_light_modulator_module_amd.algorithms import gradient_descent

    engine, _ = select(back_end)
    shape, lr, loops = (45, 77), 0.005, 12
    with gpu.Plan(gpu.ALGO_GD, 1, shape[0], shape[1], gpu.TGT_F32, False, loops) as p:  # the plan the entry creates
        assert p.engine() == (engine, engine) and p.generic_info()["precision"] == "f64", p.engine()
    t = np.random.default_rng(9).uniform(0, 255, shape).astype(np.float32)
    _, _, full, _ = orc.gradient_descent_faithful(t, loops, lr, 0.5, 2)
    full = np.array(full)
    stop = 4
    tol = float(0.5 * (full[:stop].min() + full[stop]))
    assert full[stop] < 0.99 * tol and full[:stop].min() > 1.01 * tol, (full, tol)
    ph_o, out_o, err_o, lr_o = orc.gradient_descent_faithful(t, loops, lr, 0.5, 2, tolerance=tol)
    assert len(err_o) == stop + 1 and lr_o == 2 * lr
    x0 = orc.make_initial_guess("random", None, t, 42)
    ph_c, _, err_c, _ = orc.gradient_descent_faithful(t, loops, lr, 0.5, 2, tolerance=tol,
                                                      initial_field=x0.astype(np.complex64))
    assert orc.phase_rms(ph_c, ph_o) < 1e-6
    np.testing.assert_allclose(err_c, err_o, rtol=1e-6)

    args = argparse.Namespace(incomming_intensity="uniform", tolerance=tol, max_loops=loops, gif=False,
                              print_info=False, plot_error=False, learning_rate=lr, white_attention=0.5, unsettle=2,
                              initial_guess="random", random_seed=42)
    holo, out, err = gradient_descent(t, args)
    assert len(err) == len(err_o)
    rms = orc.phase_rms(holo, ph_o)
    curve = float(np.max(np.abs(np.array(err) / np.array(err_o) - 1)))
    print(f"[parity] GD entry {back_end} 45x77, unsettle 2, tolerance stop after {len(err)} of 12: phase rms "
          f"{rms:.3e}, curve {curve:.3e}")
    assert rms < 1e-5
    np.testing.assert_allclose(err, err_o, rtol=1e-5)
    np.testing.assert_allclose(out, out_o, rtol=1e-5, atol=1e-5 * float(t.max()))
    assert args.learning_rate == lr_o
