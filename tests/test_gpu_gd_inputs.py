"""GD on the float32 engine (kernels.hpp) with every input that can be indexed
or scheduled wrongly: a non-uniform incoming amplitude, white_attention != 1,
a learning rate that changes every iteration, and two different holograms per
batch, each held to its own float64 oracle run.

Common protocol: B = 2 targets uniform(0, 255) float32 (or integers uint8),
"random" initial fields (|x0| = 1: GD from them is not chaotic), one shared
a_in = sqrt(uniform(0.25, 2)), white_attention 2, six iterations at rates
0.005 * [1, 2, 0.5, 3, 1.5, 0.75]. Reference: oracle.fast_f64.
gradient_descent_f64 per hologram. Gates per hologram:

1. phase rms < 1e-5 (the project's float32 bar);
2. error curve rtol 1e-5 (fused / two-launch column side), 1e-4 (split);
3. expected output rtol 1e-3, atol 1e-4 * norm;
4. the field x itself, max|x_gpu - x_ref| / max|x_ref|, a per-pixel check an
   rms cannot hide: at most 4 x the same metric of the complex64 model
   (oracle.gs_gd_oracle.gradient_descent_c64: complex64 state, float32
   arithmetic, single-precision pocketfft) against the float64 oracle on the
   same inputs. Model and kernels round every stage to float32 in different
   butterfly orders, so their errors are of equal size and independent; the
   factor covers the tail of a maximum over up to 262,144 pixels.

test_inputs_discriminate (no GPU) keeps these inputs honest: every wrong
index or scalar they are meant to catch moves the float64 result by >= 1e-3
rad rms, 100 x gate 1.
"""
import argparse
import os
import types

import numpy as np
import pytest

from oracle import fast_f64
from oracle import gs_gd_oracle as orc

PHASE_RMS_TOL = 1e-5  # north_star: <= 1e-5 rms on the output phase
LOOPS = 6
RATES = 0.005 * np.array([1, 2, 0.5, 3, 1.5, 0.75])
WA = 2.0
MODEL_FACTOR = 4.0

# plan keys (csrc/plans.hpp, kPlans): what a small batch picks by default (the
# narrow variant where a length has one) and under SLM_PLAN=wide
DEFAULT_KEY = {64: 0, 128: 1, 256: 8, 512: 9, 768: 10, 1024: 11, 2048: 12, 4096: 13}
WIDE_KEY = {64: 0, 128: 1, 256: 2, 512: 3, 768: 4, 1024: 5, 2048: 6}


def field_err(x, ref):
    return float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


def make_inputs(h, w, u8=False, seed=None):
    """(targets [2][h][w], a_in [h][w] float32, x0 [2][h][w] complex128) of the common protocol."""
    from spatial_light_modulator_module_amd import algorithms as alg

    rng = np.random.default_rng([h, w, int(u8)] if seed is None else seed)
    if u8:
        t = rng.integers(0, 256, (2, h, w)).astype(np.uint8)
    else:
        t = rng.uniform(0, 255, (2, h, w)).astype(np.float32)
    ain = np.sqrt(rng.uniform(0.25, 2.0, (h, w))).astype(np.float32)
    x0 = np.stack([alg.make_initial_guess("random", None, t[k], 42 + k) for k in range(2)])
    return t, ain, x0


def oracle_run(t, x0, ain, loops=LOOPS, rates=RATES, wa=WA, tolerance=0.0):
    """(phase, output, errors, x) of the float64 oracle for one hologram."""
    ph, out, err, x = fast_f64.gradient_descent_f64(t, loops, rates, wa, initial_field=x0,
                                                    incoming_intensity=ain.astype(np.float64) ** 2,
                                                    tolerance=tolerance)
    return ph, out.copy(), np.asarray(err), x


_CASES = {}


def case(h, w, u8=False, seed=None):
    """Inputs, float64 oracle runs and complex64-model bounds of one shape:
    computed once for the module, shared by every test, read-only."""
    key = (h, w, u8, seed)
    if key not in _CASES:
        t, ain, x0 = make_inputs(h, w, u8, seed)
        ref, bound, model_rms = [], [], []
        for k in range(2):
            r = oracle_run(t[k], x0[k], ain)
            ph_m, _, _, x_m = orc.gradient_descent_c64(t[k], LOOPS, RATES, WA, initial_field=x0[k],
                                                       incoming_intensity=ain.astype(np.float64) ** 2)
            ref.append(tuple(_frozen(a) for a in r))
            bound.append(MODEL_FACTOR * field_err(x_m, r[3]))
            model_rms.append(orc.phase_rms(ph_m, r[0]))
        _CASES[key] = types.SimpleNamespace(h=h, w=w, u8=u8, t=_frozen(t), ain=_frozen(ain), x0=_frozen(x0), ref=ref,
                                            bound=bound, model_rms=model_rms)
    return _CASES[key]


def gd_run(lib, c, holograms=(0, 1), loops=LOOPS, rates=RATES, wa=WA, tol=0.0, checked=False, prec=None,
           timed=False, guess=True, max_loops=LOOPS):
    """One plan, one run of the holograms `holograms` of case c; everything the gates read."""
    sel = list(holograms)
    t = np.ascontiguousarray(c.t[sel])
    with lib.Plan(lib.ALGO_GD, len(sel), c.h, c.w, lib.TGT_U8 if c.u8 else lib.TGT_F32, True, max_loops) as p:
        if prec is not None:
            p.set_precision(prec)
        p.set_target(t)
        p.set_ain(c.ain)
        p.set_field(np.ascontiguousarray(c.x0[sel]) if guess else None)
        p.set_lr(np.asarray(rates, np.float32))
        cnt = None
        if timed:
            _, cnt = p.run_timed(loops, tol, checked, wa)
        else:
            p.run(loops, tol, checked, wa)
        ph, e, stats, iters = p.read()
        x = p.read_field()
        norm, _ = p.target_stats()
        return types.SimpleNamespace(ph=ph, e=e, stats=stats, iters=iters, x=x, norm=norm, info=p.info(), cnt=cnt,
                                     recoveries=p.gd_recoveries)


def check_hologram(label, c, k, r, j, curve_rtol):
    """Gates 1-4 of hologram k of case c, which is hologram j of run r."""
    from spatial_light_modulator_module_amd import algorithms as alg

    ref_ph, ref_out, ref_err, ref_x = c.ref[k]
    rms = orc.phase_rms(r.ph[j], ref_ph)
    ferr = field_err(r.x[j], ref_x)
    print(f"[parity] GD a_in/wa/rates {label} {c.h}x{c.w} hologram {k}: phase rms {rms:.3e} (complex64 model "
          f"{c.model_rms[k]:.3e}), field max err {ferr:.3e} (bound {c.bound[k]:.3e})")
    out = alg.expected_from(r.e[j], r.norm[j], r.stats[j, LOOPS - 1, 0])
    problems = []
    if not rms < PHASE_RMS_TOL:
        problems.append(f"phase rms {rms:.3e}")
    if not ferr <= c.bound[k]:
        problems.append(f"field max err {ferr:.3e} > {c.bound[k]:.3e}")
    assert not problems, f"{label} hologram {k}: " + "; ".join(problems)
    np.testing.assert_allclose(r.stats[j, :LOOPS, 3], ref_err, rtol=curve_rtol)
    np.testing.assert_allclose(out, ref_out, rtol=1e-3, atol=1e-4 * float(r.norm[j]))


def by_shape(*shapes):
    return pytest.mark.parametrize("shape", shapes, ids=[f"{h}x{w}" for h, w in shapes])


def keys_of(info):
    return info["col_plan"], info["row_plan"]


# ---------------------------------------------------------------------------
# host only: the inputs must discriminate
# ---------------------------------------------------------------------------
@by_shape((64, 128), (128, 64))
def test_inputs_discriminate(shape):
    """Each mistake the GPU tests are meant to catch -- a_in indexed one row or
    one column off or with a row pair swapped, the mask with white_attention
    1, the rate of a neighbouring iteration or a constant one, another
    hologram's target or field -- moves the float64 oracle's phase by at
    least 1e-3 rad rms after the six iterations of the protocol."""
    c = case(*shape)
    h, w = shape
    swapped = np.ascontiguousarray(c.ain.reshape(h // 2, 2, w)[:, ::-1]).reshape(h, w)
    mutations = {
        "a_in rolled one row": dict(ain=np.roll(c.ain, 1, axis=0)),
        "a_in rolled one column": dict(ain=np.roll(c.ain, 1, axis=1)),
        "a_in rows r, r^1 swapped": dict(ain=swapped),
        "white_attention 1": dict(wa=1.0),
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
            print(f"[inputs] {h}x{w} hologram {k}, {name}: {moved:.3e} rad rms")
            assert moved >= 1e-3, f"{name} moves hologram {k} by only {moved:.3e} rad rms"
    # and rounding x0 to the device's complex64 does not: four orders below
    ph, _, _, _ = oracle_run(c.t[0], c.x0[0].astype(np.complex64), c.ain)
    assert orc.phase_rms(ph, c.ref[0][0]) < 1e-6


# ---------------------------------------------------------------------------
# 1, 2: every line length on both axes, default and wide plans
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@by_shape((64, 128), (128, 64), (256, 512), (512, 256), (768, 128), (128, 768), (1024, 64), (64, 1024), (2048, 64),
          (64, 2048), (4096, 64), (64, 4096))
def test_gd_inputs_every_length_default_plans(gpu, shape):
    """The plan a small batch picks: narrow variants, the wave-shuffle pair on
    1024-point lines, and at 4096 the E = 16 key with two rows per thread
    (row pairs in 64-B sectors, lane_xor4) / two-line column tiles."""
    h, w = shape
    c = case(h, w)
    r = gd_run(gpu, c)
    info = r.info
    assert keys_of(info) == (DEFAULT_KEY[h], DEFAULT_KEY[w]), info
    assert info["precision"] == "f32" and info["layout"] == (4, 4), info
    col_engine, row_engine = info["engine"]
    assert col_engine == ("shuffle" if h == 1024 else "stockham"), info
    assert row_engine == ("shuffle" if w == 1024 else "stockham"), info
    if w == 4096:  # 256 threads carry a row pair: two rows per thread
        assert (info["rows_per_workgroup"], info["row_threads"]) == (2, 4096 // 16), info
    if h == 4096:  # 256 threads carry a 2-column tile: two lines per thread
        assert (info["col_cw"], info["col_threads"]) == (2, 4096 // 16), info
    assert r.recoveries == 0
    for k in range(2):
        check_hologram("default plan", c, k, r, k, 1e-5)


@pytest.mark.gpu
@by_shape((256, 512), (512, 256), (768, 128), (64, 1024), (1024, 64), (2048, 64))
def test_gd_inputs_wide_plans(gpu, shape, monkeypatch):
    h, w = shape
    c = case(h, w)
    monkeypatch.setenv("SLM_PLAN", "wide")  # read at plan creation; gd_run creates its own plan
    r = gd_run(gpu, c)
    assert keys_of(r.info) == (WIDE_KEY[h], WIDE_KEY[w]), r.info
    assert r.info["engine"] == ("stockham", "stockham"), r.info
    for k in range(2):
        check_hologram("wide plan", c, k, r, k, 1e-5)


# ---------------------------------------------------------------------------
# 3: the three column-side structures
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@by_shape((64, 128), (64, 1024), (768, 128), (64, 4096))
def test_gd_inputs_column_structures(gpu, shape, monkeypatch):
    """SLM_GD_MODE = fused (one column launch, grid max-barrier), two
    (statistics + gradient launches) and lin (split gradient, combined in the
    row launch): each against the oracle; fused and two bitwise equal."""
    from spatial_light_modulator_module_amd import _lib

    c = case(*shape)
    res = {}
    for mode in ("fused", "two", "lin"):
        with monkeypatch.context() as m:
            m.setenv("SLM_GD_MODE", mode)
            res[mode] = gd_run(gpu, c, timed=True)
    for mode, stats_launches in (("fused", 0), ("two", LOOPS), ("lin", 0)):
        cnt = res[mode].cnt
        assert cnt[_lib.KERNEL_GD_STATS] == stats_launches and cnt[_lib.KERNEL_COL_MAIN] == LOOPS, (mode, cnt)
        assert cnt[_lib.KERNEL_ROW_MAIN] == LOOPS and res[mode].recoveries == 0, (mode, cnt)
    for k in range(2):
        for mode in ("fused", "two", "lin"):
            check_hologram(mode, c, k, res[mode], k, 1e-4 if mode == "lin" else 1e-5)
        np.testing.assert_array_equal(res["fused"].ph[k], res["two"].ph[k])
        np.testing.assert_array_equal(res["fused"].x[k], res["two"].x[k])


# ---------------------------------------------------------------------------
# 4, 5: float64 butterflies, uint8 targets
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@by_shape((64, 128), (1024, 64), (64, 4096))
def test_gd_inputs_float64_butterflies(gpu, shape):
    """SLM_PRECISION_F64: the two-launch column side on float64 butterflies
    (complex64 state), Stockham plans on every length."""
    c = case(*shape)
    r = gd_run(gpu, c, prec=gpu.PRECISION_F64)
    assert r.info["precision"] == "f64" and r.info["engine"] == ("stockham", "stockham"), r.info
    for k in range(2):
        check_hologram("float64 butterflies", c, k, r, k, 1e-5)


@pytest.mark.gpu
@by_shape((128, 64), (64, 1024), (768, 128))
def test_gd_inputs_uint8_targets(gpu, shape):
    c = case(*shape, u8=True)
    r = gd_run(gpu, c)
    assert keys_of(r.info) == (DEFAULT_KEY[shape[0]], DEFAULT_KEY[shape[1]]), r.info
    for k in range(2):
        check_hologram("uint8 target", c, k, r, k, 1e-5)


# ---------------------------------------------------------------------------
# 6: batch equals single
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@by_shape((256, 512), (64, 1024))
def test_gd_batch_equals_single(gpu, shape):
    """Hologram k of the B = 2 run against the same hologram alone (same a_in,
    white_attention and rates, same plan keys): phases, field, |F|^2 and the
    statistics bit for bit -- the batch offsets (hoff, norm[b], the target
    offset, the per-hologram maximum) against no offsets at all."""
    c = case(*shape)
    both = gd_run(gpu, c)
    for k in range(2):
        one = gd_run(gpu, c, holograms=(k,))
        assert keys_of(one.info) == keys_of(both.info) and one.info["col_cw"] == both.info["col_cw"], (one.info,
                                                                                                       both.info)
        np.testing.assert_array_equal(both.ph[k], one.ph[0])
        np.testing.assert_array_equal(both.x[k], one.x[0])
        np.testing.assert_array_equal(both.e[k], one.e[0])
        np.testing.assert_array_equal(both.stats[k], one.stats[0])
        check_hologram("single", c, k, one, 0, 1e-5)


# ---------------------------------------------------------------------------
# 7: the device-side "fourier" guess with a_in
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@by_shape((128, 256), (64, 1024), (64, 4096))
def test_gd_fourier_guess_with_ain(gpu, shape):
    """set_field(None): ROW_GD_INIT_Y forms a_in exp(i angle(ifft2(sqrt T))).
    One iteration at rate 0 leaves that guess in the field (x -= 0 * dEdX), so
    it is compared directly -- relative l2 norm against the float64 formula,
    at most 4 x what the same formula in complex64 (scipy.fft.ifft2 on
    complex64) gives -- and the first error with the oracle's from that guess."""
    c = case(*shape)
    r = gd_run(gpu, c, loops=1, rates=[0.0], guess=False, max_loops=1)
    intensity = c.ain.astype(np.float64) ** 2
    for k in range(2):
        t64 = c.t[k].astype(np.float64)
        ref = orc.make_initial_guess("fourier", c.ain.astype(np.float64), t64, 0)
        model = orc.fourier_guess_c64(c.t[k], intensity)
        scale = np.linalg.norm(ref)
        got, bound = np.linalg.norm(r.x[k] - ref) / scale, MODEL_FACTOR * np.linalg.norm(model - ref) / scale
        print(f"[parity] GD fourier guess with a_in {shape[0]}x{shape[1]} hologram {k}: field rel l2 {got:.3e} "
              f"(bound {bound:.3e})")
        assert got <= bound
        _, _, err, _ = fast_f64.gradient_descent_f64(c.t[k], 1, [0.0], WA, initial_field=ref,
                                                     incoming_intensity=intensity)
        np.testing.assert_allclose(r.stats[k, 0, 3], err[0], rtol=1e-5)


# ---------------------------------------------------------------------------
# 8: tolerance stop with a_in
# ---------------------------------------------------------------------------
TOL_SEED, TOL_STOPS = 67, (2, 3)  # chosen on the CPU: the widest gap among seeds 0..119 with both stops inside the run


@pytest.mark.gpu
def test_gd_tolerance_stop_with_ain(gpu):
    """One tolerance, two holograms that stop at different iterations (after
    3 and 4 of 6). The tolerance is the midpoint of the gap that the two
    oracle curves leave between {errors still above} and {first errors
    below}; every one of those four errors is more than 1 % away from it
    (float32 statistics agree with the oracle to 1e-5), asserted here."""
    c = case(64, 128, seed=TOL_SEED)
    err = [c.ref[k][2] for k in range(2)]
    above = min(err[k][TOL_STOPS[k] - 1] for k in range(2))
    below = max(err[k][TOL_STOPS[k]] for k in range(2))
    tol = 0.5 * (above + below)
    assert below < 0.99 * tol and above > 1.01 * tol, (below, tol, above)
    for k in range(2):
        assert np.all(err[k][:TOL_STOPS[k]] > tol) and err[k][TOL_STOPS[k]] <= tol
    r = gd_run(gpu, c, tol=tol, checked=True)
    for k, s in enumerate(TOL_STOPS):
        n = s + 1
        assert r.iters[k] == n, (k, r.iters)
        ref = oracle_run(c.t[k], c.x0[k], c.ain, tolerance=tol)
        assert len(ref[2]) == n
        np.testing.assert_array_equal(ref[2], err[k][:n])  # the stopped oracle run is the prefix of the full one
        free = gd_run(gpu, c, loops=n)  # unchecked, exactly n iterations
        np.testing.assert_array_equal(r.ph[k], free.ph[k])
        np.testing.assert_array_equal(r.x[k], free.x[k])
        # the stopped run against the oracle stopped by the same tolerance; the bound
        # of gate 4 comes from the six-iteration model run, so it is not applied here
        rms = orc.phase_rms(r.ph[k], ref[0])
        print(f"[parity] GD a_in/wa/rates checked run 64x128 hologram {k} stops after {n}: phase rms {rms:.3e}")
        assert rms < PHASE_RMS_TOL
        np.testing.assert_allclose(r.stats[k, :n, 3], ref[2], rtol=1e-5)


# ---------------------------------------------------------------------------
# 9: the drop-in entry point
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gradient_descent_entry_with_incoming_image_and_unsettle(gpu, golden_dir):
    """gradient_descent(t, args) with an incoming-intensity image,
    white_attention 0.5 and unsettle 2 over 12 loops (the rate doubles after
    iterations 4, 8 and 12): a_in from the PNG and the unsettle schedule
    through set_lr, against the faithful restatement fed the same image.

    The image's intensity is 4..255 (mean 90) and the step in x scales with
    it, so the learning rate is 5e-5 ~ 0.005 / 90: the step size of the
    common protocol. At 0.005 the iteration is chaotic (the complex64 model
    ends 6e-5 rad rms from the float64 run after these 12 loops, at 5e-5
    1.5e-6), which no float32 path could hold to 1e-5."""
    from PIL import Image

    from spatial_light_modulator_module_amd.algorithms import gradient_descent

    png = os.path.join(golden_dir, "g8_incoming_128.png")
    t = np.random.default_rng(9).uniform(0, 255, (128, 128)).astype(np.float32)
    lr = 5e-5
    args = argparse.Namespace(incomming_intensity=png, tolerance=0.0, max_loops=12, gif=False, print_info=False,
                              plot_error=False, learning_rate=lr, white_attention=0.5, unsettle=2,
                              initial_guess="random", random_seed=42)
    holo, out, err = gradient_descent(t, args)
    ph_o, out_o, err_o, lr_o = orc.gradient_descent_faithful(t, 12, lr, 0.5, 2, incoming_intensity=np.array(
        Image.open(png)), initial_guess="random", random_seed=42)
    rms = orc.phase_rms(holo, ph_o)
    print(f"[parity] GD entry, incoming image, unsettle 2, 12 loops: phase rms {rms:.3e}")
    assert len(err) == 12
    assert rms < PHASE_RMS_TOL
    np.testing.assert_allclose(err, err_o, rtol=1e-4)
    np.testing.assert_allclose(out, out_o, rtol=1e-3, atol=1e-4 * float(t.max()))
    assert lr_o == lr * 8 and args.learning_rate == lr_o
