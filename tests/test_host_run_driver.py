"""The Python layer over libslm_hip, pinned without a device: _lib.Plan is a
recording fake, so every test here asserts which library calls algorithms.py
and generate_hologram_sequence.py make, in which order and with which
arguments, and what they build from the scripted read-backs: return values
(element types and nesting included), stdout, exceptions and files."""
import argparse
import collections
import os
import warnings
import zlib

import numpy as np
import pytest

from spatial_light_modulator_module_amd import _lib
from spatial_light_modulator_module_amd import algorithms as alg
from spatial_light_modulator_module_amd import generate_hologram_sequence as ghs
from spatial_light_modulator_module_amd import parallel
from spatial_light_modulator_module_amd._lib import ALGO_GD, ALGO_GS, ALGO_GSW, ALGO_MRAF, TGT_F32, TGT_U8

SETTERS = ("set_target", "set_target_stats", "set_ain", "set_phase", "set_field", "set_lr", "set_feedback",
           "set_weights", "set_region", "set_mixing", "run", "sequence", "close")
READERS = ("read", "read_weights", "read_efficiency", "read_field", "target_stats", "sequence_read")


def rec(v):
    """What the log keeps of an argument: scalars by value (and type), arrays
    by shape, dtype and a checksum."""
    if isinstance(v, np.ndarray):
        return ("array", v.shape, str(v.dtype), zlib.crc32(np.ascontiguousarray(v).tobytes()))
    if isinstance(v, np.generic):
        return (type(v).__name__, v.item())
    if isinstance(v, (list, tuple)):
        return tuple(rec(x) for x in v)
    return v


class Fake:
    """The log, the scripted read-backs (a queue per reader) and the scripted
    failures (an exception per call name; "Plan" is the constructor)."""

    def __init__(self):
        self.log = []
        self.returns = collections.defaultdict(list)
        self.raises = {}

    def script(self, name, *values):
        self.returns[name].extend(values)

    def call(self, name, args, kwargs):
        entry = (name,) + tuple(rec(a) for a in args)
        if kwargs:
            entry += (tuple(sorted((k, rec(v)) for k, v in kwargs.items())),)
        self.log.append(entry)
        if name in self.raises:
            raise self.raises[name]
        if name in READERS:
            assert self.returns[name], f"unscripted {name}()"
            return self.returns[name].pop(0)

    def plan(self, *ctor):
        self.call("Plan", ctor, {})
        return FakePlan(self, *ctor)

    def names(self, *wanted):
        return [e for e in self.log if e[0] in wanted]


class FakePlan:
    def __init__(self, fake, algo, batch, height, width, tgt_type, has_ain, max_loops):
        self.fake = fake
        self.algo, self.batch, self.height, self.width = algo, batch, height, width
        self.tgt_type, self.has_ain, self.max_loops = tgt_type, bool(has_ain), max_loops


def _method(name):
    def method(self, *args, **kwargs):
        return self.fake.call(name, args, kwargs)
    return method


for _name in SETTERS + READERS:
    setattr(FakePlan, _name, _method(_name))


@pytest.fixture
def fake(monkeypatch):
    f = Fake()
    monkeypatch.setattr(_lib, "Plan", f.plan)
    monkeypatch.setattr(alg, "_PLANS", collections.OrderedDict())
    monkeypatch.setattr(_lib, "release_caches", lambda: f.call("release_caches", (), {}))
    monkeypatch.delenv("SLM_ENGINE", raising=False)
    monkeypatch.delenv("SLM_GPUS", raising=False)
    return f


def assert_log(got, want):
    want = [tuple(rec(x) for x in e) for e in want]
    assert [repr(e) for e in got] == [repr(e) for e in want]


def assert_same(got, want):
    """Equal values of equal types, through tuples and lists; NaN equals NaN."""
    assert type(got) is type(want), (type(got), type(want))
    if isinstance(want, (tuple, list)):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert_same(g, w)
    elif isinstance(want, dict):
        assert list(got) == list(want)
        for key in want:
            assert_same(got[key], want[key])
    elif isinstance(want, np.ndarray):
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(got, want, equal_nan=want.dtype.kind in "fc")
    elif isinstance(want, (float, np.floating)):
        assert got == want or (np.isnan(got) and np.isnan(want))
    else:
        assert got == want


def f64(values):
    return [np.float64(v) for v in values]


def stats_of(errs, base=100.0):
    """Plan.read()'s stats [B][rows][4]: column 3 holds the errors, column 0 a
    max E that differs in every row of every hologram."""
    errs = np.asarray(errs, np.float64)
    b, rows = errs.shape
    s = np.empty((b, rows, 4), np.float64)
    s[..., 0] = base + 10 * np.arange(b)[:, None] + np.arange(rows)[None]
    s[..., 1], s[..., 2], s[..., 3] = -1.0, -2.0, errs
    return s


def images(seed, shape, lo=0.0, hi=50.0):
    return np.random.default_rng(seed).uniform(lo, hi, shape).astype(np.float32)


def target(n, dtype=np.float32, batch=1, seed=1):
    """Positive everywhere, with values float32 does not hold exactly where dtype is float64."""
    return np.random.default_rng(seed).uniform(0.1, 1.0, (batch, n, n)).astype(dtype)


def a_read(shape, errs, iters, seed=0, base=100.0):
    return (images(seed, shape, -3.0, 3.0), images(seed + 1, shape), stats_of(errs, base),
            np.asarray(iters, np.int32))


RATES = np.linspace(0.005, 0.011, 7)

# name -> (side, algorithm code, run(targets, loops, tol), run's fourth argument, the reader after read())
RUNNERS = {
    "gs": (8, ALGO_GS, lambda t, loops, tol: alg.run_gs(t, loops, tol), (), "target_stats"),
    "gsw": (64, ALGO_GSW, lambda t, loops, tol: alg.run_gsw(t, loops, 0.7, tol), (), "target_stats"),
    "mraf": (64, ALGO_MRAF, lambda t, loops, tol: alg.run_mraf(t, np.ones(t.shape, np.uint8), loops, 0.4, tol), (),
             "read_efficiency"),
    "gd": (8, ALGO_GD, lambda t, loops, tol: alg.run_gd(t, loops, RATES, 0.25, tol), (0.25,), "target_stats"),
}


def script_tail(fake, batch, loops=5, times=1):
    """The read-backs after read(): target_stats() and read_efficiency(); a run uses one of them."""
    norm = 7.0 + np.arange(batch, dtype=np.float64)
    eff = 0.5 + 0.01 * np.arange(batch * loops, dtype=np.float64).reshape(batch, loops)
    for _ in range(times):
        fake.script("target_stats", (norm, norm * 2))
        fake.script("read_efficiency", eff)
    return norm, eff


def norm_of(name, t, norm):
    """run_*'s norm: target_stats()'s, or for MRAF the host's maximum over the (full) region."""
    if name != "mraf":
        return norm
    return np.array([np.float64(x.max()) for x in t.astype(np.float32)])


# ---------------------------------------------------------------------------
# call order
# ---------------------------------------------------------------------------
def exact_stats(t):
    tf = t.astype(np.float64).reshape(t.shape[0], -1)
    return tf.max(axis=1), np.einsum("ij,ij->i", tf, tf)


def test_call_order_gs(fake):
    t = target(8, np.float64)
    ain, ph0 = images(3, (8, 8), 0.5, 1.0), images(4, (1, 8, 8), -3, 3)
    rd = a_read(t.shape, [[5, 4, 3, 2, 1]], [-1])
    fake.script("read", rd)
    norm, _ = script_tail(fake, 1)
    out = alg.run_gs(t, 5, 0.0, ain, ph0)
    assert_log(fake.log, [("Plan", ALGO_GS, 1, 8, 8, TGT_F32, True, 5), ("set_target", t.astype(np.float32)),
                          ("set_target_stats",) + exact_stats(t), ("set_ain", ain), ("set_phase", ph0),
                          ("run", 5, 0.0, False), ("read",), ("target_stats",)])
    assert_same(out, (rd[0], rd[1], [f64([5, 4, 3, 2, 1])], norm, np.array([104.0])))
    assert out[0] is rd[0] and out[1] is rd[1] and out[3] is norm


def test_call_order_gs_without_the_optional_calls(fake):
    t = (target(8) * 200).astype(np.uint8)
    fake.script("read", a_read(t.shape, [[5, 4, 3, 2, 1]], [-1]))
    script_tail(fake, 1)
    alg.run_gs(t, 5)
    assert_log(fake.log, [("Plan", ALGO_GS, 1, 8, 8, TGT_U8, False, 5), ("set_target", t), ("set_phase", None),
                          ("run", 5, 0.0, False), ("read",), ("target_stats",)])


def test_call_order_gsw(fake):
    t = target(64, np.float64)
    ain, ph0, w0 = images(3, (64, 64), 0.5, 1.0), images(4, t.shape, -3, 3), images(5, t.shape, 0.5, 2.0)
    rd = a_read(t.shape, [[5, 4, 3, 2, 1]], [-1])
    fake.script("read", rd)
    norm, _ = script_tail(fake, 1)
    out = alg.run_gsw(t, 5, 0.7, 0.0, ain, ph0, w0)
    assert_log(fake.log, [("Plan", ALGO_GSW, 1, 64, 64, TGT_F32, True, 5), ("set_target", t.astype(np.float32)),
                          ("set_target_stats",) + exact_stats(t), ("set_ain", ain), ("set_feedback", 0.7),
                          ("set_phase", ph0), ("set_weights", w0), ("run", 5, 0.0, False), ("read",),
                          ("target_stats",)])
    assert_same(out, (rd[0], rd[1], [f64([5, 4, 3, 2, 1])], norm, np.array([104.0])))


def test_call_order_mraf_never_sets_exact_stats(fake):
    t = target(64, np.float64)
    t[0, 0, 0] = 1.7  # the maximum lies outside the region
    region = np.zeros(t.shape, np.int16)
    region[0, 10:40, 10:40] = 3
    ain, ph0 = images(3, (64, 64), 0.5, 1.0), images(4, t.shape, -3, 3)
    rd = a_read(t.shape, [[5, 4, 3, 2, 1]], [-1])
    fake.script("read", rd)
    script_tail(fake, 1)
    out = alg.run_mraf(t, region, 5, 0.3, 0.0, ain, ph0)
    assert_log(fake.log, [("Plan", ALGO_MRAF, 1, 64, 64, TGT_F32, True, 5), ("set_target", t.astype(np.float32)),
                          ("set_region", region != 0), ("set_ain", ain), ("set_mixing", 0.3), ("set_phase", ph0),
                          ("run", 5, 0.0, False), ("read",), ("read_efficiency",)])
    assert not fake.names("set_target_stats", "target_stats")
    norm = np.array([np.float64(t.astype(np.float32)[0, 10:40, 10:40].max())])  # not the whole target's maximum
    assert norm[0] < t.astype(np.float32).max()
    assert_same(out, (rd[0], rd[1], [f64([5, 4, 3, 2, 1])], norm, np.array([104.0])))


def test_call_order_gd(fake):
    t = target(8, np.float64)
    ain = images(3, (8, 8), 0.5, 1.0)
    x0 = (images(4, t.shape, -1, 1) + 1j * images(5, t.shape, -1, 1)).astype(np.complex128)
    rd = a_read(t.shape, [[5, 4, 3, 2, 1]], [-1])
    fake.script("read", rd)
    norm, _ = script_tail(fake, 1)
    out = alg.run_gd(t, 5, RATES, 0.25, 0.0, ain, x0)
    assert_log(fake.log, [("Plan", ALGO_GD, 1, 8, 8, TGT_F32, True, 5), ("set_target", t.astype(np.float32)),
                          ("set_target_stats",) + exact_stats(t), ("set_ain", ain), ("set_field", x0),
                          ("set_lr", RATES.astype(np.float32)[:5]), ("run", 5, 0.0, False, 0.25), ("read",),
                          ("target_stats",)])
    assert_same(out, (rd[0], rd[1], [f64([5, 4, 3, 2, 1])], norm, np.array([104.0])))


def test_plans_are_cached_by_key_and_closed_by_clear_plans(fake):
    t = target(8)
    for _ in range(2):
        fake.script("read", a_read(t.shape, [[2, 1]], [-1]))
        script_tail(fake, 1, 2)
        alg.run_gs(t, 2)
    assert len(fake.names("Plan")) == 1
    alg.clear_plans()
    assert_log(fake.log[-2:], [("close",), ("release_caches",)])


# ---------------------------------------------------------------------------
# the speculative run (tol = 0) and the checked run (tol > 0)
# ---------------------------------------------------------------------------
def run_and_read_calls(fake):
    return fake.names("run", "read")


@pytest.mark.parametrize("name", sorted(RUNNERS))
def test_speculative_run_reruns_checked_when_a_hologram_should_have_stopped(fake, name):
    n, algo, run, extra, tail = RUNNERS[name]
    t = target(n)
    first = a_read(t.shape, [[4, 3, 0, 2, 1]], [-1], seed=10)
    second = a_read(t.shape, [[4, 3, 0, 9, 9]], [3], seed=20, base=500.0)
    fake.script("read", first, second)
    norm, eff = script_tail(fake, 1)
    out = run(t, 5, 0.0)
    assert_log(run_and_read_calls(fake), [("run", 5, 0.0, False) + extra, ("read",), ("run", 5, 0.0, True) + extra,
                                          ("read",)])
    assert_log(fake.log[-1:], [(tail,)])
    assert_same(out, (second[0], second[1], [f64([4, 3, 0])], norm_of(name, t, norm), np.array([502.0])))
    assert out[0] is second[0] and out[1] is second[1]


@pytest.mark.parametrize("name", sorted(RUNNERS))
def test_speculative_run_keeps_a_curve_that_only_ends_at_the_tolerance(fake, name):
    n, algo, run, extra, tail = RUNNERS[name]
    t = target(n)
    rd = a_read(t.shape, [[4, 3, 2, 1, 0]], [2])  # an unchecked run's iters are not looked at
    fake.script("read", rd)
    norm, _ = script_tail(fake, 1)
    out = run(t, 5, 0.0)
    assert_log(run_and_read_calls(fake), [("run", 5, 0.0, False) + extra, ("read",)])
    assert_same(out, (rd[0], rd[1], [f64([4, 3, 2, 1, 0])], norm_of(name, t, norm), np.array([104.0])))


@pytest.mark.parametrize("name", sorted(RUNNERS))
def test_speculative_run_reruns_on_a_nan_in_the_middle(fake, name):
    n, algo, run, extra, tail = RUNNERS[name]
    t = target(n)
    curve = [[4, np.nan, 2, 1, 0.5]]
    second = a_read(t.shape, curve, [2], seed=20)
    fake.script("read", a_read(t.shape, curve, [-1], seed=10), second)
    norm, _ = script_tail(fake, 1)
    out = run(t, 5, 0.0)
    assert_log(run_and_read_calls(fake), [("run", 5, 0.0, False) + extra, ("read",), ("run", 5, 0.0, True) + extra,
                                          ("read",)])
    assert_same(out, (second[0], second[1], [f64([4, np.nan])], norm_of(name, t, norm), np.array([101.0])))


@pytest.mark.parametrize("name", sorted(RUNNERS))
def test_speculative_run_of_a_batch_where_one_hologram_triggers(fake, name):
    n, algo, run, extra, tail = RUNNERS[name]
    t = target(n, batch=2)
    curves = [[5, 4, 3, 2, 1], [4, 3, 0, 2, 1]]
    second = a_read(t.shape, curves, [-1, 3], seed=20)
    fake.script("read", a_read(t.shape, curves, [-1, -1], seed=10), second)
    norm, _ = script_tail(fake, 2)
    out = run(t, 5, 0.0)
    assert_log(run_and_read_calls(fake), [("run", 5, 0.0, False) + extra, ("read",), ("run", 5, 0.0, True) + extra,
                                          ("read",)])
    assert_same(out, (second[0], second[1], [f64([5, 4, 3, 2, 1]), f64([4, 3, 0])], norm_of(name, t, norm),
                      np.array([104.0, 112.0])))


@pytest.mark.parametrize("name", sorted(RUNNERS))
def test_checked_run_truncates_at_iters(fake, name):
    n, algo, run, extra, tail = RUNNERS[name]
    t = target(n, batch=2)
    rd = a_read(t.shape, [[5, 4, 3, 2, 1], [4, 0.4, 0, 0, 0]], [-1, 2])
    fake.script("read", rd)
    norm, _ = script_tail(fake, 2)
    out = run(t, 5, 0.5)
    assert_log(run_and_read_calls(fake), [("run", 5, 0.5, True) + extra, ("read",)])
    assert_same(out, (rd[0], rd[1], [f64([5, 4, 3, 2, 1]), f64([4, 0.4])], norm_of(name, t, norm),
                      np.array([104.0, 111.0])))


# ---------------------------------------------------------------------------
# the optional last element of the result
# ---------------------------------------------------------------------------
def test_return_weights(fake):
    t = target(64)
    rd, weights = a_read(t.shape, [[3, 2, 1]], [-1]), images(9, t.shape, 0.5, 2.0)
    fake.script("read", rd)
    fake.script("read_weights", weights)
    norm, _ = script_tail(fake, 1, 3)
    out = alg.run_gsw(t, 3, return_weights=True)
    assert_log(fake.log[-4:], [("run", 3, 0.0, False), ("read",), ("target_stats",), ("read_weights",)])
    assert_log(fake.names("set_feedback", "set_weights"), [("set_feedback", 1.0), ("set_weights", None)])
    assert_same(out, (rd[0], rd[1], [f64([3, 2, 1])], norm, np.array([102.0]), weights))
    assert out[5] is weights


def test_return_efficiency_is_truncated_like_the_errors(fake):
    t = target(64, batch=2)
    rd = a_read(t.shape, [[5, 4, 3, 2, 1], [4, 0.4, 0, 0, 0]], [-1, 2])
    fake.script("read", rd)
    _, eff = script_tail(fake, 2)
    out = alg.run_mraf(t, np.ones(t.shape, np.uint8), 5, tol=0.5, return_efficiency=True)
    assert_log(fake.log[-3:], [("run", 5, 0.5, True), ("read",), ("read_efficiency",)])
    assert_same(out, (rd[0], rd[1], [f64([5, 4, 3, 2, 1]), f64([4, 0.4])], norm_of("mraf", t, None),
                      np.array([104.0, 111.0]), [f64(eff[0]), f64(eff[1, :2])]))


def test_return_field(fake):
    t = target(8)
    rd = a_read(t.shape, [[3, 2, 1]], [-1])
    field = (images(8, t.shape, -1, 1) + 1j * images(9, t.shape, -1, 1)).astype(np.complex64)
    fake.script("read", rd)
    fake.script("read_field", field)
    norm, _ = script_tail(fake, 1, 3)
    out = alg.run_gd(t, 3, RATES, 1.0, return_field=True)
    assert_log(fake.log[-6:], [("set_field", None), ("set_lr", RATES.astype(np.float32)[:3]),
                               ("run", 3, 0.0, False, 1.0), ("read",), ("target_stats",), ("read_field",)])
    assert_same(out, (rd[0], rd[1], [f64([3, 2, 1])], norm, np.array([102.0]), field))
    assert out[5] is field


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------
def slm_error(code):
    e = _lib.SlmError("scripted")
    e.code = code
    return e


FUSED_ONLY = ("{} runs on the fused engine only: both sides of the target must be one of 64, 128, 256, 512, 1024, "
              "2048, 4096 (powers of two) or 768, and $SLM_ENGINE=float64 must not be set")


def test_the_message_constants():
    assert alg.GSW_SHAPES == FUSED_ONLY.format("weighted Gerchberg-Saxton")
    assert alg.MRAF_SHAPES == FUSED_ONLY.format("MRAF")


@pytest.mark.parametrize("name,display", [("gsw", "weighted Gerchberg-Saxton"), ("mraf", "MRAF")])
def test_unsupported_from_the_constructor_becomes_the_shape_refusal(fake, name, display):
    run = RUNNERS[name][2]
    fake.raises["Plan"] = slm_error(_lib.ERR_UNSUPPORTED)
    with pytest.raises(ValueError) as info:
        run(target(64), 5, 0.0)
    assert str(info.value) == FUSED_ONLY.format(display) + " (got 64 x 64)"
    assert info.value.__cause__ is fake.raises["Plan"]
    assert [e[0] for e in fake.log] == ["Plan"]


@pytest.mark.parametrize("name", sorted(RUNNERS))
def test_another_code_from_the_constructor_passes_through(fake, name):
    run = RUNNERS[name][2]
    fake.raises["Plan"] = slm_error(_lib.ERR_HIP)
    with pytest.raises(_lib.SlmError) as info:
        run(target(RUNNERS[name][0]), 5, 0.0)
    assert info.value is fake.raises["Plan"]


@pytest.mark.parametrize("name", ["gs", "gd"])
def test_unsupported_passes_through_where_every_engine_takes_the_algorithm(fake, name):
    fake.raises["Plan"] = slm_error(_lib.ERR_UNSUPPORTED)
    with pytest.raises(_lib.SlmError) as info:
        RUNNERS[name][2](target(8), 5, 0.0)
    assert info.value is fake.raises["Plan"]


def test_bad_initial_weights(fake):
    fake.raises["set_weights"] = slm_error(_lib.ERR_ARG)
    with pytest.raises(ValueError) as info:
        alg.run_gsw(target(64), 5, initial_weights=np.zeros((1, 64, 64), np.float32))
    assert str(info.value) == "initial weights must be positive and finite wherever the target is > 0"
    assert info.value.__cause__ is fake.raises["set_weights"]
    assert fake.log[-1][0] == "set_weights" and not fake.names("run")
    fake.raises["set_weights"] = slm_error(_lib.ERR_STATE)
    with pytest.raises(_lib.SlmError) as info:
        alg.run_gsw(target(64), 5)
    assert info.value is fake.raises["set_weights"]


def test_fused_only_refusals_come_before_any_device_call(fake, monkeypatch):
    with pytest.raises(ValueError) as info:
        alg.run_gsw(target(8), 5, feedback=-1.0)  # the shape before the feedback
    assert str(info.value) == alg.GSW_SHAPES + " (got 8 x 8)"
    with pytest.raises(ValueError) as info:
        alg.run_gsw(target(64), 5, feedback=-1.0)
    assert str(info.value) == "feedback must be a finite number >= 0, got -1.0"
    with pytest.raises(ValueError) as info:
        alg.run_mraf(target(8), np.zeros((1, 8, 8)), 5, mixing=7)  # the shape before mixing and region
    assert str(info.value) == alg.MRAF_SHAPES + " (got 8 x 8)"
    with pytest.raises(ValueError) as info:
        alg.run_mraf(target(64), np.zeros((1, 64, 64)), 5, mixing=7)  # mixing before the region
    assert str(info.value) == "mixing must be in (0, 1], got 7.0"
    with pytest.raises(ValueError) as info:
        alg.run_mraf(target(64, batch=2), np.stack([np.ones((64, 64)), np.zeros((64, 64))]), 5)
    assert str(info.value) == "the signal region of hologram 1 holds no pixel with T > 0"
    with pytest.raises(ValueError) as info:
        alg.run_mraf(target(64)[0], np.ones((64, 64)), 5)
    assert str(info.value) == "targets must be [B][H][W], got shape (64, 64)"
    with pytest.raises(ValueError) as info:
        alg.run_mraf(target(64), np.ones((1, 64, 64)), 5, ain=np.ones((8, 8)))
    assert str(info.value) == "ain of shape (8, 8) does not match (64, 64)"
    with pytest.raises(ValueError) as info:
        alg.run_mraf(target(64), np.ones((1, 64, 64)), 5, initial_phase=np.ones((64, 64)))
    assert str(info.value) == "initial_phase of shape (64, 64) does not match (1, 64, 64)"
    monkeypatch.setenv("SLM_ENGINE", "float64")
    with pytest.raises(ValueError) as info:
        alg.run_gsw(target(64), 5)
    assert str(info.value) == alg.GSW_SHAPES + " (got 64 x 64)"
    with pytest.raises(ValueError) as info:
        alg.run_mraf(target(64), np.ones((1, 64, 64)), 5)
    assert str(info.value) == alg.MRAF_SHAPES + " (got 64 x 64)"
    assert fake.log == []


def test_sequence_inputs_refusals(fake):
    t = (target(64, batch=2) * 200).astype(np.uint8)
    ok = np.ones(t.shape, np.uint8)

    def refused(*a):
        with pytest.raises(ValueError) as info:
            alg._sequence_inputs(*a)
        return str(info.value)

    small = t[:, :8, :8]
    assert refused(small, 5, 5, "weighted_gerchberg_saxton", 0.0, None, None, -1.0, 0.4, None, None) \
        == alg.GSW_SHAPES + " (got 8 x 8)"
    assert refused(t, 5, 5, "weighted_gerchberg_saxton", 0.0, None, None, -1.0, 0.4, None, None) \
        == "feedback must be a finite number >= 0, got -1.0"
    assert refused(small, 5, 5, "mraf", 0.0, None, None, 1.0, 7, None, None) == alg.MRAF_SHAPES + " (got 8 x 8)"
    assert refused(t, 5, 5, "mraf", 0.0, None, None, 1.0, 7, None, None) == "mixing must be in (0, 1], got 7"
    assert refused(t, 5, 5, "mraf", 0.0, None, None, 1.0, 0.4, None, None) \
        == "an MRAF sequence needs the signal regions of its frames"
    assert refused(t, 5, 5, "mraf", 0.0, None, None, 1.0, 0.4, ok[:1], None) \
        == "regions of shape (1, 64, 64) do not match targets of shape (2, 64, 64)"
    bad = ok.copy()
    bad[1] = 0
    assert refused(t, 5, 5, "mraf", 0.0, None, None, 1.0, 0.4, bad, None) \
        == "frame 1: the signal region of hologram 0 holds no pixel with T > 0"
    assert refused(t, 5, 5, "gerchberg_saxton", 0.0, None, None, 1.0, 0.4, ok, None) \
        == "regions apply to algorithm 'mraf' only"
    assert refused(t, 0, 5, "gerchberg_saxton", 0.0, None, None, 1.0, 0.4, None, None) \
        == "loops_first must be an integer >= 1, got 0"
    assert refused(t, 5, 5, "gerchberg_saxton", -1.0, None, None, 1.0, 0.4, None, None) \
        == "tol must be finite and >= 0, got -1.0"
    assert refused(t, 5, 5, "simulated_annealing", 0.0, None, None, 1.0, 0.4, None, None).startswith(
        "unknown sequence algorithm 'simulated_annealing': one of ['gerchberg_saxton', 'mraf', ")
    tdev, tt, algo, sr = alg._sequence_inputs(t, 5, 5, "mraf", 0.0, None, None, 1.0, 0.4, ok * 5, None)
    assert tdev.shape == (2, 1, 64, 64) and tt == TGT_U8 and algo == ALGO_MRAF
    assert sr.dtype == bool and sr.shape == (2, 1, 64, 64) and sr.all()
    assert fake.log == []


# ---------------------------------------------------------------------------
# the reference-compatible entry points
# ---------------------------------------------------------------------------
def namespace(**kw):
    ns = argparse.Namespace(incomming_intensity="uniform", tolerance=0.0, max_loops=5, gif=False, print_info=False,
                            plot_error=False, initial_guess="random", random_seed=42, learning_rate=0.005,
                            white_attention=1, unsettle=0)
    vars(ns).update(kw)
    return ns


def picture(n):
    t = np.zeros((n, n), np.uint8)
    t[n // 4:n // 2, n // 4:n // 2 + 2] = 200
    t[1, 2] = 90
    return t


# name -> (entry point, side, the variable of the UnboundLocalError, the reader after read())
ENTRIES = {
    "gs": (lambda t, a: alg.gerchberg_saxton(t, a), 8, "expected_outcome", "target_stats"),
    "gsw": (lambda t, a: alg.weighted_gerchberg_saxton(t, a), 64, "expected_outcome", "target_stats"),
    "mraf": (lambda t, a: alg.mraf(t, a), 64, "expected_outcome", "read_efficiency"),
    "gd": (lambda t, a: alg.gradient_descent(t, a), 8, "output", "target_stats"),
}
LOOP_LINES = "".join(f"\rloop {i}/5" for i in range(1, 6)) + "\n"


def entry_norm(name, t, norm):
    if name != "mraf":
        return norm[0]
    return np.float64(t[alg.signal_region(t, 8) != 0].max())


@pytest.mark.parametrize("print_info", [False, True])
@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_point_result_and_stdout(fake, capsys, name, print_info):
    entry, n, _, tail = ENTRIES[name]
    t = picture(n)
    rd = a_read((1, n, n), [[5, 4, 3, 2, 1.5]], [-1])
    fake.script("read", rd)
    norm, _ = script_tail(fake, 1)
    args = namespace(print_info=print_info)
    out = entry(t, args)
    want = LOOP_LINES + ("\nerror: 1.5\nnumber of loops: 5\n" if print_info else "")
    if name == "gd" and print_info:
        want = "computing hologram\n" + want
    assert capsys.readouterr().out == want
    expected = rd[1][0].astype(np.float64)
    expected *= entry_norm(name, t, norm) / np.float64(104.0)
    assert_same(out, (np.clip(rd[0][0].astype(np.float64), -np.pi, np.pi), expected, f64([5, 4, 3, 2, 1.5])))
    assert fake.log[-1] == (tail,)
    assert args.learning_rate == 0.005


def test_entry_point_arguments_reach_the_plan(fake):
    """What each entry point hands down: (1, h, w) targets, the feedback, the
    default region and mixing, GD's start field, rates and white attention."""
    for name, extra in (("gs", {}), ("gsw", {"feedback": 0.6}), ("mraf", {"mixing": 0.7, "region_margin": 2}),
                        ("gd", {"white_attention": 3, "unsettle": 1, "max_loops": 4, "learning_rate": 0.25})):
        entry, n, _, _ = ENTRIES[name]
        loops = extra.get("max_loops", 5)
        fake.script("read", a_read((1, n, n), [list(range(loops + 1, 1, -1))], [-1]))
        script_tail(fake, 1, loops)
        entry(picture(n), namespace(**extra))
    t8, t64 = picture(8), picture(64)
    field = alg.make_initial_guess("random", np.ones((8, 8)), t8, 42)[None]
    rates = np.array([0.25, 0.25, 0.5, 0.5], np.float32)
    assert_log([e for e in fake.log if e[0] not in ("read", "target_stats", "read_efficiency")], [
        ("Plan", ALGO_GS, 1, 8, 8, TGT_U8, False, 5), ("set_target", t8[None]), ("set_phase", None),
        ("run", 5, 0.0, False),
        ("Plan", ALGO_GSW, 1, 64, 64, TGT_U8, False, 5), ("set_target", t64[None]), ("set_feedback", 0.6),
        ("set_phase", None), ("set_weights", None), ("run", 5, 0.0, False),
        ("Plan", ALGO_MRAF, 1, 64, 64, TGT_U8, False, 5), ("set_target", t64[None]),
        ("set_region", alg.signal_region(t64, 2)[None] != 0), ("set_mixing", 0.7), ("set_phase", None),
        ("run", 5, 0.0, False),
        ("Plan", ALGO_GD, 1, 8, 8, TGT_U8, False, 4), ("set_target", t8[None]), ("set_field", field),
        ("set_lr", rates), ("run", 4, 0.0, False, 3.0)])


@pytest.mark.parametrize("print_info", [False, True])
@pytest.mark.parametrize("zero", [{"max_loops": 0}, {"tolerance": float("inf")}])
@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_point_zero_iterations(fake, capsys, name, zero, print_info):
    entry, n, variable, _ = ENTRIES[name]
    args = namespace(print_info=print_info, **zero)
    with pytest.raises(UnboundLocalError) as info:
        entry(picture(n), args)
    assert str(info.value) == f"local variable '{variable}' referenced before assignment"
    error = "inf" if "tolerance" in zero else "1.0"
    want = f"\n\nerror: {error}\nnumber of loops: 0\n" if print_info else "\n"
    if name == "gd" and print_info:
        want = "computing hologram\n" + want
    assert capsys.readouterr().out == want
    assert fake.log == []


def test_gd_learning_rate_after_an_early_stop_with_unsettle(fake, capsys):
    t = picture(8)
    fake.script("read", a_read((1, 8, 8), [[6, 5, 4, 0.1, 0, 0]], [4]))
    script_tail(fake, 1, 6)
    args = namespace(max_loops=6, unsettle=1, tolerance=0.5)
    _, _, errors = alg.gradient_descent(t, args)
    assert_same(errors, f64([6, 5, 4, 0.1]))
    assert type(args.learning_rate) is float and args.learning_rate == 0.01  # doubled once, after iteration 3
    assert_log(fake.names("set_lr", "run"), [("set_lr", np.array([0.005] * 3 + [0.01] * 3, np.float32)),
                                              ("run", 6, 0.5, True, 1.0)])
    assert capsys.readouterr().out == "".join(f"\rloop {i}/6" for i in range(1, 5)) + "\n"


def test_gd_zero_division(fake, capsys):
    with pytest.raises(ZeroDivisionError) as info:
        alg.gradient_descent(picture(8), namespace(max_loops=2, unsettle=5, print_info=True))
    assert str(info.value) == "integer division or modulo by zero"
    assert capsys.readouterr().out == "computing hologram\n"
    with pytest.raises(UnboundLocalError):  # the zero-iteration exit comes first
        alg.gradient_descent(picture(8), namespace(max_loops=0, unsettle=5))
    assert fake.log == []


def test_order_of_refusals_mraf(fake, capsys):
    t = picture(8)  # not a fused shape
    with pytest.raises(ValueError) as info:
        alg.mraf(t, namespace(signal_region=np.ones((4, 4)), mixing=7))
    assert str(info.value) == "signal region of shape (4, 4) does not match the target's (8, 8)"
    with pytest.raises(ValueError) as info:
        alg.mraf(t, namespace(signal_region=np.zeros((8, 8)), mixing=7))
    assert str(info.value) == alg.MRAF_SHAPES + " (got 8 x 8)"
    with pytest.raises(UnboundLocalError):  # the shape is refused by the run, which zero iterations never reach
        alg.mraf(t, namespace(signal_region=np.zeros((8, 8)), mixing=7, max_loops=0))
    with pytest.raises(ValueError) as info:
        alg.mraf(t, namespace(region_margin=-1))
    assert str(info.value) == "region margin must be >= 0, got -1"
    with pytest.raises(ValueError) as info:
        alg.mraf(np.zeros((2, 8, 8)), namespace())
    assert str(info.value) == "too many values to unpack (expected 2): target has shape (2, 8, 8)"
    assert fake.log == []


def test_order_of_refusals_weighted_gs(fake):
    with pytest.raises(ValueError) as info:
        alg.weighted_gerchberg_saxton(picture(8), argparse.Namespace())  # no attribute of args is read
    assert str(info.value) == alg.GSW_SHAPES + " (got 8 x 8)"
    with pytest.raises(AttributeError, match="incomming_intensity"):
        alg.weighted_gerchberg_saxton(picture(64), argparse.Namespace(feedback="1"))
    with pytest.raises(ValueError, match="could not convert string to float"):  # the feedback before the intensity
        alg.weighted_gerchberg_saxton(picture(64), argparse.Namespace(feedback="p"))
    with pytest.raises(AttributeError, match="incomming_intensity"):  # GS and GD read it first
        alg.gerchberg_saxton(picture(8), argparse.Namespace())
    with pytest.raises(AttributeError, match="incomming_intensity"):
        alg.gradient_descent(picture(8), argparse.Namespace())
    assert fake.log == []


# ---------------------------------------------------------------------------
# GIF runs
# ---------------------------------------------------------------------------
def gif_namespace(tmp_path, **kw):
    return namespace(**{**dict(gif=True, max_loops=7, gif_skip=3, gif_type="h", gif_source_dir=str(tmp_path),
                                correspond_to2pi=256), **kw})


def script_chunks(fake, n, steps, iters=None):
    """One read per chunk; the error falls by one each iteration, from 20."""
    reads, at = [], 0
    for c, step in enumerate(steps):
        curve = [[20.0 - at - j for j in range(step)]]
        reads.append(a_read((1, n, n), curve, [-1] if iters is None else [iters[c]], seed=30 + c))
        fake.script("read", reads[-1])
        script_tail(fake, 1, step)
        at += step
    return reads


def saved(tmp_path):
    from PIL import Image

    return {name: np.array(Image.open(tmp_path / name)) for name in sorted(os.listdir(tmp_path))}


def as_l(values):
    from PIL import Image

    return np.array(Image.fromarray(values).convert("L"))


def test_gif_gs(fake, capsys, tmp_path):
    t = picture(8)
    reads = script_chunks(fake, 8, [1, 2, 1, 2, 1])
    hologram, expected, errors = alg.gerchberg_saxton(t, gif_namespace(tmp_path, print_info=True))
    want = [("Plan", ALGO_GS, 1, 8, 8, TGT_U8, False, 1), ("set_target", t[None]), ("set_phase", None),
            ("run", 1, 0.0, False), ("read",), ("target_stats",),
            ("Plan", ALGO_GS, 1, 8, 8, TGT_U8, False, 2)]
    for c, step in enumerate([2, 1, 2, 1]):
        want += [("set_target", t[None]), ("set_phase", reads[c][0]), ("run", step, 0.0, False), ("read",),
                 ("target_stats",)]
    assert_log(fake.log, want)
    frames = saved(tmp_path)
    assert sorted(frames) == ["0.png", "1.png", "2.png"]
    for name, c in (("0.png", 0), ("1.png", 2), ("2.png", 4)):
        ang = np.clip(reads[c][0][0].astype(np.float64), -np.pi, np.pi)
        assert np.array_equal(frames[name], as_l((ang + np.pi) * 256 / (2 * np.pi)))
    assert_same(errors, f64([20, 19, 18, 17, 16, 15, 14]))
    assert_same(hologram, np.clip(reads[4][0][0].astype(np.float64), -np.pi, np.pi))
    last = reads[4][1][0].astype(np.float64)
    last *= np.float64(7.0) / np.float64(100.0)
    assert_same(expected, last)
    assert capsys.readouterr().out == ("".join(f"\rloop {i}/7" for i in range(1, 8))
                                       + "\n\nerror: 14.0\nnumber of loops: 7\n")


def test_gif_intensity_frames_and_no_frames(fake, tmp_path):
    reads = script_chunks(fake, 8, [1, 2, 1, 2, 1])
    alg.gerchberg_saxton(picture(8), gif_namespace(tmp_path, gif_type="i"))
    frames = saved(tmp_path)
    assert sorted(frames) == ["0.png", "1.png", "2.png"]
    for name, c in (("0.png", 0), ("1.png", 2), ("2.png", 4)):
        e = reads[c][1][0].astype(np.float64)
        e *= np.float64(7.0) / np.float64(100.0 + [0, 1, 0, 1, 0][c])
        assert np.array_equal(frames[name], as_l(e))
    for name in frames:
        os.remove(tmp_path / name)
    script_chunks(fake, 8, [1, 2, 1, 2, 1])
    alg.gerchberg_saxton(picture(8), gif_namespace(tmp_path, gif_type="none"))
    assert saved(tmp_path) == {}


def test_gif_weighted_gs_hands_on_phase_and_weights(fake, tmp_path):
    t = picture(64)
    reads = script_chunks(fake, 64, [1, 2, 1, 2, 1])
    weights = [images(60 + c, (1, 64, 64), 0.5, 2.0) for c in range(5)]
    fake.script("read_weights", *weights)
    hologram, _, errors = alg.weighted_gerchberg_saxton(t, gif_namespace(tmp_path, feedback=0.6))
    want = []
    for c, step in enumerate([1, 2, 1, 2, 1]):
        if c < 2:
            want.append(("Plan", ALGO_GSW, 1, 64, 64, TGT_U8, False, step))
        want += [("set_target", t[None]), ("set_feedback", 0.6), ("set_phase", reads[c - 1][0] if c else None),
                 ("set_weights", weights[c - 1] if c else None), ("run", step, 0.0, False), ("read",),
                 ("target_stats",), ("read_weights",)]
    assert_log(fake.log, want)
    assert sorted(saved(tmp_path)) == ["0.png", "1.png", "2.png"]
    assert_same(errors, f64([20, 19, 18, 17, 16, 15, 14]))
    assert_same(hologram, np.clip(reads[4][0][0].astype(np.float64), -np.pi, np.pi))


def test_gif_mraf_hands_on_phase(fake, tmp_path):
    t = picture(64)
    reads = script_chunks(fake, 64, [1, 2, 1, 2, 1])
    alg.mraf(t, gif_namespace(tmp_path, mixing=0.7))
    region = alg.signal_region(t, 8)[None] != 0
    want = []
    for c, step in enumerate([1, 2, 1, 2, 1]):
        if c < 2:
            want.append(("Plan", ALGO_MRAF, 1, 64, 64, TGT_U8, False, step))
        want += [("set_target", t[None]), ("set_region", region), ("set_mixing", 0.7),
                 ("set_phase", reads[c - 1][0] if c else None), ("run", step, 0.0, False), ("read",),
                 ("read_efficiency",)]
    assert_log(fake.log, want)
    assert sorted(saved(tmp_path)) == ["0.png", "1.png", "2.png"]


def test_gif_gd_hands_on_field_and_rate_slices(fake, capsys, tmp_path):
    t = picture(8)
    reads = script_chunks(fake, 8, [1, 2, 1, 2, 1])
    fields = [(images(70 + c, (1, 8, 8), -1, 1) + 1j * images(80 + c, (1, 8, 8), -1, 1)).astype(np.complex64)
              for c in range(5)]
    fake.script("read_field", *fields)
    args = gif_namespace(tmp_path, unsettle=1, white_attention=2)
    hologram, output, errors = alg.gradient_descent(t, args)
    rates, after = alg.learning_rates(0.005, 7, 1)
    assert list(rates) == [0.005] * 4 + [0.01] * 3
    x0 = alg.make_initial_guess("random", np.ones((8, 8)), t, 42)[None]
    want, at = [], 0
    for c, step in enumerate([1, 2, 1, 2, 1]):
        if c < 2:
            want.append(("Plan", ALGO_GD, 1, 8, 8, TGT_U8, False, step))
        want += [("set_target", t[None]), ("set_field", fields[c - 1] if c else x0),
                 ("set_lr", rates[at:at + step].astype(np.float32)), ("run", step, 0.0, False, 2.0), ("read",),
                 ("target_stats",), ("read_field",)]
        at += step
    assert_log(fake.log, want)
    frames = saved(tmp_path)
    assert sorted(frames) == ["0.png", "1.png", "2.png"]
    for name, c in (("0.png", 0), ("1.png", 2), ("2.png", 4)):
        ang = np.angle(fields[c][0].astype(np.complex128))
        assert np.array_equal(frames[name], as_l((ang + np.pi) / (2 * np.pi) * 256))
    assert_same(errors, f64([20, 19, 18, 17, 16, 15, 14]))
    assert_same(hologram, np.clip(reads[4][0][0].astype(np.float64), -np.pi, np.pi))
    assert type(args.learning_rate) is float and args.learning_rate == 0.01 == float(after[7])
    assert capsys.readouterr().out == "".join(f"\rloop {i}/7" for i in range(1, 8)) + "\n"


@pytest.mark.parametrize("name", ["gs", "gd"])
def test_gif_stops_with_an_early_stop_in_the_second_chunk(fake, capsys, tmp_path, name):
    reads = script_chunks(fake, 8, [1, 2], iters=[-1, 1])
    fake.script("read_field", *[np.ones((1, 8, 8), np.complex64)] * 2)
    _, _, errors = ENTRIES[name][0](picture(8), gif_namespace(tmp_path, tolerance=0.5))
    assert_log(fake.names("run"), [("run", 1, 0.5, True) + ((1.0,) if name == "gd" else ()),
                                   ("run", 2, 0.5, True) + ((1.0,) if name == "gd" else ())])
    assert_same(errors, f64([20, 19]))
    assert sorted(saved(tmp_path)) == ["0.png"]
    assert capsys.readouterr().out == "\rloop 1/7\rloop 2/7\n"


def test_gif_stops_when_a_chunk_ends_at_the_tolerance(fake, tmp_path):
    script_chunks(fake, 8, [1, 2])
    _, _, errors = alg.gerchberg_saxton(picture(8), gif_namespace(tmp_path, tolerance=18.5))
    assert_same(errors, f64([20, 19, 18]))  # the device reported no early stop; the host's test ends the run
    assert len(fake.names("run")) == 2


# ---------------------------------------------------------------------------
# run_gs_multi
# ---------------------------------------------------------------------------
@pytest.fixture
def multi(fake, monkeypatch):
    def gs_multi(*args, **kwargs):
        fake.call("gs_multi", args, kwargs)
        return fake.returns["gs_multi"].pop(0)

    monkeypatch.setattr(_lib, "gs_multi", gs_multi)
    return fake


def test_gs_multi_result(multi):
    t = target(8, batch=2)
    rd = a_read(t.shape, [[5, 4, 3, 2, 1], [4, 0.4, 0, 0, 0]], [-1, 2])
    multi.script("gs_multi", rd)
    ain = images(3, (8, 8), 0.5, 1.0)
    out = alg.run_gs_multi(t, 5, [0, 1], 0.5, ain)
    assert_log(multi.log, [("gs_multi", t, 5, [0, 1], (("ain", ain), ("feedback", None), ("tol", 0.5)))])
    assert_same(out, (rd[0], rd[1], [f64([5, 4, 3, 2, 1]), f64([4, 0.4])],
                      t.reshape(2, -1).max(axis=1).astype(np.float64), np.array([104.0, 111.0])))


def test_gs_multi_float64_targets_fall_back_to_one_device(multi):
    t = target(8, np.float64, batch=2)
    rd = a_read(t.shape, [[2, 1], [3, 2]], [-1, -1])
    multi.script("read", rd)
    norm, _ = script_tail(multi, 2, 2)
    with pytest.warns(RuntimeWarning) as caught:
        out = alg.run_gs_multi(t, 2, [0, 1], 0.0)
    assert len(caught) == 1 and caught[0].filename == __file__
    assert str(caught[0].message) == (
        "float64 targets are not exact in float32: the batch runs on this process's one GPU (run_gs) so the error "
        "keeps its float64 terms; `devices` [0, 1] is ignored -- pass uint8 or float32 frames to shard them")
    assert_log(multi.log, [("Plan", ALGO_GS, 2, 8, 8, TGT_F32, False, 2), ("set_target", t.astype(np.float32)),
                           ("set_target_stats",) + exact_stats(t), ("set_phase", None), ("run", 2, 0.0, False),
                           ("read",), ("target_stats",)])
    assert_same(out, (rd[0], rd[1], [f64([2, 1]), f64([3, 2])], norm, np.array([101.0, 111.0])))
    multi.script("read", rd)
    script_tail(multi, 2, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        alg.run_gs_multi(t, 2, [1, 1], 0.0)  # one device: nothing is ignored, nothing to warn of


def test_gs_multi_feedback_goes_to_weighted_gs(multi):
    t = target(64, batch=2)
    rd = a_read(t.shape, [[2, 1], [3, 2]], [-1, -1])
    multi.script("gs_multi", rd)
    out = alg.run_gs_multi(t, 2, [0, 1], feedback=0.6)
    assert_log(multi.log, [("gs_multi", t, 2, [0, 1], (("ain", None), ("feedback", 0.6), ("tol", 0.0)))])
    assert_same(out[2], [f64([2, 1]), f64([3, 2])])
    with pytest.raises(ValueError) as info:
        alg.run_gs_multi(target(8, batch=2), 2, [0, 1], feedback=0.6)
    assert str(info.value) == alg.GSW_SHAPES + " (got 8 x 8)"
    assert len(multi.log) == 1
    t64 = target(64, np.float64, batch=2)
    multi.script("read", rd)
    script_tail(multi, 2, 2)
    with pytest.warns(RuntimeWarning):
        alg.run_gs_multi(t64, 2, [0, 1], 0.0, None, 0.6)
    assert_log(multi.names("Plan", "set_feedback", "run"),
               [("Plan", ALGO_GSW, 2, 64, 64, TGT_F32, False, 2), ("set_feedback", 0.6), ("run", 2, 0.0, False)])


# ---------------------------------------------------------------------------
# run_sequence
# ---------------------------------------------------------------------------
def a_sequence_read(f, b, n, rows, errs, iters, expected=False):
    shape = (f, b, n, n)
    stats = np.stack([stats_of(e, 100.0 * (i + 1)) for i, e in enumerate(errs)])
    assert stats.shape == (f, b, rows, 4)
    return ((images(1, shape, 0, 255)).astype(np.uint8), images(2, shape, -3, 3),
            images(3, shape) if expected else None, stats, None, np.asarray(iters, np.int32))


def test_sequence_gs(fake):
    t = (target(8, batch=3) * 200).astype(np.uint8)
    ain, ph0, mask = images(3, (8, 8), 0.5, 1.0), images(4, (1, 8, 8), -3, 3), np.ones((8, 8))
    rd = a_sequence_read(3, 1, 8, 4, [[[9, 8, 7, 6]], [[5, 0.4, 0, 0]], [[4, 3, 0, 0]]], [[-1], [2], [-1]], True)
    fake.script("sequence_read", rd)
    out = alg.run_sequence(t, 4, 2, tol=0.5, ain=ain, initial_phase=ph0, mask=mask, ct2pi=200, return_expected=True)
    assert_log(fake.log, [
        ("Plan", ALGO_GS, 1, 8, 8, TGT_U8, True, 4), ("set_ain", ain), ("set_phase", ph0),
        ("sequence", t[:, None], None, (("ct2pi", 200), ("expected", True), ("frames", True), ("loops", 2),
                                        ("loops_first", 4), ("mask", mask), ("phases", True),
                                        ("rule", _lib.QUANT_PIL), ("tol", 0.5))),
        ("sequence_read", (("expected", True), ("frames", True), ("phases", True)))])
    assert_same(out, (rd[1], rd[0], [[f64([9, 8, 7, 6])], [f64([5, 0.4])], [f64([4, 3])]],
                      t.reshape(3, 1, -1).max(axis=2).astype(np.float64), np.array([[103.0], [201.0], [301.0]]),
                      rd[2]))


def test_sequence_unchecked_ignores_iters(fake):
    t = (target(8, batch=4).reshape(2, 2, 8, 8) * 200).astype(np.uint8)
    rd = a_sequence_read(2, 2, 8, 3, [[[9, 8, 7], [6, 5, 4]], [[3, 2, 1], [2, 1, 0]]], [[1, -1], [0, 2]])
    fake.script("sequence_read", rd)
    out = alg.run_sequence(t, 2, 3)
    assert_log(fake.names("Plan", "sequence_read"), [("Plan", ALGO_GS, 2, 8, 8, TGT_U8, False, 3),
                                                     ("sequence_read", (("expected", False), ("frames", True),
                                                                        ("phases", True)))])
    assert len(out) == 5
    assert_same(out[2], [[f64([9, 8]), f64([6, 5])], [f64([3, 2, 1]), f64([2, 1, 0])]])
    assert_same(out[4], np.array([[101.0, 111.0], [202.0, 212.0]]))


def test_sequence_weighted_gs_and_mraf_setters_and_region_norm(fake):
    t = (target(64, batch=2) * 200).astype(np.uint8)
    t[:, 0, 0] = 255  # each frame's maximum lies outside the regions below
    fake.script("sequence_read", a_sequence_read(2, 1, 64, 2, [[[9, 8]], [[7, 6]]], [[-1], [-1]]))
    alg.run_sequence(t, 2, 2, "weighted_gerchberg_saxton", feedback=0.6)
    assert_log(fake.log[:4], [("Plan", ALGO_GSW, 1, 64, 64, TGT_U8, False, 2), ("set_feedback", 0.6),
                              ("set_phase", None),
                              ("sequence", t[:, None], None, (("ct2pi", 256), ("expected", False), ("frames", True),
                                                              ("loops", 2), ("loops_first", 2), ("mask", None),
                                                              ("phases", True), ("rule", _lib.QUANT_PIL),
                                                              ("tol", 0.0)))])
    del fake.log[:]
    regions = np.zeros(t.shape, np.uint8)
    regions[:, 10:40, 10:40] = 2
    fake.script("sequence_read", a_sequence_read(2, 1, 64, 2, [[[9, 8]], [[7, 6]]], [[-1], [-1]]))
    out = alg.run_sequence(t.astype(np.float64), 2, 2, "mraf", mixing=0.7, regions=regions)
    tdev = t.astype(np.float32)[:, None]
    assert_log(fake.log[:4], [("Plan", ALGO_MRAF, 1, 64, 64, TGT_F32, False, 2), ("set_mixing", 0.7),
                              ("set_phase", None),
                              ("sequence", tdev, regions[:, None] != 0,
                               (("ct2pi", 256), ("expected", False), ("frames", True), ("loops", 2),
                                ("loops_first", 2), ("mask", None), ("phases", True), ("rule", _lib.QUANT_PIL),
                                ("tol", 0.0)))])
    norm = tdev[:, :, 10:40, 10:40].reshape(2, 1, -1).max(axis=2).astype(np.float64)
    assert (norm < tdev.reshape(2, 1, -1).max(axis=2)).all()  # the maximum over the region, not the frame
    assert_same(out[3], norm)
    assert not fake.names("set_target_stats")  # a sequence's constant terms come from the float32 copy


# ---------------------------------------------------------------------------
# generate_hologram_sequence
# ---------------------------------------------------------------------------
def frame(i, shape=(8, 8)):
    return ((np.arange(shape[0] * shape[1]).reshape(shape) * 3 + i * 7) % 256).astype(np.uint8)


def batch_result(stack, loops):
    """What the patched run_* return for a batch: a function of the frames alone, so the test can ask again."""
    b = stack.shape[0]
    seed = int(stack.astype(np.int64).sum())
    phase, e = images(seed, stack.shape, -3.3, 3.3), images(seed + 1, stack.shape, 0, 300)
    errs = [f64([loops - j + k for j in range(loops - k % 2)]) for k in range(b)]
    return (phase, e, errs, stack.reshape(b, -1).max(axis=1).astype(np.float64),
            e.reshape(b, -1).max(axis=1).astype(np.float64) * 1.5)


@pytest.fixture
def sequence_dir(fake, monkeypatch, tmp_path):
    """images/moving_traps/seq of five frames, frame 2 of another shape, and
    the run_* the tool calls replaced by recorders."""
    from PIL import Image

    monkeypatch.chdir(tmp_path)
    for name, shapes in (("seq", [(8, 8), (8, 8), (8, 16), (8, 8), (8, 8)]), ("even", [(8, 8)] * 5)):
        os.makedirs(f"images/moving_traps/{name}")
        for i, shape in enumerate(shapes):
            Image.fromarray(frame(i, shape)).save(f"images/moving_traps/{name}/{i}.png")

    def run_gs(stack, loops, tol, ain):
        fake.call("run_gs", (stack, loops, tol, ain), {})
        return batch_result(stack, loops)

    def run_gsw(stack, loops, feedback, tol, ain):
        fake.call("run_gsw", (stack, loops, feedback, tol, ain), {})
        return batch_result(stack, loops)

    def run_gs_multi(stack, loops, devices, tol, ain, feedback):
        fake.call("run_gs_multi", (stack, loops, devices, tol, ain, feedback), {})
        return batch_result(stack, loops)

    def run_sequence(stack, loops_first, loops, algorithm, tol, ain, initial_phase, feedback, return_expected):
        fake.call("run_sequence", (stack, loops_first, loops, algorithm, tol, ain, initial_phase, feedback,
                                   return_expected), {})
        phase, e, errs, norm, emax = batch_result(stack, loops)
        return (phase[:, None], None, [[x] for x in errs], norm[:, None], emax[:, None], e[:, None])

    for f in (run_gs, run_gsw, run_gs_multi, run_sequence):
        monkeypatch.setattr(ghs, f.__name__, f)
    monkeypatch.setattr(parallel, "world", lambda: fake.call("world", (), {}) or (0, 1, 0))
    return tmp_path


def sequence_namespace(**kw):
    ns = argparse.Namespace(source_dir="seq", version="v1", incomming_intensity="uniform", correspond_to2pi=256,
                            tolerance=0.0, max_loops=3, preview=True, algorithm="gerchberg_saxton", feedback=1.5,
                            chain=False)
    vars(ns).update(kw)
    return ns


SEQ_SHAPES = [(8, 8), (8, 8), (8, 16), (8, 8), (8, 8)]


def check_outputs(root, capsys, errors, groups, source="seq", preview=True):
    """stdout, the .npy and preview files and the returned dict for frames run in `groups`."""
    out, want_errors = "", {}
    for idx in groups:
        shapes = SEQ_SHAPES if source == "seq" else [(8, 8)] * 5
        stack = np.stack([frame(i, shapes[i]) for i in idx])
        phase, e, errs, norm, emax = batch_result(stack, 3)
        for k, i in enumerate(idx):
            out += f"\rcreating {i}. hologram " + "".join(f"\rloop {j}/3" for j in range(1, len(errs[k]) + 1)) + "\n"
            want_errors[i] = errs[k]
            assert_same(np.load(root / f"holograms/{source}_v1_holograms/{i}.npy"),
                        np.clip(phase[k].astype(np.float64), -np.pi, np.pi))
            if preview:
                from PIL import Image

                expected = e[k].astype(np.float64)
                expected *= norm[k] / np.float64(emax[k])
                assert np.array_equal(np.array(Image.open(root / f"images/moving_traps/{source}_v1_preview/{i}.png")),
                                      as_l(expected))
    assert capsys.readouterr().out == out
    assert_same(errors, want_errors)
    assert list(errors) == sorted(errors)
    assert sorted(os.listdir(root / f"holograms/{source}_v1_holograms")) == [f"{i}.npy" for i in range(5)]
    assert sorted(os.listdir(root / f"images/moving_traps/{source}_v1_preview")) \
        == ([f"{i}.png" for i in range(5)] if preview else [])


def stacks(groups, source="seq"):
    shapes = SEQ_SHAPES if source == "seq" else [(8, 8)] * 5
    return [np.stack([frame(i, shapes[i]) for i in idx]) for idx in groups]


BATCHES = [[0, 1], [2], [3, 4]]


def test_sequence_tool_plain(fake, capsys, sequence_dir):
    errors = ghs.generate_hologram_sequence(sequence_namespace(), 0, 1)
    assert_log(fake.log, [("run_gs", s, 3, 0.0, None) for s in stacks(BATCHES)])
    check_outputs(sequence_dir, capsys, errors, BATCHES)


def test_sequence_tool_asks_the_launcher_and_skips_previews(fake, capsys, sequence_dir):
    errors = ghs.generate_hologram_sequence(sequence_namespace(preview=False, tolerance=0.5))
    assert_log(fake.log, [("world",)] + [("run_gs", s, 3, 0.5, None) for s in stacks(BATCHES)])
    check_outputs(sequence_dir, capsys, errors, BATCHES, preview=False)


def test_sequence_tool_batches_are_at_most_seq_batch_long(fake, capsys, sequence_dir, monkeypatch):
    monkeypatch.setattr(ghs, "SEQ_BATCH", 2)
    groups = [[0, 1], [2, 3], [4]]
    errors = ghs.generate_hologram_sequence(sequence_namespace(source_dir="even"), 0, 1)
    assert_log(fake.log, [("run_gs", s, 3, 0.0, None) for s in stacks(groups, "even")])
    check_outputs(sequence_dir, capsys, errors, groups, "even")


def test_sequence_tool_weighted(fake, capsys, sequence_dir):
    errors = ghs.generate_hologram_sequence(sequence_namespace(algorithm="weighted_gerchberg_saxton"), 0, 1)
    assert_log(fake.log, [("run_gsw", s, 3, 1.5, 0.0, None) for s in stacks(BATCHES)])
    check_outputs(sequence_dir, capsys, errors, BATCHES)


def test_sequence_tool_two_gpus(fake, capsys, sequence_dir, monkeypatch):
    monkeypatch.setenv("SLM_GPUS", "2")
    errors = ghs.generate_hologram_sequence(sequence_namespace(), 0, 1)
    assert_log(fake.log, [("run_gs_multi", s, 3, [0, 1], 0.0, None, None) for s in stacks(BATCHES)])
    check_outputs(sequence_dir, capsys, errors, BATCHES)
    del fake.log[:]
    ghs.generate_hologram_sequence(sequence_namespace(algorithm="weighted_gerchberg_saxton"), 0, 1)
    assert_log(fake.log, [("run_gs_multi", s, 3, [0, 1], 0.0, None, 1.5) for s in stacks(BATCHES)])
    del fake.log[:]
    ghs.generate_hologram_sequence(sequence_namespace(), 0, 2)  # under a launcher $SLM_GPUS is not read
    assert_log(fake.log, [("run_gs", s, 3, 0.0, None) for s in stacks([[0, 1], [2]])])


def test_sequence_tool_chain(fake, capsys, sequence_dir, monkeypatch):
    monkeypatch.setattr(ghs, "SEQ_CHAIN", 2)
    errors = ghs.generate_hologram_sequence(sequence_namespace(chain=True), 0, 1)
    assert_log(fake.log, [("run_sequence", s, 3, 3, "gerchberg_saxton", 0.0, None, None, 1.5, True)
                          for s in stacks(BATCHES)])
    check_outputs(sequence_dir, capsys, errors, BATCHES)


def test_sequence_tool_chain_pieces_continue_from_the_last_phase(fake, capsys, sequence_dir, monkeypatch):
    monkeypatch.setattr(ghs, "SEQ_CHAIN", 2)
    pieces = [[0, 1], [2, 3], [4]]
    errors = ghs.generate_hologram_sequence(
        sequence_namespace(chain=True, source_dir="even", algorithm="weighted_gerchberg_saxton"), 0, 1)
    ss = stacks(pieces, "even")
    last = [None] + [batch_result(s, 3)[0][-1][None] for s in ss[:2]]
    assert_log(fake.log, [("run_sequence", s, 3, 3, "weighted_gerchberg_saxton", 0.0, None, p, 1.5, True)
                          for s, p in zip(ss, last)])
    check_outputs(sequence_dir, capsys, errors, pieces, "even")


@pytest.mark.parametrize("chain", [False, True])
@pytest.mark.parametrize("zero", [{"max_loops": 0}, {"tolerance": float("inf")}])
def test_sequence_tool_zero_iterations(fake, capsys, sequence_dir, chain, zero):
    with pytest.raises(UnboundLocalError) as info:
        ghs.generate_hologram_sequence(sequence_namespace(chain=chain, **zero), 0, 1)
    assert str(info.value) == "local variable 'expected_outcome' referenced before assignment"
    assert fake.log == [] and capsys.readouterr().out == ""


def test_batches_and_chains():
    frames = {i: np.zeros(s, d) for i, (s, d) in enumerate([((8, 8), np.uint8), ((8, 8), np.uint8),
                                                            ((8, 8), np.uint16), ((8, 8), np.uint16),
                                                            ((4, 8), np.uint16), ((4, 8), np.uint16)])}
    assert list(ghs._batches([0, 1, 2, 3, 4, 5], frames)) == [[0, 1], [2, 3], [4, 5]]
    assert list(ghs._chains([0, 1, 2, 3, 4, 5], frames)) == [[0, 1], [2, 3], [4, 5]]
    assert list(ghs._batches([0, 1, 3, 5], frames)) == [[0, 1], [3], [5]]
    assert list(ghs._batches([2, 3], frames)) == [[2, 3]] and list(ghs._batches([], frames)) == []
    same = {i: np.zeros((8, 8), np.uint8) for i in range(70)}
    assert list(ghs._batches([0, 2, 4], same)) == [[0, 2, 4]]  # a batch takes frames that are not neighbours
    assert list(ghs._chains([0, 2, 3, 5], same)) == [[0], [2, 3], [5]]  # a chain does not
    assert [len(r) for r in ghs._batches(range(70), same)] == [ghs.SEQ_BATCH, 70 - ghs.SEQ_BATCH]
    assert [len(r) for r in ghs._chains(range(70), same)] == [70]
