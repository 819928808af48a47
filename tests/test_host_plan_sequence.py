"""Host side of the image sequences (no device): run_sequence's argument
checks, the --chain flag of generate_hologram_sequence, and the shared cases
(deterministic, traps inside the image, a tolerance that gives mixed stops in
the float64 oracle chain)."""
import numpy as np
import pytest

import plan_sequence_cases as cases
from spatial_light_modulator_module_amd import algorithms as alg
from spatial_light_modulator_module_amd import generate_hologram_sequence as ghs


def test_run_sequence_refuses_bad_arguments_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("argument checks come before the plan")

    monkeypatch.setattr(alg, "get_plan", no_device)
    t = cases.trap_grid(3, 64, 64)
    tm, rm = cases.mraf_frames(3, 64, 64)
    for bad in (
        lambda: alg.run_sequence(t[0], 3, 3),                                    # one image is not a sequence
        lambda: alg.run_sequence(t[None, None], 3, 3),                           # five axes
        lambda: alg.run_sequence(t[:0], 3, 3),                                   # no frame
        lambda: alg.run_sequence(t, 0, 3),
        lambda: alg.run_sequence(t, 3, 0),
        lambda: alg.run_sequence(t, 2.5, 3),
        lambda: alg.run_sequence(t, 3, 3, "gradient_descent"),
        lambda: alg.run_sequence(t, 3, 3, tol=-1.0),
        lambda: alg.run_sequence(t, 3, 3, tol=float("nan")),
        lambda: alg.run_sequence(t, 3, 3, regions=np.ones_like(t)),              # regions without MRAF
        lambda: alg.run_sequence(t, 3, 3, ain=np.ones((64, 32), np.float32)),
        lambda: alg.run_sequence(t, 3, 3, initial_phase=np.zeros((32, 64))),
        lambda: alg.run_sequence(t, 3, 3, mask=np.zeros((64, 65))),
        lambda: alg.run_sequence(t, 3, 3, "weighted_gerchberg_saxton", feedback=-1.0),
        lambda: alg.run_sequence(cases.trap_grid(3, 60, 100), 3, 3, "weighted_gerchberg_saxton"),
        lambda: alg.run_sequence(cases.trap_grid(3, 60, 100), 3, 3, "mraf", regions=np.ones((3, 60, 100))),
        lambda: alg.run_sequence(tm, 3, 3, "mraf"),                              # MRAF needs regions
        lambda: alg.run_sequence(tm, 3, 3, "mraf", regions=rm[:2]),
        lambda: alg.run_sequence(tm, 3, 3, "mraf", regions=rm, mixing=0.0),
        lambda: alg.run_sequence(tm, 3, 3, "mraf", regions=rm, mixing=1.5),
    ):
        with pytest.raises(ValueError):
            bad()
    empty = rm.copy()
    empty[1] = 0
    with pytest.raises(ValueError, match="frame 1: the signal region of hologram 0"):
        alg.run_sequence(tm, 3, 3, "mraf", regions=empty)


def test_run_sequence_input_shapes_and_dtypes():
    t = cases.trap_grid(3, 64, 64)
    tdev, tt, algo, sr = alg._sequence_inputs(t, 3, 2, "gerchberg_saxton", 0.0, None, None, 1.0, 0.4, None, None)
    assert tdev.shape == (3, 1, 64, 64) and tdev.dtype == np.uint8 and tt == alg.TGT_U8 and algo == alg.ALGO_GS
    assert sr is None
    tdev, tt, _, _ = alg._sequence_inputs(cases.batch_of_two(t).astype(np.float64), 3, 2, "gerchberg_saxton", 0.0,
                                          None, None, 1.0, 0.4, None, None)
    assert tdev.shape == (3, 2, 64, 64) and tdev.dtype == np.float32 and tt == alg.TGT_F32
    tm, rm = cases.mraf_frames(3, 64, 64)
    _, _, algo, sr = alg._sequence_inputs(tm, 3, 2, "mraf", 0.0, None, None, 1.0, 0.4, rm * 7, None)
    assert algo == alg.ALGO_MRAF and sr.shape == (3, 1, 64, 64) and sr.dtype == bool
    np.testing.assert_array_equal(sr[:, 0], rm != 0)


def test_chain_flag_and_unchanged_defaults():
    a = ghs.build_parser().parse_args(["walk", "-v", "1", "-ct2pi", "255"])
    assert a.chain is False
    assert (a.max_loops, a.tolerance, a.preview, a.algorithm, a.feedback, a.incomming_intensity) == \
        (5, 0, False, "gerchberg_saxton", 1.0, "uniform")
    b = ghs.build_parser().parse_args(["walk", "-v", "1", "-ct2pi", "255", "--chain", "-loops", "7"])
    assert b.chain is True and b.max_loops == 7


def test_chains_are_runs_of_consecutive_equal_frames():
    frames = {i: np.zeros((4, 4), np.uint8) for i in range(7)}
    frames[3] = np.zeros((4, 5), np.uint8)
    frames[5] = np.zeros((4, 4), np.float32)
    assert list(ghs._chains(range(7), frames)) == [[0, 1, 2], [3], [4], [5], [6]]
    assert list(ghs._chains([0, 1, 4, 6], frames)) == [[0, 1], [4], [6]]
    assert list(ghs._chains([], frames)) == []


def test_cases_are_deterministic_and_keep_the_traps_inside():
    for h, w, n in ((64, 64, 6), (64, 768, 4), (128, 256, 5), (97, 101, 3), (60, 100, 3), (600, 800, 3),
                    (96, 128, 5), (768, 1024, 32), (1024, 1024, 32), (1080, 1920, 32)):
        assert n <= cases.max_frames(h, w)
        t = cases.trap_grid(n, h, w)
        np.testing.assert_array_equal(t, cases.trap_grid(n, h, w))
        assert t.dtype == np.uint8 and t.shape == (n, h, w)
        for f in range(n):
            assert np.count_nonzero(t[f]) == 12 and set(np.unique(t[f])) == {0, 255}
            if f:  # one pixel to the right per frame, no wrap
                np.testing.assert_array_equal(t[f][:, 1:], t[f - 1][:, :-1])
                assert not t[f][:, 0].any()
    assert cases.trap_grid(2, 64, 64, np.float32).dtype == np.float32
    two = cases.batch_of_two(cases.trap_grid(4, 128, 256))
    assert two.shape == (4, 2, 128, 256)
    np.testing.assert_array_equal(two[:, 1], np.roll(two[:, 0], (5, 9), axis=(1, 2)))
    t, r = cases.mraf_frames(6, 64, 64)
    t0, r0 = cases.shapes(64, 64)
    for f in range(6):
        np.testing.assert_array_equal(t[f], np.roll(t0, (f, 2 * f), axis=(0, 1)))
        np.testing.assert_array_equal(r[f], np.roll(r0, (f, 2 * f), axis=(0, 1)))
        assert np.any((r[f] > 0) & (t[f] > 0)) and np.any((r0 > 0) & (t[f] > 0))


def test_tolerance_gives_mixed_stops_in_the_oracle_chain():
    """tol: the geometric mean of two neighbouring values, more than 1 % apart,
    of frame 0's float64 error curve. In the float64 oracle chain hologram 0
    then stops early in every frame, and hologram 1 never comes within a
    factor of ten of the tolerance."""
    t, tol, n = cases.tolerance_targets(), cases.tolerance(), cases.TOL_LOOPS
    curve = cases.oracle_chain(t[:1], n, n, 0.0)[0][0]
    a, b = curve[cases.TOL_PAIR], curve[cases.TOL_PAIR + 1]
    assert min(a, b) < tol < max(a, b) and abs(a - b) > 0.01 * max(a, b)
    errs = cases.oracle_chain(t, n, n, tol)
    ran = np.array([[len(e) for e in frame] for frame in errs])
    assert np.all(ran[:, 0] < n) and ran[0, 0] == cases.TOL_PAIR + 2
    assert np.all(ran[:, 1] == n) and min(min(frame[1]) for frame in errs) > 10 * tol
