"""Host-side checks of trap trajectories (no GPU): the float64 reference chain
(tests/spots_sequence_reference.py), the ValueErrors of
move_traps.trap_array_sequence that are raised before the device is touched,
and the argument parsing and file naming of the generate_trap_sequence CLI on
a stubbed trap_array_sequence."""
import os

import numpy as np
import pytest

import spots_reference as sr
import spots_sequence_reference as ssr
from spatial_light_modulator_module_amd import generate_trap_sequence as gts
from spatial_light_modulator_module_amd import move_traps as mt
from spatial_light_modulator_module_amd.algorithms import hologram_from


# ---------------------------------------------------------------------------
# 1. the reference chain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,m", [(45, 70, 5), (48, 80, 12)])
def test_same_list_chain_is_one_long_run(h, w, m):
    li = sr.trap_list(h, w, m, 3)
    frames = ssr.sequence_reference((h, w), [li] * 4, 5, 5)
    phase, v, stats, wt = sr.spots_reference((h, w), *li, loops=20)
    assert [fr[4] for fr in frames] == [5] * 4
    # the chain hands the phase on, the long run the field: the same to rounding
    np.testing.assert_allclose(np.concatenate([fr[2] for fr in frames]), stats, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(frames[-1][3], wt, rtol=1e-9)
    np.testing.assert_allclose(frames[-1][1], v, rtol=1e-9, atol=1e-9 * h * w)
    assert np.max(np.abs(np.angle(np.exp(1j * (frames[-1][0] - phase))))) <= 1e-8


def test_reference_tolerance_stop():
    h, w, m, tol = 45, 70, 5, 0.01
    lists = ssr.trajectory(h, w, m, 3, 6)
    frames = ssr.sequence_reference((h, w), lists, 30, 8, tol)
    full = ssr.sequence_reference((h, w), lists, 30, 8, 0.0)
    assert [fr[4] for fr in frames] == [2, 4, 4, 4, 4, 3]
    assert [fr[4] for fr in full] == [30, 8, 8, 8, 8, 8]
    for fr in frames:
        n = fr[4]
        assert fr[2].shape == (n, 4)
        # only the last iteration's incoming uniformity is at or under tol (or the count ran out)
        assert np.all(fr[2][:n - 1, 1] > tol)
    # a frame of the stopped chain is the same frame run for exactly that many iterations
    again = ssr.frame_reference((h, w), lists[1], frames[1][4], 0.0, 1.0, None, frames[0][0], frames[0][3])
    np.testing.assert_array_equal(again[0], frames[1][0])
    np.testing.assert_array_equal(again[3], frames[1][3])


def test_trajectory_moves_every_trap():
    lists = ssr.trajectory(96, 160, 33, 3, 3)
    y0, x0, z0, i0 = sr.trap_list(96, 160, 33, 3)
    np.testing.assert_array_equal(lists[0][0], y0)
    np.testing.assert_array_equal(lists[0][2], z0)
    step_y, step_x = lists[1][0] - lists[0][0], lists[1][1] - lists[0][1]
    assert np.all(np.abs(step_y) <= 0.3) and np.all(np.abs(step_x) <= 0.3) and np.all(step_y != 0)
    np.testing.assert_allclose(lists[2][0] - y0, 2 * step_y)
    np.testing.assert_allclose(lists[2][2], z0 * 1.1)
    np.testing.assert_array_equal(lists[2][3], i0)


# ---------------------------------------------------------------------------
# 2. ValueErrors of the Python layer, before any device call
# ---------------------------------------------------------------------------
def test_sequence_value_errors(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(mt, "_get_spots", no_device)
    ys, xs = np.zeros((3, 5)), np.zeros((3, 5))
    shape = (45, 70)
    with pytest.raises(ValueError):
        mt.trap_array_sequence(shape, np.zeros(5), np.zeros(5))  # no frame axis
    with pytest.raises(ValueError):
        mt.trap_array_sequence(shape, np.zeros((3, 0)), np.zeros((3, 0)))
    with pytest.raises(ValueError):
        mt.trap_array_sequence(shape, ys, np.zeros((3, 4)))
    with pytest.raises(ValueError):
        mt.trap_array_sequence(shape, ys, np.zeros((2, 5)))
    with pytest.raises(ValueError):
        mt.trap_array_sequence(shape, ys, xs, zs=np.zeros((3, 6)))
    with pytest.raises(ValueError):
        mt.trap_array_sequence(shape, ys, xs, intensity=np.ones(5))
    with pytest.raises(ValueError):
        mt.trap_array_sequence(shape, ys, xs, initial_weights=np.ones(4))
    with pytest.raises(ValueError):
        mt.trap_array_sequence(shape, ys, xs, initial_phase=np.zeros((45, 69)))
    with pytest.raises(ValueError):
        mt.trap_array_sequence(shape, ys, xs, mask=np.zeros((45, 71)))
    with pytest.raises(ValueError):
        mt.trap_array_sequence(shape, np.zeros((3, 2, 5)), np.zeros((3, 5)))  # a batch against one trajectory
    with pytest.raises(ValueError):
        mt.trap_array_sequence(shape, np.zeros((3, 2, 5)), np.zeros((3, 2, 5)), initial_weights=np.ones((3, 5)))


def test_resume_without_a_sequence_is_a_value_error():
    mt.clear_spots()
    ys, xs = np.zeros((3, 5)), np.zeros((3, 5))
    with pytest.raises(ValueError, match="resume"):
        mt.trap_array_sequence((45, 70), ys, xs, resume=True)
    with pytest.raises(ValueError, match="resume"):
        mt.trap_array_sequence((45, 70), ys, xs, resume=True, initial_weights=np.ones(5))
    assert not mt._SPOTS  # no handle was made


# ---------------------------------------------------------------------------
# 3. the CLI on a stubbed trap_array_sequence
# ---------------------------------------------------------------------------
def test_cli_arguments():
    a = gts.build_parser().parse_args(["walk", "-v", "7", "-ct2pi", "200"])
    assert (a.name, a.version, a.correspond_to2pi) == ("walk", "7", 200)
    assert (a.max_loops, a.first, a.tolerance, a.feedback) == (4, 30, 0.0, 1.0)
    assert a.shape == (1080, 1920) and a.incomming_intensity == "uniform" and a.preview is False
    a = gts.build_parser().parse_args(["walk", "-v", "a", "-ct2pi", "256", "-loops", "6", "-first", "12", "-tol",
                                       "0.01", "--feedback", "0.5", "--shape", "45x70", "-ii", "beam.png", "-p"])
    assert (a.max_loops, a.first, a.tolerance, a.feedback) == (6, 12, 0.01, 0.5)
    assert a.shape == (45, 70) and a.incomming_intensity == "beam.png" and a.preview is True
    for bad in (["walk", "-v", "7"], ["-v", "7", "-ct2pi", "200"], ["walk", "-ct2pi", "200"],
                ["walk", "-v", "7", "-ct2pi", "200", "--shape", "45"],
                ["walk", "-v", "7", "-ct2pi", "200", "--shape", "1x70"]):
        with pytest.raises(SystemExit):
            gts.build_parser().parse_args(bad)
    assert gts.output_dirs("walk", "7") == ("holograms/walk_7_holograms", "images/moving_traps/walk_7_preview")


@pytest.mark.parametrize("columns,preview", [(2, False), (4, True)])
def test_cli_files(tmp_path, monkeypatch, capsys, columns, preview):
    frames_n, m, shape = 3, 4, (6, 8)
    rng = np.random.default_rng(1)
    traj = rng.uniform(-1, 1, (frames_n, m, columns))
    if columns == 4:
        traj[:, :, 3] = rng.uniform(0.5, 1.0, (frames_n, m))
    os.makedirs(tmp_path / "images" / "moving_traps")
    np.save(tmp_path / "images" / "moving_traps" / "walk.npy", traj.astype(np.float32))
    monkeypatch.chdir(tmp_path)
    phases = rng.uniform(-np.pi, np.pi, (frames_n,) + shape).astype(np.float32).astype(np.float64)
    phases[0, 0, 0] = float(np.float32(np.pi))  # rounds above pi: hologram_from clips it
    levels = rng.integers(0, 256, (frames_n,) + shape, dtype=np.uint8)
    stats = np.zeros((frames_n, 5, 4))
    stats[:, :, 1] = rng.uniform(0.01, 0.1, (frames_n, 5))
    iters = np.array([5, 2, 3], np.int32)
    seen = {}

    def stub(shape_, ys, xs, zs=None, intensity=None, **kw):
        seen.update(kw, shape=shape_, ys=ys, xs=xs, zs=zs, intensity=intensity)
        return mt.SequenceResult(levels, phases, np.ones((frames_n, m)), stats, iters, np.ones((frames_n, m)))

    monkeypatch.setattr(mt, "trap_array_sequence", stub)
    argv = ["walk", "-v", "2", "-ct2pi", "200", "--shape", "6x8", "-loops", "5", "-first", "5", "-tol", "0.02"]
    curves = gts.cli(argv + (["-p"] if preview else []))
    want = traj.astype(np.float32).astype(np.float64)
    assert seen["shape"] == shape
    np.testing.assert_array_equal(seen["ys"], want[:, :, 0])
    np.testing.assert_array_equal(seen["xs"], want[:, :, 1])
    if columns == 4:
        np.testing.assert_array_equal(seen["zs"], want[:, :, 2])
        np.testing.assert_array_equal(seen["intensity"], want[:, :, 3])
    else:
        assert seen["zs"] is None and seen["intensity"] is None
    assert (seen["loops_first"], seen["loops"], seen["tol"], seen["feedback"]) == (5, 5, 0.02, 1.0)
    assert seen["ct2pi"] == 200 and seen["ain"] is None and seen["holograms"] is True
    out = tmp_path / "holograms" / "walk_2_holograms"
    assert sorted(os.listdir(out)) == [f"{i}.npy" for i in range(frames_n)]
    for i in range(frames_n):
        got = np.load(out / f"{i}.npy")
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, hologram_from(phases[i]))
    assert got.max() <= np.pi
    prev = tmp_path / "images" / "moving_traps" / "walk_2_preview"
    if preview:
        from PIL import Image

        assert sorted(os.listdir(prev)) == [f"{i}.png" for i in range(frames_n)]
        np.testing.assert_array_equal(np.array(Image.open(prev / "1.png")), levels[1])
    else:
        assert not prev.exists()
    assert [len(c) for c in curves] == [5, 2, 3]
    assert curves[1] == [float(u) for u in stats[1, :2, 1]]
    printed = capsys.readouterr().out
    for i in range(frames_n):
        assert f"\rcreating {i}. hologram " in printed


def test_cli_rejects_a_malformed_trajectory(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "images" / "moving_traps")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(mt, "trap_array_sequence", lambda *a, **k: pytest.fail("ran"))
    for bad in (np.zeros((3, 4)), np.zeros((3, 4, 1)), np.zeros((3, 4, 5)), np.zeros((0, 4, 2))):
        np.save("images/moving_traps/bad.npy", bad)
        with pytest.raises(ValueError):
            gts.cli(["bad", "-v", "1", "-ct2pi", "256", "--shape", "6x8"])
