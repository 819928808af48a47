"""The resident zoom without a device: every ValueError of _lib.Zoom and of
trap_array_sequence(expected=...) is raised before the library is touched, the
window arithmetic of move_traps.trap_windows, the masked reference
(tests/zoom_handle_reference.py) and the CLI's new flag."""
import numpy as np
import pytest

import zoom_handle_reference as zhr
import zoom_reference as zr
from spatial_light_modulator_module_amd import _lib
from spatial_light_modulator_module_amd import generate_trap_sequence as gts
from spatial_light_modulator_module_amd import move_traps as mt


def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(_lib, "init", no_device)


def _touches():
    return pytest.raises(AssertionError, match="touched")


# ---------------------------------------------------------------------------
# _lib.Zoom refuses in Python, before any device call
# ---------------------------------------------------------------------------
def test_zoom_refusals_before_the_device(monkeypatch):
    _no_device(monkeypatch)
    for bad in (dict(batch=0), dict(batch=1025), dict(batch=1.5), dict(height=1), dict(height=4097), dict(width=1),
                dict(width=4097), dict(height=8.5), dict(max_size=0), dict(max_size=(4, 4097)), dict(max_size=(4, 4, 4)),
                dict(max_size=4.5)):
        with pytest.raises(ValueError):
            _lib.Zoom(**{**dict(batch=3, height=8, width=12, max_size=(6, 5)), **bad})
    zm = _lib.Zoom(3, 8, 12, (6, 5))  # touches nothing
    assert zm.handle is None and zm.max_size == (6, 5)
    ok = dict(origin=(0.0, 0.0), pitch=0.25, size=(4, 4))

    def refused(fn, *a, **kw):
        with pytest.raises(ValueError):
            fn(*a, **kw)

    def window(**kw):
        zm.set_window(**{**ok, **kw})

    # a_in and the mask
    refused(zm.set_ain, np.ones((8, 11), np.float32))
    bad = np.ones((8, 12), np.float32)
    bad[3, 3] = np.nan
    refused(zm.set_ain, bad)
    refused(zm.set_ain, np.zeros((8, 12), np.float32))
    refused(zm.set_mask, np.zeros((8, 11)))
    for v in (np.nan, np.inf):
        m = np.zeros((8, 12))
        m[1, 2] = v
        refused(zm.set_mask, m)
    # the window
    refused(window, size=(0, 4))
    refused(window, size=(4, 4097))
    refused(window, size=(4.5, 4))
    refused(window, size=(7, 4))   # above the handle's max_size
    refused(window, size=(4, 6))
    refused(window, origin=(0.0, 0.0, 0.0))
    refused(window, origin=np.zeros((2, 2)))      # neither (y0, x0) nor [batch 3][2]
    refused(window, z=np.zeros(2))                # neither a number nor [batch 3]
    for v in (np.nan, np.inf):
        refused(window, origin=(v, 0.0))
        refused(window, origin=np.array([[0.0, 0.0], [0.0, v], [0.0, 0.0]]))
        refused(window, pitch=(v, 0.25))
        refused(window, z=v)
        refused(window, z=np.array([0.0, v, 0.0]))
    refused(window, pitch=0.0)
    refused(window, pitch=(0.25, -0.25))
    # runs: before a window, then with one (set behind the library's back: the device is out of reach here)
    ph = np.zeros((3, 8, 12), np.float32)
    fr = np.zeros((3, 8, 12), np.uint8)
    refused(zm.run, ph)
    refused(zm.read)
    zm.size = (4, 4)
    refused(zm.run, np.zeros(8, np.float32))
    refused(zm.run, np.zeros((3, 8, 12), np.int32))
    refused(zm.run, np.zeros((0, 8, 12), np.float32))
    refused(zm.run, np.zeros((4, 8, 12), np.float32))   # more than the batch
    refused(zm.run, np.zeros((3, 8, 13), np.float32))   # another shape
    refused(zm.run, fr)                                 # frames without ct2pi
    for v in (0, -256, np.nan, np.inf):
        refused(zm.run, fr, ct2pi=v)

    class Source:  # what run_spots / run_plan read of a Spots or a Plan
        def __init__(self, batch, height, width, seq, handle=1):
            self.batch, self.height, self.width, self._seq, self.handle = batch, height, width, seq, handle

    for run in (zm.run_spots, zm.run_plan):
        refused(run, Source(1, 8, 12, None), 0, 1, 256)            # no sequence
        refused(run, Source(1, 8, 12, (2, 5, 4), None), 0, 1, 256)  # a closed source
        refused(run, Source(1, 8, 13, (2, 5, 4)), 0, 1, 256)        # another shape
        refused(run, Source(1, 8, 12, (2, 5, 4)), 0, 3, 256)        # past the end
        refused(run, Source(1, 8, 12, (2, 5, 4)), -1, 1, 256)
        refused(run, Source(1, 8, 12, (2, 5, 4)), 1, 2, 256)
        refused(run, Source(2, 8, 12, (2, 5, 4)), 0, 4, 256)        # more than the handle's batch
        refused(run, Source(1, 8, 12, (2, 5, 4)), 0, 0, 256)
        refused(run, Source(1, 8, 12, (2, 5, 4)), 0.5, 1, 256)
        refused(run, Source(1, 8, 12, (2, 5, 4)), 0, 1, None)
        refused(run, Source(1, 8, 12, (2, 5, 4)), 0, 1, np.inf)
    # calls that pass every check reach the library
    zm.size = None
    for call in (lambda: zm.set_ain(np.ones((8, 12), np.float32)), lambda: zm.set_mask(np.zeros((8, 12))),
                 lambda: window(), lambda: window(origin=np.zeros((3, 2)), z=np.zeros(3))):
        with _touches():
            call()
    zm.size = (4, 4)
    with _touches():
        zm.run(ph)
    with _touches():
        zm.run(fr[:2], ct2pi=200)
    with _touches():
        zm.run_spots(Source(2, 8, 12, (2, 5, 4)), 1, 3, 256)
    with _touches():
        zm.run_plan(Source(1, 8, 12, (2, 4)), 0, 2, 256)


# ---------------------------------------------------------------------------
# trap_array_sequence(expected=...) refuses before any device call
# ---------------------------------------------------------------------------
def test_expected_refusals_before_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    _no_device(monkeypatch)
    monkeypatch.setattr(mt, "_get_spots", no_device)
    monkeypatch.setattr(mt, "_get_zoom", no_device)
    ys = np.array([[1.0, -2.0], [1.25, -2.0]])
    xs = np.array([[2.0, 3.0], [2.0, 3.25]])

    def refused(expected):
        with pytest.raises(ValueError):
            mt.trap_array_sequence((45, 70), ys, xs, expected=expected)

    refused(True)
    refused(dict(oversampling=4))
    refused(dict(oversample=0))
    refused(dict(margin=-1.0))
    refused(dict(margin=np.nan))
    refused(dict(z=np.inf))
    refused(dict(margin=300.0))                 # a window above 4096 samples
    refused(dict(margin=300.0, follow=True))
    with _touches():
        mt.trap_array_sequence((45, 70), ys, xs, expected=dict(oversample=4, follow=True, mask_off=True, z=1e-4))
    with _touches():
        mt.trap_array_sequence((45, 70), ys, xs)


# ---------------------------------------------------------------------------
# trap_windows
# ---------------------------------------------------------------------------
def test_trap_windows_arithmetic():
    rng = np.random.default_rng(3)
    f, m = 6, 5
    ys = rng.uniform(-20, 20, (f, m)) + np.arange(f)[:, None] * 1.3
    xs = rng.uniform(-30, 30, (f, m)) - np.arange(f)[:, None] * 0.7
    ys[2] = [0.0, 0.1, 0.2, 0.3, 0.4]  # one frame much tighter than the others
    for margin, oversample in ((4.0, 8), (1.5, 3)):
        origins, pitch, size = mt.trap_windows(ys, xs, margin=margin, oversample=oversample)
        assert origins.shape == (f, 2) and pitch == (1.0 / oversample,) * 2
        boxes = [mt.trap_window(ys[i], xs[i], margin=margin, oversample=oversample) for i in range(f)]
        assert size == (max(b[2][0] for b in boxes), max(b[2][1] for b in boxes))  # the common size is the maximum
        assert size[0] > boxes[2][2][0]
        for i in range(f):
            assert tuple(origins[i]) == boxes[i][0] and boxes[i][1] == pitch
            for o, n, v, own in ((origins[i][0], size[0], ys[i], boxes[i][2][0]),
                                 (origins[i][1], size[1], xs[i], boxes[i][2][1])):
                assert abs(o * oversample - round(o * oversample)) < 1e-9  # a multiple of the pitch
                assert o <= v.min() - margin and o + (own - 1) / oversample >= v.max() + margin - 1e-9
                assert n >= own  # the frame's own box lies inside its window
    one = mt.trap_windows(ys[:1], xs[:1])
    box = mt.trap_window(ys[0], xs[0])
    assert tuple(one[0][0]) == box[0] and one[1] == box[1] and one[2] == box[2]
    for bad in ((ys[0], xs[0]), (ys, xs[:, :4]), (np.zeros((0, 3)), np.zeros((0, 3)))):
        with pytest.raises(ValueError):
            mt.trap_windows(*bad)
    with pytest.raises(ValueError):
        mt.trap_windows(ys, xs, oversample=0)
    nan = ys.copy()
    nan[1, 1] = np.nan
    with pytest.raises(ValueError):
        mt.trap_windows(nan, xs)


# ---------------------------------------------------------------------------
# the masked reference
# ---------------------------------------------------------------------------
def test_masked_reference():
    h, w = 24, 40
    rng = np.random.default_rng(5)
    phase = rng.uniform(-np.pi, np.pi, (h, w)).astype(np.float32)
    mask = rng.uniform(0, 2 * np.pi, (h, w))
    window = ((-3.375, 2.625), 0.125, (9, 11))
    # no mask: the reference of the one-shot
    np.testing.assert_array_equal(zhr.zoom(phase, *window, z=1e-4), zr.zoom(phase, *window, z=1e-4))
    # a mask is a phase taken off: the zoom of (phase - mask) up to the float32 rounding of that phase
    v = zhr.zoom(phase, *window, mask=mask)
    near = zr.zoom((phase.astype(np.float64) - mask).astype(np.float32), *window)
    assert np.abs(v - near).max() / (h * w) < 1e-6
    assert np.abs(v - zr.zoom(phase, *window)).max() / (h * w) > 1e-2
    u = zhr.unit_field(phase, mask)
    np.testing.assert_array_equal(u, u.astype(np.complex64))  # rounded to complex64
    # the mask-off identity in float64, as the GPU test leans on it
    for ct2pi in (256, 200):
        levels = rng.integers(0, ct2pi, (h, w))
        k = rng.integers(0, ct2pi, (h, w))
        frame = ((levels + k) % ct2pi).astype(np.uint8)
        dev = np.abs(zhr.zoom(frame, *window, ct2pi=ct2pi, mask=k * (2 * np.pi / ct2pi)) -
                     zr.zoom(levels.astype(np.uint8), *window, ct2pi=ct2pi)).max() / (h * w)
        print(f"mask-off identity in the reference, ct2pi={ct2pi}: {dev:.3e} sum(a)")
        assert dev <= 1e-7  # complex64 rounding of u on both sides: 2^-24 per component at the most


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------
def test_cli_parser_takes_follow():
    base = ["walk", "-v", "1", "-ct2pi", "256"]
    assert gts.build_parser().parse_args(base).follow is False
    args = gts.build_parser().parse_args(base + ["--expected", "--follow"])
    assert args.expected is True and args.follow is True


def test_cli_hands_the_preview_to_the_sequence(tmp_path, monkeypatch):
    import os

    traj = np.array([[[1.0, 2.0], [-3.0, 4.5]], [[1.25, 2.0], [-3.0, 4.25]]])
    os.makedirs(tmp_path / "images" / "moving_traps")
    np.save(tmp_path / "images" / "moving_traps" / "walk.npy", traj)
    monkeypatch.chdir(tmp_path)
    seen = {}

    def stub(shape, ys, xs, zs=None, intensity=None, **kw):
        seen.update(kw)
        exp = None if kw["expected"] is None else np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
        return mt.SequenceResult(np.zeros((2, 6, 8), np.uint8), np.zeros((2, 6, 8)), np.ones((2, 2)),
                                 np.zeros((2, 5, 4)), np.array([5, 2], np.int32), np.ones((2, 2)), exp)

    monkeypatch.setattr(mt, "trap_array_sequence", stub)
    base = ["walk", "-ct2pi", "200", "--shape", "6x8"]
    gts.cli(base + ["-v", "1"])
    assert seen["expected"] is None
    gts.cli(base + ["-v", "2", "--expected", "--margin", "2.5", "--oversample", "4", "--expected_z", "1e-4"])
    assert seen["expected"] == dict(margin=2.5, oversample=4, z=1e-4, follow=False)
    gts.cli(base + ["-v", "3", "--expected", "--follow"])
    assert seen["expected"] == dict(margin=4.0, oversample=8, z=0.0, follow=True)
    from PIL import Image

    png = np.array(Image.open(tmp_path / "images" / "moving_traps" / "walk_3_expected" / "1.png"))
    want = np.arange(12, 24, dtype=np.float64).reshape(3, 4)
    np.testing.assert_array_equal(png, np.floor(255.0 * want / 23.0).astype(np.uint8))
