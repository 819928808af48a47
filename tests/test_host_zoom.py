"""The zoomed far field without a device: the float64 reference
(tests/zoom_reference.py) against the two closed forms it must reproduce, the
window arithmetic of move_traps.trap_window, the argument checks of
_lib.farfield_zoom (all raised before the library is touched), and the new
flags of the trap-trajectory CLI."""
import numpy as np
import pytest

import spots_reference as sr
import zoom_reference as zr
from spatial_light_modulator_module_amd import _lib
from spatial_light_modulator_module_amd import generate_trap_sequence as gts
from spatial_light_modulator_module_amd import move_traps as mt


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_ain", [False, True], ids=["uniform", "ain"])
def test_reference_is_fft2_on_whole_bins(with_ain):
    h, w = 24, 40
    rng = np.random.default_rng(1)
    phase = rng.uniform(-np.pi, np.pi, (h, w)).astype(np.float32)
    ain = rng.uniform(0.2, 1.0, (h, w)).astype(np.float32) if with_ain else None
    v = zr.zoom(phase, (-7, 30), 1.0, (20, 25), ain=ain)
    u = zr.unit_field(phase) * (1.0 if ain is None else ain.astype(np.float64))
    full = np.fft.fft2(u)
    want = full[np.ix_((-7 + np.arange(20)) % h, (30 + np.arange(25)) % w)]
    dev = np.abs(v - want).max() / zr.sum_a((h, w), ain)
    print(f"reference vs fft2: {dev:.3e} of sum a")
    assert dev <= 1e-12


def _dirichlet(n_pix, p, trap):
    """sum_n exp(2 pi i n (trap - p) / N) for every sample position p."""
    n = np.arange(n_pix, dtype=np.float64)[:, None]
    return np.exp(2j * np.pi * n * (trap - p) / n_pix).sum(axis=0)


def test_reference_is_the_dirichlet_product_of_one_trap():
    h, w = 45, 70
    y, x, z = 3.37, -5.81, 2e-4
    phase = sr.delta(h, w, y, x, z)  # float64: kept exact below by handing the reference float64 tables
    origin, pitch, size = (1.0, -8.0), 0.125, (33, 41)
    # the single-trap hologram as a unit field (not through float32: the identity is about the sums)
    u = np.exp(1j * phase)
    py = zr.table(h, origin[0], pitch, size[0], z)
    px = zr.table(w, origin[1], pitch, size[1], z)
    v = np.conj(py).T @ (u @ np.conj(px))
    pj = origin[0] + np.arange(size[0]) * pitch
    pi_ = origin[1] + np.arange(size[1]) * pitch
    want = _dirichlet(h, pj, y)[:, None] * _dirichlet(w, pi_, x)[None, :]
    dev = np.abs(v - want).max() / (h * w)
    print(f"reference vs Dirichlet product: {dev:.3e} of sum a")
    assert dev <= 1e-12
    # and through the public reference (float32 phase): the peak is sum a at the trap, within a sample
    v32 = zr.zoom(phase.astype(np.float32), origin, pitch, size, z=z)
    j, i = np.unravel_index(np.abs(v32).argmax(), v32.shape)
    assert abs(pj[j] - y) <= pitch and abs(pi_[i] - x) <= pitch
    assert abs(np.abs(v32).max() / (h * w) - 1.0) < 2e-2  # the nearest sample is within 1/16 bin of the peak


def test_reference_uint8_rule():
    frame = np.arange(256, dtype=np.uint8).reshape(16, 16)
    u = zr.unit_field(frame, 200)
    want = np.exp(2j * np.pi * np.arange(256) / 200.0).reshape(16, 16)
    assert u.dtype == np.complex128
    np.testing.assert_array_equal(u, u.astype(np.complex64))  # rounded to complex64
    assert np.abs(u - want).max() <= 2.0 ** -24  # half a float32 ulp at 1 per component, at most


# ---------------------------------------------------------------------------
# trap_window
# ---------------------------------------------------------------------------
def test_trap_window_arithmetic():
    ys = np.array([[3.37, -2.2], [10.01, 0.5]])
    xs = np.array([[-5.81, 7.0], [6.99, 1.25]])
    origin, pitch, size = mt.trap_window(ys, xs)
    assert pitch == (0.125, 0.125)
    for o, n, v in ((origin[0], size[0], ys), (origin[1], size[1], xs)):
        last = o + (n - 1) * 0.125
        assert o <= v.min() - 4.0 and last >= v.max() + 4.0  # the margin holds
        assert o > v.min() - 4.0 - 0.125 and last < v.max() + 4.0 + 0.125  # and is not wider than a sample
        assert (o * 8) == int(o * 8)  # whole bins are samples: the origin is a multiple of the pitch
        pos = o + np.arange(n) * 0.125
        for b in range(int(np.ceil(o)), int(np.floor(last)) + 1):
            assert b in pos
    origin, pitch, size = mt.trap_window([0.0], [0.0], margin=1.0, oversample=3)
    assert size == (7, 7) and pitch == (1 / 3, 1 / 3) and origin == (-1.0, -1.0)
    origin, pitch, size = mt.trap_window([2.5], [2.5], margin=0.0, oversample=1)
    assert origin == (2.0, 2.0) and size == (2, 2)


def test_trap_window_size_cap():
    origin, pitch, size = mt.trap_window([0.0, 503.0], [0.0], margin=4.0, oversample=8)
    assert size[0] == 511 * 8 + 1 <= 4096
    with pytest.raises(ValueError, match="oversample.*margin"):
        mt.trap_window([0.0, 504.0], [0.0], margin=4.0, oversample=8)
    with pytest.raises(ValueError, match="oversample.*margin"):
        mt.trap_window([0.0], [-300.0, 300.0])
    with pytest.raises(ValueError):
        mt.trap_window([], [])
    with pytest.raises(ValueError):
        mt.trap_window([np.nan], [0.0])
    with pytest.raises(ValueError):
        mt.trap_window([0.0], [0.0], oversample=0)
    with pytest.raises(ValueError):
        mt.trap_window([0.0], [0.0], margin=-1.0)


# ---------------------------------------------------------------------------
# farfield_zoom refuses in Python, before any device call
# ---------------------------------------------------------------------------
def test_refusals_before_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(_lib, "init", no_device)
    ph = np.zeros((8, 12), np.float32)
    fr = np.zeros((8, 12), np.uint8)
    ok = dict(origin=(0.0, 0.0), pitch=0.25, size=(4, 4))

    def refused(holo, **kw):
        args = {**ok, **kw}
        with pytest.raises(ValueError):
            _lib.farfield_zoom(holo, args.pop("origin"), args.pop("pitch"), args.pop("size"), **args)

    refused(np.zeros(8, np.float32))                      # not [H][W] or [B][H][W]
    refused(np.zeros((1, 1, 8, 12), np.float32))
    refused(np.zeros((8, 12), np.int32))                  # neither a phase nor a frame
    refused(np.zeros((0, 8, 12), np.float32))             # batch < 1
    refused(np.zeros((1, 12), np.float32))                # a side outside 2 .. 4096
    refused(np.zeros((8, 4097), np.float32))
    refused(ph, size=(0, 4))                              # ny or nx outside 1 .. 4096
    refused(ph, size=(4, 4097))
    refused(ph, size=(4.5, 4))
    refused(ph, size=(4, 4, 4))
    for bad in (np.nan, np.inf):
        refused(ph, origin=(bad, 0.0))
        refused(ph, origin=(0.0, bad))
        refused(ph, pitch=(bad, 0.25))
        refused(ph, pitch=(0.25, bad))
        refused(ph, z=bad)
    refused(ph, pitch=0.0)                                # dy or dx <= 0
    refused(ph, pitch=(0.25, -0.25))
    refused(fr)                                           # a frame without ct2pi
    for bad in (0, -256, np.nan, np.inf):
        refused(fr, ct2pi=bad)
    refused(ph, ain=np.ones((8, 11), np.float32))         # ain of another shape
    bad_ain = np.ones((8, 12), np.float32)
    bad_ain[3, 3] = np.nan
    refused(ph, ain=bad_ain)
    refused(ph, ain=np.zeros((8, 12), np.float32))        # zero everywhere
    # a call that passes every check reaches the library
    with pytest.raises(AssertionError, match="touched"):
        _lib.farfield_zoom(ph, **ok)
    with pytest.raises(AssertionError, match="touched"):
        mt.expected_outcome(fr, (ok["origin"], ok["pitch"], ok["size"]), ct2pi=256)


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------
def test_cli_parser_takes_the_new_flags():
    base = ["walk", "-v", "1", "-ct2pi", "256"]
    args = gts.build_parser().parse_args(base)
    assert args.expected is False and args.oversample == 8 and args.margin == 4.0 and args.expected_z == 0.0
    args = gts.build_parser().parse_args(base + ["--expected", "--oversample", "4", "--margin", "2.5", "--expected_z",
                                                 "1e-4"])
    assert args.expected is True and args.oversample == 4 and args.margin == 2.5 and args.expected_z == 1e-4
    assert gts.expected_dir("walk", "1") == "images/moving_traps/walk_1_expected"
