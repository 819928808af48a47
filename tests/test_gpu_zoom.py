"""The zoomed far field (slm_farfield_zoom) on the MI355X: parity with the
float64 reference (tests/zoom_reference.py) on shapes that are no multiple of
the tile and on summed axes of several 256-pixel chunks, the coherent worst
case the chunked accumulation exists for, the uint8 path, agreement with the
trap lists' own field product, the bitwise identities (repeat, batch, a window
inside a larger one), the refusals of the C boundary, and the --expected
preview of the trap-trajectory CLI.

Gates (both stated by the feature's definition, none measured): the field
within FIELDS_TOL = 1e-6 sum(a) of the reference, the bound tests/test_gpu_spots.py
holds the same product to, and the intensity within 2.1e-6 sum(a)^2, which
follows from it by |dI| <= |dV| (2 |V| + |dV|) with |V| <= sum(a)."""
import os

import numpy as np
import pytest

import spots_reference as sr
import zoom_reference as zr
from gsw_reference import incoming_gauss

FIELDS_TOL = 1e-6      # times sum(a)
INTENSITY_TOL = 2.1e-6  # times sum(a)^2


def _phase(h, w, seed):
    return np.random.default_rng(seed).uniform(-np.pi, np.pi, (h, w)).astype(np.float32)


def _gates(label, inten, field, ref, s_a):
    dv = np.abs(field - ref).max() / s_a
    di = np.abs(inten.astype(np.float64) - np.abs(ref) ** 2).max() / s_a ** 2
    print(f"zoom {label}: max|V - V_ref| = {dv:.3e} sum(a), max|I - I_ref| = {di:.3e} sum(a)^2")
    assert inten.dtype == np.float32 and field.dtype == np.complex128
    assert dv <= FIELDS_TOL
    assert di <= INTENSITY_TOL
    return dv, di


# ---------------------------------------------------------------------------
# 1. parity with the float64 reference
# ---------------------------------------------------------------------------
# (H, W), (ny, nx): nothing a multiple of 32; one sample and one tile; several tiles of both products;
# 16 chunks of 256 in the first product (W = 4096) and in the second (H = 4096)
PARITY = [((45, 70), (33, 70)), ((64, 64), (1, 1)), ((64, 64), (32, 32)), ((130, 264), (96, 40)),
          ((64, 4096), (40, 40)), ((4096, 64), (40, 40))]


@pytest.mark.gpu
@pytest.mark.parametrize("z", [0.0, 2e-4], ids=["z0", "z2e-4"])
@pytest.mark.parametrize("with_ain", [False, True], ids=["uniform", "ain"])
@pytest.mark.parametrize("shape,size", PARITY, ids=[f"{s[0]}x{s[1]}-{n[0]}x{n[1]}" for s, n in PARITY])
def test_parity_with_the_reference(gpu, shape, size, with_ain, z):
    h, w = shape
    phase = _phase(h, w, 3 + h + w)
    ain = incoming_gauss(h, w) if with_ain else None
    origin, pitch = (-h / 8 + 0.3125, w / 16 - 1.71), 0.125  # fractional, one of them no multiple of the pitch
    inten, field = gpu.farfield_zoom(phase, origin, pitch, size, z=z, ain=ain, return_field=True)
    assert inten.shape == size and field.shape == size
    ref = zr.zoom(phase, origin, pitch, size, z=z, ain=ain)
    _gates(f"{h}x{w} window {size[0]}x{size[1]} ain={with_ain} z={z}", inten, field, ref, zr.sum_a(shape, ain))


# ---------------------------------------------------------------------------
# 2. the coherent worst case: one trap, every pixel in phase at its position
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("with_ain", [False, True], ids=["uniform", "ain"])
@pytest.mark.parametrize("shape,trap", [((64, 4096), (5.3, -617.6)), ((4096, 64), (333.3, 7.45))],
                         ids=["64x4096", "4096x64"])
def test_single_trap_is_coherent(gpu, shape, trap, with_ain):
    h, w = shape
    pitch, n = 0.125, 41
    ain = incoming_gauss(h, w) if with_ain else None
    phase = np.float32(np.mod(sr.delta(h, w, trap[0], trap[1]), 2 * np.pi))
    origin = tuple(np.round(np.array(trap) / pitch) * pitch - (n // 2) * pitch)  # the centre sample is the nearest to the trap
    inten, field = gpu.farfield_zoom(phase, origin, pitch, (n, n), ain=ain, return_field=True)
    ref = zr.zoom(phase, origin, pitch, (n, n), ain=ain)
    s_a = zr.sum_a(shape, ain)
    _gates(f"single trap {h}x{w} ain={with_ain}", inten, field, ref, s_a)
    j, i = np.unravel_index(inten.argmax(), inten.shape)
    assert abs(origin[0] + j * pitch - trap[0]) <= pitch and abs(origin[1] + i * pitch - trap[1]) <= pitch
    peak = np.sqrt(float(inten.max())) / s_a
    print(f"zoom single trap {h}x{w}: peak |V| = {peak:.6f} sum(a)")
    assert 0.97 < peak <= 1.0 + 1e-6  # sum(a) at the trap; the nearest sample is within 1/16 bin of it


# ---------------------------------------------------------------------------
# 3. uint8 frames
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ct2pi", [256, 200])
def test_uint8_frames(gpu, ct2pi):
    h, w, size = 130, 264, (33, 70)
    frames = np.random.default_rng(ct2pi).integers(0, 256, (3, h, w), dtype=np.uint8)
    ain = incoming_gauss(h, w)
    origin, pitch = (-7.4375, 11.29), (0.125, 0.25)
    inten, field = gpu.farfield_zoom(frames, origin, pitch, size, z=1e-4, ain=ain, ct2pi=ct2pi, return_field=True)
    assert inten.shape == (3,) + size
    for b in range(3):
        ref = zr.zoom(frames[b], origin, pitch, size, z=1e-4, ain=ain, ct2pi=ct2pi)
        _gates(f"uint8 ct2pi={ct2pi} frame {b}", inten[b], field[b], ref, zr.sum_a((h, w), ain))
        solo_i, solo_v = gpu.farfield_zoom(frames[b], origin, pitch, size, z=1e-4, ain=ain, ct2pi=ct2pi,
                                           return_field=True)
        np.testing.assert_array_equal(solo_i, inten[b])
        np.testing.assert_array_equal(solo_v, field[b])
    # the levels are read with ct2pi, not as radians
    other = gpu.farfield_zoom(frames[0], origin, pitch, size, z=1e-4, ain=ain, ct2pi=456 - ct2pi)
    assert not np.array_equal(other, inten[0])


# ---------------------------------------------------------------------------
# 4. the window's samples as a trap list through the fields product that exists
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("with_ain", [False, True], ids=["uniform", "ain"])
def test_agrees_with_spots_fields(gpu, with_ain):
    h, w, size = 96, 160, (12, 20)
    origin, pitch, z = (-4.3, 9.55), 0.125, 2e-4
    phase = _phase(h, w, 8)
    ain = incoming_gauss(h, w) if with_ain else None
    _, field = gpu.farfield_zoom(phase, origin, pitch, size, z=z, ain=ain, return_field=True)
    ys = np.repeat(origin[0] + np.arange(size[0]) * pitch, size[1])
    xs = np.tile(origin[1] + np.arange(size[1]) * pitch, size[0])
    v = gpu.spots_fields(phase, ys, xs, np.full(ys.size, z), ain=ain)[0].reshape(size)
    s_a = zr.sum_a((h, w), ain)
    dev = np.abs(field - v).max() / s_a
    print(f"zoom vs spots_fields 96x160 ain={with_ain}: {dev:.3e} sum(a)")
    assert dev <= 2 * FIELDS_TOL  # each side is within FIELDS_TOL of the same reference
    ref = zr.zoom(phase, origin, pitch, size, z=z, ain=ain)
    assert np.abs(field - ref).max() / s_a <= FIELDS_TOL and np.abs(v - ref).max() / s_a <= FIELDS_TOL


# ---------------------------------------------------------------------------
# 5. bitwise identities
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_bitwise_repeat_and_sub_window(gpu):
    h, w = 130, 600  # three chunks in the first product; one in the second
    phase = _phase(h, w, 21)
    ain = incoming_gauss(h, w)
    # every position is a dyadic fraction, so y0 + j dy is the same float64 in both windows
    origin, pitch, size, z = (-3.375, 2.625), 0.125, (70, 90), 2e-4
    big_i, big_v = gpu.farfield_zoom(phase, origin, pitch, size, z=z, ain=ain, return_field=True)
    again_i, again_v = gpu.farfield_zoom(phase, origin, pitch, size, z=z, ain=ain, return_field=True)
    np.testing.assert_array_equal(again_i, big_i)
    np.testing.assert_array_equal(again_v, big_v)
    j0, i0, sub = 19, 37, (33, 40)  # other tiles, another padding
    sub_i, sub_v = gpu.farfield_zoom(phase, (origin[0] + j0 * pitch, origin[1] + i0 * pitch), pitch, sub, z=z, ain=ain,
                                     return_field=True)
    np.testing.assert_array_equal(sub_i, big_i[j0:j0 + sub[0], i0:i0 + sub[1]])
    np.testing.assert_array_equal(sub_v, big_v[j0:j0 + sub[0], i0:i0 + sub[1]])
    # the tall case: several chunks in the second product, the sub-window in another band of tiles
    phase = _phase(600, 45, 22)
    big_i, big_v = gpu.farfield_zoom(phase, origin, pitch, size, return_field=True)
    sub_i, sub_v = gpu.farfield_zoom(phase, (origin[0] + j0 * pitch, origin[1] + i0 * pitch), pitch, sub,
                                     return_field=True)
    np.testing.assert_array_equal(sub_i, big_i[j0:j0 + sub[0], i0:i0 + sub[1]])
    np.testing.assert_array_equal(sub_v, big_v[j0:j0 + sub[0], i0:i0 + sub[1]])
    # 33 row tiles x 128 sample tiles (4224 waves): the first product adds its two chunks in registers;
    # the sub-window's 2 sample tiles split the columns over workgroups and fold them afterwards
    phase = _phase(1056, 300, 23)
    big_i, big_v = gpu.farfield_zoom(phase, origin, pitch, (8, 4096), z=z, return_field=True)
    sub_i, sub_v = gpu.farfield_zoom(phase, (origin[0], origin[1] + i0 * pitch), pitch, (8, 40), z=z,
                                     return_field=True)
    np.testing.assert_array_equal(sub_i, big_i[:, i0:i0 + 40])
    np.testing.assert_array_equal(sub_v, big_v[:, i0:i0 + 40])
    ref = zr.zoom(phase, (origin[0], origin[1] + i0 * pitch), pitch, (8, 40), z=z)
    _gates("1056x300 window 8x40 inside 8x4096", sub_i, sub_v, ref, zr.sum_a((1056, 300)))


# ---------------------------------------------------------------------------
# 6. refusals of the C boundary
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(gpu):
    lib = gpu.load()
    h, w, ny, nx = 8, 12, 4, 5
    ph = np.zeros((1, h, w), np.float32)
    fr = np.zeros((1, h, w), np.uint8)
    ones = np.ones((h, w), np.float32)
    out = np.zeros((1, ny, nx), np.float32)
    ok = dict(hologram=gpu.ptr(ph), kind=gpu.ZOOM_PHASE_F32, batch=1, height=h, width=w, ain=None, ct2pi=0.0, y0=0.0,
              x0=0.0, dy=0.25, dx=0.25, ny=ny, nx=nx, z=0.0, intensity=gpu.ptr(out), field=None)

    def call(**kw):
        return lib.slm_farfield_zoom(*{**ok, **kw}.values())

    def refused(**kw):
        assert call(**kw) == gpu.ERR_ARG, kw
        assert gpu.last_error(), kw

    assert call() == 0
    assert call(hologram=gpu.ptr(fr), kind=gpu.ZOOM_LEVELS_U8, ct2pi=200.0) == 0
    refused(hologram=None)
    refused(intensity=None)
    refused(kind=2)
    refused(kind=-1)
    refused(batch=0)
    for side in (1, 4097):
        refused(height=side)
        refused(width=side)
    for n in (0, 4097):
        refused(ny=n)
        refused(nx=n)
    for bad in (np.nan, np.inf, -np.inf):
        for name in ("y0", "x0", "dy", "dx", "z"):
            refused(**{name: bad})
    for name in ("dy", "dx"):
        refused(**{name: 0.0})
        refused(**{name: -0.25})
    for bad in (0.0, -200.0, np.nan, np.inf):
        refused(hologram=gpu.ptr(fr), kind=gpu.ZOOM_LEVELS_U8, ct2pi=bad)
    bad_ain = ones.copy()
    bad_ain[2, 3] = np.inf
    refused(ain=gpu.ptr(bad_ain))
    refused(ain=gpu.ptr(np.zeros((h, w), np.float32)))
    assert call(ain=gpu.ptr(ones)) == 0
    assert "4096" in _message(gpu, call, height=4097) and "4096" in _message(gpu, call, nx=4097)


def _message(gpu, call, **kw):
    assert call(**kw) == gpu.ERR_ARG
    return gpu.last_error()


# ---------------------------------------------------------------------------
# 7. the CLI's --expected
# ---------------------------------------------------------------------------
def _brightest_maxima(img, count, radius):
    """The `count` brightest local maxima of img, each the brightest sample left
    once the samples within `radius` of the earlier ones are set aside."""
    img = img.astype(np.float64).copy()
    found = []
    for _ in range(count):
        j, i = np.unravel_index(img.argmax(), img.shape)
        found.append((j, i))
        img[max(0, j - radius):j + radius + 1, max(0, i - radius):i + radius + 1] = -1.0
    return found


@pytest.mark.gpu
def test_cli_writes_the_expected_outcome(gpu, tmp_path, monkeypatch):
    from PIL import Image

    from spatial_light_modulator_module_amd import generate_trap_sequence as gts
    from spatial_light_modulator_module_amd import move_traps as mt

    # four traps in no regular arrangement, each drifting a quarter pixel per frame
    start = np.array([[-9.5, -14.25], [-6.0, 11.5], [7.25, -8.0], [10.5, 15.75]])
    step = np.array([[0.25, 0.0], [0.0, -0.25], [-0.25, 0.25], [0.25, 0.25]])
    traj = np.stack([start + f * step for f in range(3)])  # [F][M][2]: y, x (z = 0, intensity 1)
    os.makedirs(tmp_path / "images" / "moving_traps")
    np.save(tmp_path / "images" / "moving_traps" / "walk.npy", traj)
    monkeypatch.chdir(tmp_path)
    base = ["walk", "-ct2pi", "256", "--shape", "45x70", "-first", "20", "-loops", "4"]

    gts.cli(base + ["-v", "plain"])
    assert not os.path.exists(tmp_path / "images" / "moving_traps" / "walk_plain_expected")
    assert sorted(os.listdir(tmp_path / "images" / "moving_traps")) == ["walk.npy"]

    gts.cli(base + ["-v", "1", "--expected", "--oversample", "4"])
    origin, pitch, size = mt.trap_window(traj[:, :, 0], traj[:, :, 1], margin=4.0, oversample=4)
    dest = tmp_path / "images" / "moving_traps" / "walk_1_expected"
    assert sorted(os.listdir(dest)) == ["0.png", "1.png", "2.png"]
    for f in range(3):
        np.testing.assert_array_equal(np.load(tmp_path / "holograms" / "walk_1_holograms" / f"{f}.npy"),
                                      np.load(tmp_path / "holograms" / "walk_plain_holograms" / f"{f}.npy"))
        im = Image.open(dest / f"{f}.png")
        assert im.mode == "L"
        png = np.array(im)
        assert png.shape == size and png.dtype == np.uint8 and png.max() == 255
        # a trap's main lobe ends one far-field pixel (4 samples) from it: set aside 6 around each maximum
        peaks = _brightest_maxima(png, 4, 6)
        want = [((y - origin[0]) / pitch[0], (x - origin[1]) / pitch[1]) for y, x in traj[f]]
        for j, i in peaks:
            assert min(max(abs(j - wj), abs(i - wi)) for wj, wi in want) <= 1.0, (f, j, i, want)
        assert len({min(range(4), key=lambda m: abs(j - want[m][0]) + abs(i - want[m][1])) for j, i in peaks}) == 4
    mt.clear_spots()


# ---------------------------------------------------------------------------
# 8. the one-shot is a resident zoom of one hologram: its bands, its caps, its timing
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_banded_one_shot(gpu):
    """One hologram's chunk results, 5 chunks x 1312 x 1312 x 8 B = 68.9 MB, exceed
    the 64 MB cap: the one-shot runs two bands, of 1248 and 64 rows."""
    h, w, size, z = 1056, 300, (1300, 1300), 2e-4
    origin, pitch = (-3.375, 2.625), 0.125  # dyadic: y0 + j dy is the same float64 in both windows
    phase = _phase(h, w, 23)
    big_i, big_v = gpu.farfield_zoom(phase, origin, pitch, size, z=z, return_field=True)
    with gpu.Zoom(1, h, w, size) as zm:
        zm.set_window(origin, pitch, size, z)
        zm.run(phase, return_field=True)
        got_i, got_v = zm.read()
        assert zm.info()["bands"] == 2
    np.testing.assert_array_equal(got_i[0], big_i)
    np.testing.assert_array_equal(got_v[0], big_v)
    j0, i0, sub = 1236, 37, (24, 40)  # rows 1236 .. 1259 lie across the two bands
    sub_i, sub_v = gpu.farfield_zoom(phase, (origin[0] + j0 * pitch, origin[1] + i0 * pitch), pitch, sub, z=z,
                                     return_field=True)
    np.testing.assert_array_equal(sub_i, big_i[j0:j0 + sub[0], i0:i0 + sub[1]])
    np.testing.assert_array_equal(sub_v, big_v[j0:j0 + sub[0], i0:i0 + sub[1]])


@pytest.mark.gpu
def test_the_environment_does_not_reach_the_one_shot(gpu, monkeypatch):
    h, w, size = 130, 264, (96, 40)
    holos = np.stack([_phase(h, w, 17), _phase(h, w, 18)])
    origin, pitch, z = (-3.375, 2.625), 0.125, 2e-4
    monkeypatch.delenv("SLM_ZOOM_PARTIAL_BYTES", raising=False)
    want_i, want_v = gpu.farfield_zoom(holos, origin, pitch, size, z=z, return_field=True)
    for value in ("32768", "many"):
        monkeypatch.setenv("SLM_ZOOM_PARTIAL_BYTES", value)
        got_i, got_v = gpu.farfield_zoom(holos, origin, pitch, size, z=z, return_field=True)
        np.testing.assert_array_equal(got_i, want_i)
        np.testing.assert_array_equal(got_v, want_v)


@pytest.mark.gpu
def test_timed_one_shot(gpu):
    h, w, size = 45, 70, (33, 70)
    frames = np.random.default_rng(41).integers(0, 256, (2, h, w), dtype=np.uint8)
    origin, pitch = (-3.375, 2.625), 0.125
    plain = gpu.farfield_zoom(frames, origin, pitch, size, ct2pi=200)
    inten, us = gpu.farfield_zoom(frames, origin, pitch, size, ct2pi=200, timed=True)
    print(f"zoom timed one-shot: {dict(zip(gpu.ZOOM_KERNEL_CLASS_NAMES, us))} us")
    assert us.shape == (gpu.ZOOM_NUM_KERNEL_CLASSES,) and gpu.ZOOM_NUM_KERNEL_CLASSES == 4
    assert np.isfinite(us).all() and (us > 0).all()
    np.testing.assert_array_equal(inten, plain)
