"""The resident zoom (slm_zoom_*, _lib.Zoom) on the MI355X. The one-shot
slm_farfield_zoom is its oracle, bit for bit: batched launches, groups, bands,
the per-launch split of the first product and per-hologram windows must not
move a bit of any sample. The correction mask, the only new arithmetic, is held
to the float64 reference (tests/zoom_handle_reference.py) with the gates of
tests/test_gpu_zoom.py. The frames of trap and image sequences are previewed
where they lie on the device, in order with the chains that write them."""
import os

import numpy as np
import pytest

import zoom_handle_reference as zhr
import zoom_reference as zr
from gsw_reference import incoming_gauss

pytestmark = pytest.mark.gpu

FIELDS_TOL = 1e-6      # times sum(a)         (tests/test_gpu_zoom.py)
INTENSITY_TOL = 2.1e-6  # times sum(a)^2

eq = np.testing.assert_array_equal
ORIGIN, PITCH = (-3.375, 2.625), 0.125  # dyadic: y0 + j dy is the same float64 however it is reached


def _phases(b, h, w, seed):
    return np.random.default_rng(seed).uniform(-np.pi, np.pi, (b, h, w)).astype(np.float32)


def _frames(b, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (b, h, w), dtype=np.uint8)


def _oneshot(gpu, holos, origins, pitch, size, zs, ain=None, ct2pi=None):
    """The oracle: the one-shot per hologram, hologram i on window i."""
    n = len(holos)
    origins = np.broadcast_to(np.asarray(origins, np.float64), (n, 2))
    zs = np.broadcast_to(np.asarray(zs, np.float64), (n,))
    out = [gpu.farfield_zoom(holos[i], tuple(origins[i]), pitch, size, z=float(zs[i]), ain=ain, ct2pi=ct2pi,
                             return_field=True) for i in range(n)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _run(zm, holos, ct2pi=None):
    zm.run(holos, ct2pi=ct2pi, return_field=True)
    inten, field = zm.read()
    assert inten.dtype == np.float32 and field.dtype == np.complex128
    return inten, field


# ---------------------------------------------------------------------------
# 1. bitwise against the one-shot
# ---------------------------------------------------------------------------
# (label, (H, W), windows, B, uint8 ct2pi or None, a_in, z, split launches expected per window)
BITWISE = [
    ("nothing-a-multiple-of-32", (45, 70), [(33, 70)], 3, None, True, 2e-4, [0]),
    ("three-chunks-in-product-1", (130, 600), [(70, 90)], 2, None, False, 2e-4, [1]),
    ("three-chunks-in-product-2", (600, 45), [(70, 90)], 2, None, False, 2e-4, [0]),
    ("both-forms-of-product-1", (1056, 300), [(8, 40), (8, 4096)], 2, None, False, 2e-4, [1, 0]),
    ("uint8-levels", (130, 264), [(33, 70)], 3, 200, True, 1e-4, [1]),
]


@pytest.mark.parametrize("label,shape,sizes,b,ct2pi,with_ain,z,splits", BITWISE, ids=[c[0] for c in BITWISE])
def test_bitwise_against_the_one_shot(gpu, label, shape, sizes, b, ct2pi, with_ain, z, splits):
    h, w = shape
    holos = _frames(b, h, w, 5) if ct2pi else _phases(b, h, w, 5)
    ain = incoming_gauss(h, w) if with_ain else None
    with gpu.Zoom(b, h, w, (max(s[0] for s in sizes), max(s[1] for s in sizes))) as zm:
        zm.set_ain(ain)
        for size, split in zip(sizes, splits):
            want_i, want_v = _oneshot(gpu, holos, ORIGIN, PITCH, size, z, ain, ct2pi)
            zm.set_window(ORIGIN, PITCH, size, z)
            got_i, got_v = _run(zm, holos, ct2pi)
            assert got_i.shape == (b,) + size
            eq(got_i, want_i)
            eq(got_v, want_v)
            info = zm.info()
            print(f"zoom handle {label} window {size}: {info}")
            assert info["groups"] == 1 and info["bands"] == 1 and info["split_launches"] == split
            # fewer holograms than the handle's batch: the same bits
            part_i, part_v = _run(zm, holos[:b - 1], ct2pi)
            eq(part_i, want_i[:b - 1])
            eq(part_v, want_v[:b - 1])


# ---------------------------------------------------------------------------
# 2. resident state
# ---------------------------------------------------------------------------
def test_resident_state(gpu):
    h, w, b = 130, 264, 2
    holos = _phases(b, h, w, 9)
    ain = incoming_gauss(h, w)
    mask = np.random.default_rng(2).uniform(0, 2 * np.pi, (h, w))
    first, second = (ORIGIN, PITCH, (33, 70), 2e-4), ((1.5, -7.25), 0.25, (40, 33), 0.0)
    with gpu.Zoom(b, h, w, (40, 70)) as zm:
        zm.set_window(*first)
        one = _run(zm, holos)
        again = _run(zm, holos)  # no set_window in between
        eq(again[0], one[0])
        eq(again[1], one[1])
        zm.set_window(*second)
        other = _run(zm, holos)
        want = _oneshot(gpu, holos, second[0], second[1], second[2], second[3])
        eq(other[0], want[0])
        eq(other[1], want[1])
        zm.set_window(*first)
        back = _run(zm, holos)
        eq(back[0], one[0])
        eq(back[1], one[1])
        zm.set_ain(ain)
        zm.set_mask(mask)
        changed = _run(zm, holos)
        assert not np.array_equal(changed[0], one[0])
        zm.set_ain(None)
        zm.set_mask(None)
        plain = _run(zm, holos)
        eq(plain[0], one[0])
        eq(plain[1], one[1])
        want = _oneshot(gpu, holos, *first)
        eq(one[0], want[0])
        eq(one[1], want[1])


# ---------------------------------------------------------------------------
# 3. per-hologram windows
# ---------------------------------------------------------------------------
def test_per_hologram_windows(gpu):
    h, w, b, size = 130, 264, 4, (33, 70)
    holos = _phases(b, h, w, 13)
    ain = incoming_gauss(h, w)
    origins = np.array([[-3.375, 2.625], [5.5, -11.125], [0.0, 0.25], [-20.75, 17.0]])
    zs = np.array([2e-4, 0.0, 2e-4, 0.0])
    want_i, want_v = _oneshot(gpu, holos, origins, PITCH, size, zs, ain)
    with gpu.Zoom(b, h, w, size) as zm:
        zm.set_ain(ain)
        zm.set_window(origins, PITCH, size, zs)
        assert zm.per_hologram
        got_i, got_v = _run(zm, holos)
        eq(got_i, want_i)
        eq(got_v, want_v)
        # hologram 0 on a shared window is hologram 0 on window 0 of the per-hologram tables
        zm.set_window(origins[0], PITCH, size, zs[0])
        assert not zm.per_hologram
        shared_i, shared_v = _run(zm, holos[:1])
        eq(shared_i[0], want_i[0])
        eq(shared_v[0], want_v[0])


# ---------------------------------------------------------------------------
# 4. groups and bands
# ---------------------------------------------------------------------------
# whole-window partials of one hologram at (130, 264) / (96, 40): 1 chunk x 96 x 64 x 8 B = 49152 B.
# 32768 B: less than one hologram's, so 5 groups of one hologram in 2 bands of 64 and 32 rows;
# 100000 B: two holograms' whole windows, so 3 groups (2, 2, 1) of one band. Neither admits the
# split of the first product (133120 B per hologram), which the uncapped handle takes.
@pytest.mark.parametrize("cap,groups,bands", [(32768, 5, 2), (100000, 3, 1)])
def test_groups_and_bands(gpu, monkeypatch, cap, groups, bands):
    h, w, b, size = 130, 264, 5, (96, 40)
    holos = _phases(b, h, w, 17)
    origins = ORIGIN + np.arange(b)[:, None] * np.array([0.5, -1.25])
    zs = np.where(np.arange(b) % 2, 2e-4, 0.0)
    with gpu.Zoom(b, h, w, size) as zm:
        zm.set_window(origins, PITCH, size, zs)
        want = _run(zm, holos)
        assert zm.info() == {"groups": 1, "bands": 1, "split_launches": 1}
    monkeypatch.setenv("SLM_ZOOM_PARTIAL_BYTES", str(cap))
    with gpu.Zoom(b, h, w, size) as zm:
        zm.set_window(origins, PITCH, size, zs)
        got = _run(zm, holos)
        info = zm.info()
        print(f"zoom handle cap {cap}: {info}")
        assert info == {"groups": groups, "bands": bands, "split_launches": 0}
        eq(got[0], want[0])
        eq(got[1], want[1])
    monkeypatch.setenv("SLM_ZOOM_PARTIAL_BYTES", "many")
    with pytest.raises(gpu.SlmError) as ei:
        gpu.Zoom(b, h, w, size).set_ain(None)
    assert ei.value.code == gpu.ERR_ARG


# ---------------------------------------------------------------------------
# 5. the correction mask
# ---------------------------------------------------------------------------
def _gates(label, inten, field, ref, s_a):
    dv = np.abs(field - ref).max() / s_a
    di = np.abs(inten.astype(np.float64) - np.abs(ref) ** 2).max() / s_a ** 2
    print(f"zoom handle {label}: max|V - V_ref| = {dv:.3e} sum(a), max|I - I_ref| = {di:.3e} sum(a)^2")
    assert dv <= FIELDS_TOL
    assert di <= INTENSITY_TOL


@pytest.mark.parametrize("ct2pi", [None, 200], ids=["phase", "levels200"])
def test_mask_against_the_reference(gpu, ct2pi):
    h, w, size, z = 130, 264, (33, 70), 1e-4
    holos = _frames(2, h, w, 23) if ct2pi else _phases(2, h, w, 23)
    mask = np.random.default_rng(29).uniform(0, 2 * np.pi, (h, w))
    ain = incoming_gauss(h, w)
    origin, pitch = (-7.4375, 11.29), (0.125, 0.25)
    with gpu.Zoom(2, h, w, size) as zm:
        zm.set_ain(ain)
        zm.set_mask(mask)
        zm.set_window(origin, pitch, size, z)
        inten, field = _run(zm, holos, ct2pi)
    for b in range(2):
        ref = zhr.zoom(holos[b], origin, pitch, size, z=z, ain=ain, ct2pi=ct2pi, mask=mask)
        _gates(f"mask ct2pi={ct2pi} hologram {b}", inten[b], field[b], ref, zr.sum_a((h, w), ain))
        plain = zr.zoom(holos[b], origin, pitch, size, z=z, ain=ain, ct2pi=ct2pi)
        assert np.abs(ref - plain).max() > 1e3 * FIELDS_TOL * zr.sum_a((h, w), ain)  # the mask matters


@pytest.mark.parametrize("ct2pi", [256, 200])
def test_mask_off_identity(gpu, ct2pi):
    """frame = (levels + k) mod ct2pi with mask = k 2 pi / ct2pi: taking the mask
    off gives the field of `levels` again (2 pi (level + k) / ct2pi - mask is 2 pi
    level / ct2pi, or that plus 2 pi, to a few float64 ulps)."""
    h, w, size = 130, 264, (33, 70)
    rng = np.random.default_rng(ct2pi)
    levels = rng.integers(0, ct2pi, (1, h, w))
    k = rng.integers(0, ct2pi, (h, w))
    frame = ((levels + k) % ct2pi).astype(np.uint8)
    mask = k * (2 * np.pi / ct2pi)
    with gpu.Zoom(1, h, w, size) as zm:
        zm.set_window(ORIGIN, PITCH, size, 2e-4)
        _, plain = _run(zm, levels.astype(np.uint8), ct2pi)
        zm.set_mask(mask)
        _, masked = _run(zm, frame, ct2pi)
    dev = np.abs(masked - plain).max() / (h * w)
    print(f"zoom handle mask-off identity ct2pi={ct2pi}: {dev:.3e} sum(a)")
    assert dev <= 2 * FIELDS_TOL


# ---------------------------------------------------------------------------
# 6. the frames of a trap sequence, where they are
# ---------------------------------------------------------------------------
START = np.array([[-9.5, -14.25], [-6.0, 11.5], [7.25, -8.0], [10.5, 15.75], [0.5, 2.25]])
STEP = np.array([[0.25, 0.0], [0.0, -0.25], [-0.25, 0.25], [0.25, 0.25], [-0.25, -0.25]])


def _walk(n_frames, b):
    """ys, xs [F][B][M]: five traps drifting a quarter pixel per frame; hologram 1 is hologram 0 moved."""
    t = np.stack([START + f * STEP for f in range(n_frames)])  # [F][M][2]
    both = np.stack([t + np.array([1.75, -2.5]) * i for i in range(b)], axis=1)  # [F][B][M][2]
    return np.ascontiguousarray(both[..., 0]), np.ascontiguousarray(both[..., 1])


def _brightest(img):
    return np.unravel_index(img.argmax(), img.shape)


@pytest.mark.parametrize("with_mask", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("b", [1, 2])
def test_trap_sequence_frames_where_they_are(gpu, b, with_mask):
    from spatial_light_modulator_module_amd import move_traps as mt

    h, w, m, f = 45, 70, 5, 4
    ys, xs = _walk(f, b)
    mask = np.random.default_rng(11).uniform(0, 2 * np.pi, (h, w)) if with_mask else None
    origins, pitch, size = mt.trap_windows(ys.reshape(f, -1), xs.reshape(f, -1), margin=4.0, oversample=4)
    per_frame = np.repeat(origins, b, axis=0)  # flat index f B + b
    n = f * b
    with gpu.Spots(b, h, w, m, False, 12) as sp, gpu.Zoom(n, h, w, size) as zm:
        zm.set_window(per_frame, pitch, size)
        zm.set_mask(mask)
        sp.sequence(ys, xs, loops_first=12, loops=3, mask=mask, ct2pi=200)
        zm.run_spots(sp, 0, n, 200, return_field=True)  # enqueued behind the chain: no read in between
        got_i, got_v = zm.read()
        frames = sp.sequence_read()[0].reshape(n, h, w)
        host_i, host_v = _run(zm, frames, 200)
        eq(got_i, host_i)
        eq(got_v, host_v)
        # a part of the sequence: hologram i of the run is frame 1 + i, on window i
        zm.set_window(np.concatenate([per_frame[1:], per_frame[:1]]), pitch, size)
        zm.run_spots(sp, 1, n - 1, 200, return_field=True)
        part_i, part_v = zm.read()
        eq(part_i, got_i[1:])
        eq(part_v, got_v[1:])
        zm.set_window(per_frame, pitch, size)
        # without the mask taken off, the handle is the one-shot on every frame
        zm.set_mask(None)
        zm.run_spots(sp, 0, n, 200, return_field=True)
        raw_i, raw_v = zm.read()
        want_i, want_v = _oneshot(gpu, frames, per_frame, pitch, size, 0.0, None, 200)
        eq(raw_i, want_i)
        eq(raw_v, want_v)
        zm.set_mask(mask)
        # the traps are where the preview is brightest (with its mask taken off, if it has one)
        for i in range(n):
            j0, i0 = _brightest(got_i[i])
            fy, fx = ys.reshape(n, m)[i], xs.reshape(n, m)[i]
            near = min(max(abs(per_frame[i][0] + j0 * pitch[0] - y), abs(per_frame[i][1] + i0 * pitch[1] - x))
                       for y, x in zip(fy, fx))
            assert near <= pitch[0], (i, j0, i0)
        # order, both ways: this run reads the old frames although the next sequence is enqueued at once,
        # and the run after that sequence sees the new frames
        zm.run_spots(sp, 0, n, 200, return_field=True)
        sp.sequence(ys[::-1].copy(), xs[::-1].copy(), loops_first=12, loops=3, mask=mask, ct2pi=200)
        old_i, old_v = zm.read()
        eq(old_i, got_i)
        eq(old_v, got_v)
        zm.run_spots(sp, 0, n, 200, return_field=True)
        new_i, new_v = zm.read()
        new_frames = sp.sequence_read()[0].reshape(n, h, w)
        assert not np.array_equal(new_frames, frames)
        host_i, host_v = _run(zm, new_frames, 200)
        eq(new_i, host_i)
        eq(new_v, host_v)


def test_trap_array_sequence_expected(gpu):
    from spatial_light_modulator_module_amd import move_traps as mt

    h, w, f = 45, 70, 4
    ys, xs = _walk(f, 1)
    ys, xs = ys[:, 0], xs[:, 0]
    mask = np.random.default_rng(11).uniform(0, 2 * np.pi, (h, w))
    mt.clear_spots()
    kw = dict(loops_first=12, loops=3, ct2pi=200)
    res = mt.trap_array_sequence((h, w), ys, xs, **kw, expected=dict(oversample=4))
    window = mt.trap_window(ys, xs, oversample=4)
    assert res.expected.shape == (f,) + window[2] and res.expected.dtype == np.float32
    eq(res.expected, mt.expected_outcome(res.frames, window, ct2pi=200))
    follow = mt.trap_array_sequence((h, w), ys, xs, **kw, expected=dict(oversample=4, follow=True))
    origins, pitch, size = mt.trap_windows(ys, xs, oversample=4)
    eq(follow.frames, res.frames)
    for i in range(f):
        eq(follow.expected[i], mt.expected_outcome(res.frames[i], (tuple(origins[i]), pitch, size), ct2pi=200))
    # with the sequence's mask in the frames the preview is the aberrated one unless the mask is taken off
    masked = mt.trap_array_sequence((h, w), ys, xs, **kw, mask=mask, expected=dict(oversample=4))
    eq(masked.expected, mt.expected_outcome(masked.frames, window, ct2pi=200))
    off = mt.trap_array_sequence((h, w), ys, xs, **kw, mask=mask, expected=dict(oversample=4, mask_off=True))
    eq(off.frames, masked.frames)
    for i in range(f):
        ref = zhr.zoom(off.frames[i], window[0], window[1][0], window[2], ct2pi=200, mask=mask)
        assert np.abs(off.expected[i] - np.abs(ref) ** 2).max() <= INTENSITY_TOL * (h * w) ** 2
        assert off.expected[i].max() > 4 * masked.expected[i].max()  # the traps are back
    batch = mt.trap_array_sequence((h, w), *_walk(f, 2), **kw, expected=dict(oversample=4, follow=True))
    assert batch.expected.shape[:2] == (f, 2)
    mt.clear_spots()
    assert not mt._ZOOMS and not mt._SPOTS


# ---------------------------------------------------------------------------
# 7. the frames of an image sequence
# ---------------------------------------------------------------------------
def test_plan_sequence_frames(gpu):
    h = w = 64
    rng = np.random.default_rng(31)
    targets = np.zeros((3, 1, h, w), np.uint8)
    for fr in range(3):
        for _ in range(6):
            j, i = rng.integers(4, h - 4, 2)
            targets[fr, 0, j - 1:j + 2, i - 1:i + 2] = 255
    size = (40, 33)
    with gpu.Plan(gpu.ALGO_GS, 1, h, w, gpu.TGT_U8, False, 6) as plan, gpu.Zoom(3, h, w, size) as zm:
        zm.set_window((-5.5, 3.25), 0.25, size)
        plan.sequence(targets, loops_first=6, loops=3, ct2pi=200.0, frames=True)
        zm.run_plan(plan, 0, 3, 200, return_field=True)
        got_i, got_v = zm.read()
        frames = plan.sequence_read()[0].reshape(3, h, w)
        host_i, host_v = _run(zm, frames, 200)
        eq(got_i, host_i)
        eq(got_v, host_v)
        assert got_i.max() > 0
        zm.run_plan(plan, 2, 1, 200, return_field=True)
        last_i, last_v = zm.read()
        eq(last_i[0], got_i[2])
        eq(last_v[0], got_v[2])


# ---------------------------------------------------------------------------
# 8. refusals of the C boundary
# ---------------------------------------------------------------------------
def test_refusals(gpu):
    import ctypes

    lib = gpu.load()
    h, w, ny, nx = 8, 12, 4, 5
    ph = np.zeros((2, h, w), np.float32)
    fr = np.zeros((2, h, w), np.uint8)
    zero = np.zeros(1)
    quarter = 0.25

    def code(rc, want):
        assert rc == want, (rc, gpu.last_error())
        assert gpu.last_error()

    def create(batch=2, height=h, width=w, max_ny=ny, max_nx=nx):
        out = ctypes.c_void_p()
        return lib.slm_zoom_create(batch, height, width, max_ny, max_nx, ctypes.byref(out)), out

    for bad in (dict(batch=0), dict(batch=1025), dict(height=1), dict(height=4097), dict(width=1), dict(width=4097),
                dict(max_ny=0), dict(max_ny=4097), dict(max_nx=0), dict(max_nx=4097)):
        code(create(**bad)[0], gpu.ERR_ARG)
    rc, zm = create()
    assert rc == 0

    def window(y0=0.0, x0=0.0, z=0.0, dy=quarter, dx=quarter, n_y=ny, n_x=nx):
        a, b, c = np.array([y0]), np.array([x0]), np.array([z])
        return lib.slm_zoom_set_window(zm, 0, gpu.ptr(a), gpu.ptr(b), gpu.ptr(c), dy, dx, n_y, n_x)

    def run(holo=ph, kind=gpu.ZOOM_PHASE_F32, count=2, ct2pi=0.0, want_field=0):
        return lib.slm_zoom_run(zm, gpu.ptr(holo), kind, count, ct2pi, want_field)

    out_i = np.zeros((2, ny, nx), np.float32)
    out_v = np.zeros((2, ny, nx), np.complex128)
    us = np.zeros(gpu.ZOOM_NUM_KERNEL_CLASSES)
    code(run(), gpu.ERR_STATE)  # before set_window
    code(lib.slm_zoom_read(zm, gpu.ptr(out_i), None, None), gpu.ERR_STATE)  # before a run
    code(lib.slm_zoom_info(zm, gpu.ptr(np.zeros(3, np.int32))), gpu.ERR_STATE)
    # the window: the one-shot's refusals, and the handle's own size
    code(window(n_y=ny + 1), gpu.ERR_ARG)
    code(window(n_x=nx + 1), gpu.ERR_ARG)
    for n in (0, 4097):
        code(window(n_y=n), gpu.ERR_ARG)
        code(window(n_x=n), gpu.ERR_ARG)
    for bad in (np.nan, np.inf, -np.inf):
        for name in ("y0", "x0", "z", "dy", "dx"):
            code(window(**{name: bad}), gpu.ERR_ARG)
    for name in ("dy", "dx"):
        code(window(**{name: 0.0}), gpu.ERR_ARG)
        code(window(**{name: -0.25}), gpu.ERR_ARG)
    code(lib.slm_zoom_set_window(zm, 0, None, gpu.ptr(zero), gpu.ptr(zero), quarter, quarter, ny, nx), gpu.ERR_ARG)
    code(run(), gpu.ERR_STATE)  # a refused window is no window
    assert window() == 0
    # a_in and the mask
    bad_ain = np.ones((h, w), np.float32)
    bad_ain[2, 3] = np.inf
    code(lib.slm_zoom_set_ain(zm, gpu.ptr(bad_ain)), gpu.ERR_ARG)
    code(lib.slm_zoom_set_ain(zm, gpu.ptr(np.zeros((h, w), np.float32))), gpu.ERR_ARG)
    for bad in (np.nan, np.inf):
        bad_mask = np.zeros((h, w))
        bad_mask[5, 7] = bad
        code(lib.slm_zoom_set_mask(zm, gpu.ptr(bad_mask)), gpu.ERR_ARG)
    # the run
    code(run(holo=None), gpu.ERR_ARG)
    code(run(kind=2), gpu.ERR_ARG)
    code(run(kind=-1), gpu.ERR_ARG)
    code(run(count=0), gpu.ERR_ARG)
    code(run(count=3), gpu.ERR_ARG)
    for bad in (0.0, -200.0, np.nan, np.inf):
        code(run(holo=fr, kind=gpu.ZOOM_LEVELS_U8, ct2pi=bad), gpu.ERR_ARG)
    code(lib.slm_zoom_read(zm, gpu.ptr(out_i), None, None), gpu.ERR_STATE)  # still no run
    assert run() == 0
    assert lib.slm_zoom_read(zm, gpu.ptr(out_i), None, None) == 0
    code(lib.slm_zoom_read(zm, None, out_v.ctypes.data, None), gpu.ERR_STATE)  # the field was not asked for
    code(lib.slm_zoom_read(zm, None, None, gpu.ptr(us)), gpu.ERR_STATE)       # the run was not timed
    assert lib.slm_zoom_set_timed(zm, 1) == 0
    assert run(holo=fr, kind=gpu.ZOOM_LEVELS_U8, ct2pi=200.0, want_field=1) == 0
    assert lib.slm_zoom_read(zm, gpu.ptr(out_i), out_v.ctypes.data, gpu.ptr(us)) == 0
    assert us[gpu.ZOOM_KERNEL_TABLES] == 0 and (us[1:] > 0).all()
    assert out_i[0, 0, 0] == np.float32((h * w) ** 2)  # level 0 everywhere: every pixel in phase at bin (0, 0)
    # sequences: none, frames not kept, another shape, a range past the end
    ys = np.array([[[1.0, -2.0]], [[1.25, -2.0]]])  # [F 2][B 1][M 2]
    xs = np.array([[[2.0, 3.0]], [[2.0, 3.25]]])
    with gpu.Spots(1, h, w, 2, False, 4) as sp, gpu.Spots(1, h, w + 2, 2, False, 4) as wide:
        code(lib.slm_zoom_run_spots(zm, sp.handle, 0, 1, 200.0, 0), gpu.ERR_STATE)
        sp.sequence(ys, xs, loops_first=4, loops=2, frames=False)
        code(lib.slm_zoom_run_spots(zm, sp.handle, 0, 1, 200.0, 0), gpu.ERR_STATE)
        sp.sequence(ys, xs, loops_first=4, loops=2)
        wide.sequence(ys, xs, loops_first=4, loops=2)
        code(lib.slm_zoom_run_spots(zm, wide.handle, 0, 1, 200.0, 0), gpu.ERR_ARG)
        for first, count in ((-1, 1), (1, 2), (2, 1), (0, 0), (0, 3)):
            code(lib.slm_zoom_run_spots(zm, sp.handle, first, count, 200.0, 0), gpu.ERR_ARG)
        code(lib.slm_zoom_run_spots(zm, sp.handle, 0, 2, 0.0, 0), gpu.ERR_ARG)
        code(lib.slm_zoom_run_spots(zm, None, 0, 2, 200.0, 0), gpu.ERR_ARG)
        assert lib.slm_zoom_run_spots(zm, sp.handle, 0, 2, 200.0, 0) == 0
        assert lib.slm_zoom_read(zm, gpu.ptr(out_i), None, None) == 0
    assert lib.slm_zoom_destroy(zm) == 0
    rc, zm = create(height=64, width=64)
    assert rc == 0 and window() == 0
    targets = np.zeros((2, 1, 64, 64), np.uint8)
    targets[:, 0, 20:24, 30:34] = 255
    with gpu.Plan(gpu.ALGO_GS, 1, 64, 64, gpu.TGT_U8, False, 4) as plan, \
            gpu.Plan(gpu.ALGO_GS, 1, 128, 64, gpu.TGT_U8, False, 4) as tall:
        code(lib.slm_zoom_run_plan(zm, plan.handle, 0, 1, 256.0, 0), gpu.ERR_STATE)
        plan.sequence(targets, loops_first=3, loops=2, frames=False)
        code(lib.slm_zoom_run_plan(zm, plan.handle, 0, 1, 256.0, 0), gpu.ERR_STATE)
        plan.sequence(targets, loops_first=3, loops=2)
        tall.sequence(np.zeros((2, 1, 128, 64), np.uint8) + targets[0, 0, 20, 30], loops_first=3, loops=2)
        code(lib.slm_zoom_run_plan(zm, tall.handle, 0, 1, 256.0, 0), gpu.ERR_ARG)
        for first, count in ((-1, 1), (1, 2), (2, 1), (0, 0), (0, 3)):
            code(lib.slm_zoom_run_plan(zm, plan.handle, first, count, 256.0, 0), gpu.ERR_ARG)
        code(lib.slm_zoom_run_plan(zm, None, 0, 2, 256.0, 0), gpu.ERR_ARG)
        assert lib.slm_zoom_run_plan(zm, plan.handle, 0, 2, 256.0, 0) == 0
        assert lib.slm_zoom_read(zm, gpu.ptr(out_i), None, None) == 0
    assert lib.slm_zoom_destroy(zm) == 0


# ---------------------------------------------------------------------------
# 9. the CLI
# ---------------------------------------------------------------------------
def _png_bytes(img, path):
    from PIL import Image

    img = img.astype(np.float64)
    Image.fromarray(np.floor(255.0 * img / (img.max() or 1.0)).astype(np.uint8)).save(path)
    return open(path, "rb").read()


def test_cli_expected_and_follow(gpu, tmp_path, monkeypatch):
    from PIL import Image

    from spatial_light_modulator_module_amd import generate_trap_sequence as gts
    from spatial_light_modulator_module_amd import move_traps as mt

    f = 3
    traj = np.stack([START[:4] + i * STEP[:4] for i in range(f)])  # [F][M][2]
    os.makedirs(tmp_path / "images" / "moving_traps")
    np.save(tmp_path / "images" / "moving_traps" / "walk.npy", traj)
    monkeypatch.chdir(tmp_path)
    base = ["walk", "-ct2pi", "256", "--shape", "45x70", "-first", "20", "-loops", "4", "--oversample", "4"]
    gts.cli(base + ["-v", "1", "--expected", "-p"])
    gts.cli(base + ["-v", "2", "--expected", "--follow"])
    frames = np.stack([np.array(Image.open(tmp_path / "images" / "moving_traps" / "walk_1_preview" / f"{i}.png"))
                       for i in range(f)])
    assert frames.dtype == np.uint8 and frames.shape == (f, 45, 70)
    # the path the CLI took before the handle: the frames from the host through the one-shot
    window = mt.trap_window(traj[:, :, 0], traj[:, :, 1], margin=4.0, oversample=4)
    want = gpu.farfield_zoom(frames, *window, ct2pi=256)
    dest = tmp_path / "images" / "moving_traps" / "walk_1_expected"
    assert sorted(os.listdir(dest)) == [f"{i}.png" for i in range(f)]
    for i in range(f):
        assert open(dest / f"{i}.png", "rb").read() == _png_bytes(want[i], tmp_path / "want.png")
    origins, pitch, size = mt.trap_windows(traj[:, :, 0], traj[:, :, 1], margin=4.0, oversample=4)
    dest = tmp_path / "images" / "moving_traps" / "walk_2_expected"
    assert sorted(os.listdir(dest)) == [f"{i}.png" for i in range(f)]
    for i in range(f):
        png = np.array(Image.open(dest / f"{i}.png"))
        assert png.shape == size and png.dtype == np.uint8 and png.max() == 255
        assert size[0] < window[2][0] or size[1] < window[2][1]
        img = png.astype(np.float64)
        want_at = [((y - origins[i][0]) / pitch[0], (x - origins[i][1]) / pitch[1]) for y, x in traj[i]]
        found = set()
        for _ in range(4):  # a trap's main lobe ends 4 samples from it: set aside 6 around each maximum
            j, k = np.unravel_index(img.argmax(), img.shape)
            near = [max(abs(j - wj), abs(k - wk)) for wj, wk in want_at]
            assert min(near) <= 1.0, (i, j, k, want_at)
            found.add(int(np.argmin(near)))
            img[max(0, j - 6):j + 7, max(0, k - 6):k + 7] = -1.0
        assert len(found) == 4
    mt.clear_spots()
