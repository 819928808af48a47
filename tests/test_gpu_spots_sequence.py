"""Trap trajectories (slm_spots_sequence) on the MI355X: the identities that
must hold bit for bit (frames of one list are one long run, a sequence cut in
two with resume is the uncut one, a handle whose buffers have grown computes
what a fresh one does, a frame the device stopped is that frame run for
exactly as many iterations), parity of a moving list with the float64
NumPy chain (tests/spots_sequence_reference.py) from a warm start as
tests/test_gpu_spots.py sets it up, the tolerance stop against the reference's
iteration counts, and the refusals."""
import os

import numpy as np
import pytest

import spots_reference as sr
import spots_sequence_reference as ssr
from gsw_reference import incoming_gauss
from oracle import gs_gd_oracle as orc

PHASE_RMS_TOL = 1e-5
WEIGHT_TOL = 5e-6
# 10x the largest deviation from the float64 chain the MI355X showed when these
# tests were first run (test_sequence_parity's docstring), capped at 1e-5: the
# rule tests/test_gpu_spots.py states for the same two gates
INTENSITY_RTOL = 2.44e-6  # measured 2.437e-7
STATS_TOL = 2.43e-6       # measured 2.428e-7


def _cols(lists_per_hologram):
    """[hologram][frame](ys, xs, zs, intensity) -> four arrays [F][B][M]."""
    return [np.stack([np.stack([li[k] for li in traj]) for traj in lists_per_hologram], axis=1) for k in range(4)]


def _mask(shape):
    return np.random.default_rng(11).uniform(0, 2 * np.pi, shape)


def _assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ---------------------------------------------------------------------------
# 1. frames of one list are one long run
# ---------------------------------------------------------------------------
SAME_LIST = [("45x70-5", (45, 70), 5, (3,)), ("96x160-33", (96, 160), 33, (3,)), ("2x96x160-33", (96, 160), 33, (5, 6))]


@pytest.mark.gpu
@pytest.mark.parametrize("label,shape,m,seeds", SAME_LIST, ids=[c[0] for c in SAME_LIST])
def test_same_list_is_one_run(gpu, label, shape, m, seeds):
    h, w = shape
    b = len(seeds)
    lists = [sr.trap_list(h, w, m, s) for s in seeds]
    one = [np.stack([li[k] for li in lists]) for k in range(4)]
    cols = _cols([[li] * 4 for li in lists])
    # the batch case also starts from a caller's phase and weights
    rng = np.random.default_rng(2)
    ph0 = rng.uniform(-np.pi, np.pi, (b, h, w)).astype(np.float32) if b > 1 else None
    w0 = rng.uniform(0.8, 1.2, (b, m)).astype(np.float32) if b > 1 else None
    mask = _mask(shape)
    with gpu.Spots(b, h, w, m, False, 20) as sp:
        sp.set_traps(*one)
        sp.set_phase(ph0)
        sp.set_weights(w0)
        sp.run(20)
        phase, v, stats, wt = sp.read()
        first = True
        for rule in (gpu.QUANT_ASTYPE, gpu.QUANT_PIL):
            for mk in (None, mask):
                for ct2pi in (256, 255):
                    sp.sequence(*cols, weights0=w0, loops_first=5, loops=5, tol=0.0, mask=mk, ct2pi=ct2pi, rule=rule,
                                frames=True, phases=True)
                    fr, ph, sv, ss, sw, it = sp.sequence_read(phases=True)
                    assert fr.shape == (4, b, h, w) and fr.dtype == np.uint8 and ss.shape == (4, b, 5, 4)
                    np.testing.assert_array_equal(it, np.full((4, b), 5))
                    np.testing.assert_array_equal(ph[3], phase)
                    np.testing.assert_array_equal(sv[3], v)
                    np.testing.assert_array_equal(sw[3], wt)
                    np.testing.assert_array_equal(np.concatenate(list(ss), axis=1), stats)
                    want = gpu.quantize(ph.astype(np.float64), mk, ct2pi, rule)
                    np.testing.assert_array_equal(fr, want)
                    if first:
                        assert len(np.unique(fr)) > 100  # real levels, not a constant
                        assert not np.array_equal(ph[0], ph[3])
                        first = False


# ---------------------------------------------------------------------------
# 2. a sequence cut in two with resume is the uncut sequence
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_resume_is_the_uncut_sequence(gpu):
    h, w, m = 96, 160, 33
    cols = _cols([ssr.trajectory(h, w, m, 3, 6)])
    kw = dict(loops_first=6, loops=3, tol=0.0, mask=_mask((h, w)), ct2pi=200, frames=True, phases=True)
    with gpu.Spots(1, h, w, m, False, 6) as sp:
        sp.sequence(*cols, **kw)
        whole = sp.sequence_read(phases=True)
        sp.sequence(*[c[:3] for c in cols], **kw)
        head = sp.sequence_read(phases=True)
        sp.sequence(*[c[3:] for c in cols], resume=True, **kw)
        tail = sp.sequence_read(phases=True)
    np.testing.assert_array_equal(whole[5][:, 0], [6, 3, 3, 3, 3, 3])
    for a, hd, tl in zip(whole, head, tail):
        np.testing.assert_array_equal(a, np.concatenate([hd, tl]))
    assert not np.array_equal(whole[1][2], whole[1][3])


# ---------------------------------------------------------------------------
# 2b. a handle whose buffers have grown computes what a fresh one does
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_handle_that_has_grown(gpu):
    """One handle takes a short sequence of few traps, a longer one of more
    traps with a mask (every sequence buffer and the partial sums grow), a
    list of max_traps traps and a run (the partial sums grow again), and the
    first sequence once more in buffers that are now larger than it needs.
    Everything read back after each call equals the same call on a fresh handle."""
    h, w, max_traps, max_loops = 45, 70, 70, 6
    mask = _mask((h, w))

    def sequence(m, n_frames, mk):
        def call(sp):
            sp.sequence(*_cols([ssr.trajectory(h, w, m, 4, n_frames)]), loops_first=6, loops=3, tol=0.0, mask=mk,
                        ct2pi=200, frames=True, phases=True)
            return sp.sequence_read(phases=True)
        return call

    def run(sp):
        sp.set_traps(*sr.trap_list(h, w, max_traps, 4))
        sp.run(max_loops)
        return sp.read()

    with gpu.Spots(1, h, w, max_traps, False, max_loops) as grown:
        for call in (sequence(5, 2, None), sequence(33, 5, mask), run, sequence(5, 2, None)):
            got = call(grown)
            with gpu.Spots(1, h, w, max_traps, False, max_loops) as fresh:
                _assert_same(got, call(fresh))
    assert got[0].shape == (2, 1, h, w) and len(np.unique(got[0])) > 100  # real frames, not a constant


# ---------------------------------------------------------------------------
# 3. parity with the float64 chain from a warm start
# ---------------------------------------------------------------------------
PARITY = [
    # id, shape, trap-list seeds (one per hologram), traps, feedback, a_in
    ("45x70-5", (45, 70), (3,), 5, 1.0, False),
    ("96x160-33", (96, 160), (3,), 33, 1.0, False),
    ("96x160-33-p0.5", (96, 160), (3,), 33, 0.5, False),
    ("130x264-70", (130, 264), (3,), 70, 1.0, False),
    ("96x160-33-ain", (96, 160), (3,), 33, 1.0, True),
    ("2x96x160-33", (96, 160), (5, 6), 33, 1.0, False),
]
WARM, LOOPS, FRAMES = 30, 8, 5


@pytest.mark.gpu
@pytest.mark.parametrize("label,shape,seeds,m,feedback,with_ain", PARITY, ids=[c[0] for c in PARITY])
def test_sequence_parity(gpu, label, shape, seeds, m, feedback, with_ain):
    """30 reference iterations on list 0; the phase and the weights rounded to
    float32 go to both sides, which then run frames 1 .. 5 of the trajectory at
    8 iterations each. Measured (MI355X) when first run, the worst frame of
    each of these six cases: phase rms 2.4e-7 .. 9.3e-7 of the 1e-5 bar, max
    |dw| 8.4e-8 .. 1.3e-7 of 5e-6, per-trap intensities within 1.4e-7 ..
    2.437e-7 relative, the four statistics (efficiency relative, the others
    absolute) within 1.5e-7 .. 2.428e-7; no growth from frame 1 to frame 5.
    The last two gates are 10x those largest figures."""
    h, w = shape
    ain = incoming_gauss(h, w) if with_ain else None
    trajs = [ssr.trajectory(h, w, m, s, FRAMES + 1) for s in seeds]
    ph0, w0, want = [], [], []
    for tr in trajs:
        ph, _, _, wt = sr.spots_reference(shape, *tr[0], loops=WARM, feedback=feedback, ain=ain)
        ph0.append(ph.astype(np.float32))
        w0.append(wt.astype(np.float32))
        want.append(ssr.sequence_reference(shape, tr[1:], LOOPS, LOOPS, 0.0, feedback, ain, ph0[-1], w0[-1]))
    with gpu.Spots(len(seeds), h, w, m, with_ain, LOOPS) as sp:
        if with_ain:
            sp.set_ain(ain)
        sp.set_feedback(feedback)
        sp.set_phase(np.stack(ph0))
        sp.sequence(*_cols([tr[1:] for tr in trajs]), weights0=np.stack(w0), loops_first=LOOPS, loops=LOOPS, tol=0.0,
                    frames=False, phases=True)
        _, phase, v, stats, wt, iters = sp.sequence_read(frames=False, phases=True)
    assert stats.shape == (FRAMES, len(seeds), LOOPS, 4) and np.all(iters == LOOPS)
    worst = np.zeros(4)
    for k in range(len(seeds)):
        for f in range(FRAMES):
            ref = want[k][f]
            rms = orc.phase_rms(phase[f, k], ref[0])
            dw = float(np.max(np.abs(wt[f, k].astype(np.float64) - ref[3])))
            di = float(np.max(np.abs(np.abs(v[f, k]) ** 2 / np.abs(ref[1]) ** 2 - 1)))
            ds = np.abs(stats[f, k] - ref[2])
            ds[:, 0] /= ref[2][:, 0]  # the efficiency relative, the others absolute
            ds = float(ds.max())
            print(f"[spots sequence parity] {label}[{k}] frame {f + 1} p={feedback}: phase rms {rms:.3e}, "
                  f"max |dw| {dw:.3e}, intensities max rel {di:.3e}, statistics max dev {ds:.3e}")
            worst = np.maximum(worst, [rms, dw, di, ds])
    print(f"[spots sequence parity] {label} worst: phase rms {worst[0]:.3e}, max |dw| {worst[1]:.3e}, "
          f"intensities {worst[2]:.3e}, statistics {worst[3]:.3e}")
    assert worst[0] <= PHASE_RMS_TOL
    assert worst[1] <= WEIGHT_TOL
    assert worst[2] <= INTENSITY_RTOL
    assert worst[3] <= STATS_TOL


# ---------------------------------------------------------------------------
# 4. the tolerance stop
# ---------------------------------------------------------------------------
TOL = 0.01
TOL_MARGIN = 1.2e-4  # 60x the statistics deviation test_gpu_spots.py measured: rounding cannot move a stop
STOPS = [("96x160-33", (96, 160), 33, [9, 6, 4, 4, 4, 4]), ("45x70-5", (45, 70), 5, [2, 4, 4, 4, 4, 3])]
_SEQ_KW = dict(loops_first=30, loops=8, frames=True, phases=True, ct2pi=256)


def _frame_outputs(out, f, n):
    """Frame f of a sequence_read(phases=True), hologram axis kept, statistics cut to n rows."""
    fr, ph, v, st, wt, it = out
    return fr[f], ph[f], v[f], st[f][:, :n], wt[f], it[f]


@pytest.mark.gpu
@pytest.mark.parametrize("label,shape,m,expected", STOPS, ids=[c[0] for c in STOPS])
def test_tolerance_stop(gpu, label, shape, m, expected):
    h, w = shape
    traj = ssr.trajectory(h, w, m, 3, 6)
    ref = ssr.sequence_reference(shape, traj, 30, 8, TOL)
    assert [fr[4] for fr in ref] == expected
    assert ssr.tol_margin(ref, TOL) >= TOL_MARGIN
    cols = _cols([traj])
    with gpu.Spots(1, h, w, m, False, 30) as sp, gpu.Spots(1, h, w, m, False, 30) as fixed:
        sp.sequence(*cols, tol=TOL, **_SEQ_KW)
        got = sp.sequence_read(phases=True)
        iters = got[5][:, 0]
        print(f"[spots sequence stop] {label}: iterations per frame {iters.tolist()}, reference {expected}")
        np.testing.assert_array_equal(iters, expected)
        assert got[3].shape == (6, 1, 30, 4)
        for f in range(6):
            n = expected[f]
            assert np.all(got[3][f, 0, n:] == 0) and np.all(got[3][f, 0, :n, 0] > 0)
            assert np.all(got[3][f, 0, :n - 1, 1] > TOL)
            assert got[3][f, 0, n - 1, 1] <= TOL or n == (30 if f == 0 else 8)
            # the same frame with its count fixed: one call per frame, resumed
            fixed.sequence(*[c[f:f + 1] for c in cols], tol=0.0, resume=f > 0, **dict(_SEQ_KW, loops_first=n, loops=n))
            _assert_same(_frame_outputs(fixed.sequence_read(phases=True), 0, n), _frame_outputs(got, f, n))


@pytest.mark.gpu
def test_batch_stops_per_hologram(gpu):
    h, w, m = 96, 160, 33
    trajs = [ssr.trajectory(h, w, m, s, 6) for s in (3, 5)]
    want_iters = []
    for tr in trajs:
        ref = ssr.sequence_reference((h, w), tr, 30, 8, TOL)
        assert ssr.tol_margin(ref, TOL) >= TOL_MARGIN
        want_iters.append([fr[4] for fr in ref])
    assert want_iters[0] != want_iters[1]
    with gpu.Spots(2, h, w, m, False, 30) as sp:
        sp.sequence(*_cols(trajs), tol=TOL, **_SEQ_KW)
        both = sp.sequence_read(phases=True)
    np.testing.assert_array_equal(both[5], np.array(want_iters).T)
    for k, tr in enumerate(trajs):
        with gpu.Spots(1, h, w, m, False, 30) as sp:
            sp.sequence(*_cols([tr]), tol=TOL, **_SEQ_KW)
            solo = sp.sequence_read(phases=True)
        for a, b in zip(both, solo):
            np.testing.assert_array_equal(a[:, k], b[:, 0])


# ---------------------------------------------------------------------------
# 5. a moved list becomes uniform again in a few iterations
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_uniformity_is_restored(gpu):
    h, w, m = 96, 160, 12
    with gpu.Spots(1, h, w, m, False, 30) as sp:
        sp.sequence(*_cols([ssr.trajectory(h, w, m, 3, 6)]), loops_first=30, loops=4, tol=0.0, frames=False)
        _, _, _, stats, _, iters = sp.sequence_read(frames=False)
    for f in range(6):
        u = stats[f, 0, :iters[f, 0], 1]
        print(f"[spots sequence] 96x160 12 traps frame {f}: uniformity {u[0]:.3e} -> {u[-1]:.3e} "
              f"in {iters[f, 0]} iterations")
        assert u[-1] < u[0]
        assert u[-1] <= 0.02


# ---------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(gpu):
    def refused(code, call):
        with pytest.raises(gpu.SlmError) as ei:
            call()
        assert ei.value.code == code

    h, w, m = 64, 64, 4
    cols = _cols([ssr.trajectory(h, w, m, 1, 3)])
    ys, xs, zs, inten = cols

    def poisoned(a, bad):
        a = a.copy()
        a[2, 0, 1] = bad  # in the last frame: every frame is checked
        return a

    with gpu.Spots(1, h, w, m, False, 5) as sp:
        seq = lambda *a, **k: sp.sequence(*a, **dict(dict(loops_first=5, loops=2), **k))  # noqa: E731
        refused(gpu.ERR_STATE, lambda: sp.sequence_read())  # a read before a sequence
        refused(gpu.ERR_STATE, lambda: seq(*cols, resume=True))  # nothing to resume
        for bad in (np.nan, np.inf, -np.inf):
            refused(gpu.ERR_ARG, lambda: seq(poisoned(ys, bad), xs, zs, inten))
            refused(gpu.ERR_ARG, lambda: seq(ys, poisoned(xs, bad), zs, inten))
            refused(gpu.ERR_ARG, lambda: seq(ys, xs, poisoned(zs, bad), inten))
        for bad in (0.0, -1.0, np.nan, np.inf):
            refused(gpu.ERR_ARG, lambda: seq(ys, xs, zs, poisoned(inten, bad)))
            refused(gpu.ERR_ARG, lambda: seq(*cols, weights0=np.array([1, bad, 1, 1.0])))
        refused(gpu.ERR_ARG, lambda: seq(np.zeros((3, 1, 5)), np.zeros((3, 1, 5))))  # n_traps > max_traps
        lib, hd = gpu.load(), sp.handle
        args = (gpu.ptr(ys), gpu.ptr(xs), None, None, None)
        for n_frames, n_traps in ((0, m), (3, 0)):  # the wrapper never passes these: straight to the C entry
            refused(gpu.ERR_ARG, lambda: gpu.check(
                lib.slm_spots_sequence(hd, n_frames, n_traps, *args, 5, 2, 0.0, 0, None, 256.0, 0, 1, 0),
                "slm_spots_sequence"))
        for lf, lo in ((0, 2), (6, 2), (5, 0), (5, 6)):
            refused(gpu.ERR_ARG, lambda: seq(*cols, loops_first=lf, loops=lo))
        for bad in (-1e-3, np.nan, np.inf):
            refused(gpu.ERR_ARG, lambda: seq(*cols, tol=bad))
        for bad in (-1, 2):
            refused(gpu.ERR_ARG, lambda: seq(*cols, rule=bad))
        for bad in (0.0, -256.0, np.nan, np.inf):
            refused(gpu.ERR_ARG, lambda: seq(*cols, ct2pi=bad))
        refused(gpu.ERR_STATE, lambda: sp.sequence_read())  # none of the refused calls left a sequence
        # a sequence; what it did not keep cannot be read
        seq(*cols, frames=False, phases=False)
        refused(gpu.ERR_STATE, lambda: sp.sequence_read(frames=True))
        refused(gpu.ERR_STATE, lambda: sp.sequence_read(frames=False, phases=True))
        base = sp.sequence_read(frames=False)
        refused(gpu.ERR_ARG, lambda: seq(*cols, resume=True, weights0=np.ones(4)))
        # resume: another trap count, then after every setter and after a run
        refused(gpu.ERR_STATE, lambda: seq(ys[:, :, :3], xs[:, :, :3], resume=True))
        seq(*cols, resume=True, frames=False)
        for touch in (lambda: sp.set_traps(ys[0], xs[0]), lambda: sp.set_phase(None), lambda: sp.set_weights(None),
                      lambda: sp.set_feedback(1.0), lambda: sp.run(2)):
            seq(*cols, frames=False)
            touch()
            refused(gpu.ERR_STATE, lambda: seq(*cols, resume=True))
        # after a sequence the handle is as after set_traps with the last list
        seq(*cols, frames=False)
        _assert_same(sp.sequence_read(frames=False), base)
        refused(gpu.ERR_STATE, lambda: sp.read())
        sp.run(5)
        after = sp.read()
    with gpu.Spots(1, h, w, m, False, 5) as sp:
        sp.set_traps(ys[2], xs[2], zs[2], inten[2])
        sp.run(5)
        _assert_same(sp.read(), after)
    with gpu.Spots(1, h, w, m, True, 5) as sp:
        refused(gpu.ERR_STATE, lambda: sp.sequence(*cols, loops_first=5, loops=2))  # has_ain, no a_in yet
        sp.set_ain(incoming_gauss(h, w))
        sp.sequence(*cols, loops_first=5, loops=2)
        assert sp.sequence_read()[0].shape == (3, 1, h, w)


# ---------------------------------------------------------------------------
# 7. the Python layer and the CLI
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_python_layer(gpu):
    from spatial_light_modulator_module_amd import move_traps as mt

    shape, m = (45, 70), 5
    traj = ssr.trajectory(45, 70, m, 8, 4)
    ys, xs, zs, inten = (np.stack([li[k] for li in traj]) for k in range(4))
    mask = _mask(shape)
    mt.clear_spots()
    res = mt.trap_array_sequence(shape, ys, xs, zs, inten, loops_first=12, loops=3, mask=mask, ct2pi=200,
                                 holograms=True)
    assert res.frames.shape == (4,) + shape and res.frames.dtype == np.uint8
    assert res.holograms.shape == (4,) + shape and res.holograms.dtype == np.float64
    assert res.intensities.shape == (4, m) and res.weights.shape == (4, m)
    assert res.stats.shape == (4, 12, 4) and res.iters.tolist() == [12, 3, 3, 3]
    holo, frame, trap_i, stats, wt = mt.trap_array_frame(shape, ys[0], xs[0], zs[0], inten[0], loops=12, mask=mask,
                                                        ct2pi=200)
    np.testing.assert_array_equal(res.holograms[0], holo)
    np.testing.assert_array_equal(res.frames[0], frame)
    np.testing.assert_array_equal(res.intensities[0], trap_i)
    np.testing.assert_array_equal(res.stats[0], stats)
    np.testing.assert_array_equal(res.weights[0], wt)
    # trap_array_frame went through the handle's setters: nothing to resume
    with pytest.raises(ValueError, match="resume"):
        mt.trap_array_sequence(shape, ys[2:], xs[2:], zs[2:], inten[2:], loops_first=12, loops=3, resume=True)
    # cut in two with resume, and a batch of two trajectories
    head = mt.trap_array_sequence(shape, ys[:2], xs[:2], zs[:2], inten[:2], loops_first=12, loops=3, mask=mask,
                                  ct2pi=200)
    tail = mt.trap_array_sequence(shape, ys[2:], xs[2:], zs[2:], inten[2:], loops_first=12, loops=3, mask=mask,
                                  ct2pi=200, resume=True)
    assert head.holograms is None
    np.testing.assert_array_equal(np.concatenate([head.frames, tail.frames]), res.frames)
    np.testing.assert_array_equal(np.concatenate([head.weights, tail.weights]), res.weights)
    two = [np.stack([a, a], axis=1) for a in (ys, xs, zs, inten)]
    both = mt.trap_array_sequence(shape, *two, loops_first=12, loops=3, mask=mask, mask_flag=False, ct2pi=200)
    assert both.frames.shape == (4, 2) + shape and both.iters.shape == (4, 2) and both.stats.shape == (4, 2, 12, 4)
    np.testing.assert_array_equal(both.frames[:, 0], both.frames[:, 1])
    np.testing.assert_array_equal(both.weights[:, 1], res.weights)
    assert not np.array_equal(both.frames[:, 0], res.frames)  # mask_flag=False left the mask out
    mt.clear_spots()


@pytest.mark.gpu
def test_cli_writes_the_sequence(gpu, tmp_path, monkeypatch):
    from spatial_light_modulator_module_amd import generate_trap_sequence as gts
    from spatial_light_modulator_module_amd import move_traps as mt
    from spatial_light_modulator_module_amd.algorithms import hologram_from

    shape, m = (45, 70), 5
    traj = ssr.trajectory(45, 70, m, 9, 3)
    arr = np.stack([np.stack(li, axis=1) for li in traj])  # [F][M][4]
    os.makedirs(tmp_path / "images" / "moving_traps")
    np.save(tmp_path / "images" / "moving_traps" / "walk.npy", arr)
    monkeypatch.chdir(tmp_path)
    curves = gts.cli(["walk", "-v", "1", "-ct2pi", "256", "--shape", "45x70", "-first", "10", "-loops", "3", "-p"])
    want = mt.trap_array_sequence(shape, arr[:, :, 0], arr[:, :, 1], arr[:, :, 2], arr[:, :, 3], loops_first=10,
                                  loops=3, ct2pi=256, holograms=True)
    out = tmp_path / "holograms" / "walk_1_holograms"
    assert sorted(os.listdir(out)) == ["0.npy", "1.npy", "2.npy"]
    from PIL import Image

    for i in range(3):
        got = np.load(out / f"{i}.npy")
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, hologram_from(want.holograms[i]))
        png = np.array(Image.open(tmp_path / "images" / "moving_traps" / "walk_1_preview" / f"{i}.png"))
        np.testing.assert_array_equal(png, want.frames[i])
    assert [len(c) for c in curves] == [10, 3, 3]
    np.testing.assert_array_equal(curves[1], want.stats[1, :3, 1])
    mt.clear_spots()
