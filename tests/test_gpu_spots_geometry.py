"""The trap-list kernels (slm_spots_*) at the geometries the other spot tests
never reach: more than one 32-column chunk per column split (the steady state
of spot_fields_kernel's pipelined K loop), a ragged last split after a full
one, a fold in spot_update_kernel that wraps, a second grid-stride pass of the
table and phase kernels, and the size edges (sides 2 and 4096, odd widths, trap
counts around the padding boundary). tests/spots_geometry.py predicts each
case's cut and tests/test_host_spots_geometry.py holds the table to what it is
there for; here every case first checks that prediction against Spots.info().

The reference is tests/spots_reference.py in float64. The inputs are
hologram-like: the float32 phase the reference holds after 10 iterations from
the default start (a random phase gives |V| ~ 1e-3 sum a, of which a gate
scaled by sum a says little); min |V_ref| >= 0.01 sum a is asserted.

Gates: the caps of tests/test_gpu_spots.py (fields 1e-6 sum a per trap, phase
1e-5 rms, weights 5e-6, intensities and statistics 1e-5) and, inside them, 10x
the largest deviation the MI355X showed when these tests were first run (the
figures stand next to the constants and in the docstrings)."""
import numpy as np
import pytest

import spots_geometry as sg
import spots_reference as sr
import spots_sequence_reference as ssr
from gsw_reference import incoming_gauss
from oracle import gs_gd_oracle as orc

PHASE_RMS_TOL = 1e-5
WEIGHT_TOL = 5e-6
FIELDS_TOL = 1e-6  # times sum(a), per trap
CAP = 1e-5         # of the 10x-measured loop gates
# 10x the largest deviation from the float64 reference the MI355X showed when
# these tests were first run; where 10x the figure is above its cap, the cap is the gate
FIELDS_GATE = 7.94e-8         # measured 7.933e-9 over the nine cases of 1024 pixels or more (2x4096, 33 traps, a_in)
FIELDS_GATE_TINY = 7.71e-7    # measured 7.703e-8 over 2x2 and 3x33 (99 pixels at most: a rounding weighs 1 / sum a)
SUPERPOSE_GATE = PHASE_RMS_TOL  # measured 1.340e-6 rms (4096x45, 1000 traps): 10x is above the cap
INTENSITY_RTOL = CAP            # measured 1.885e-6 (257x97, 1023 traps): 10x is above the cap
STATS_TOL = CAP                 # measured 1.185e-6 (257x97, 1023 traps): 10x is above the cap
V_FLOOR = 0.01  # min |V_ref| / sum a of a hologram-like field

WARM = 10
_WARM = {}


def _seed(case):
    return 100 + case[2]


def _warm(case, feedback=1.0, with_ain=False):
    """(trap list, a_in, float32 phase and weights after WARM reference
    iterations from the default start), computed once per case."""
    key = (case, feedback, with_ain)
    if key not in _WARM:
        h, w, m = case
        li = sr.trap_list(h, w, m, _seed(case))
        ain = incoming_gauss(h, w) if with_ain else None
        ph, _, _, wt = sr.spots_reference((h, w), *li, loops=WARM, feedback=feedback, ain=ain)
        _WARM[key] = (li, ain, ph.astype(np.float32), wt.astype(np.float32))
    return _WARM[key]


def _check_info(gpu, case, handle=None):
    """Spots.info() is what tests/spots_geometry.py predicts."""
    h, w, m = case
    g = sg.geometry(h, w, m)
    want = {"padded_traps": g.padded_traps, "partials": g.partials, "cols_per_partial": g.cols_per_partial}
    if handle is None:
        with gpu.Spots(1, h, w, m, False, 1) as sp:
            sp.set_traps(*sr.trap_list(h, w, m, _seed(case)))
            info = sp.info()
    else:
        info = handle.info()
    assert {k: info[k] for k in want} == want, f"{sg.case_id(case)}: the device cuts this shape differently"


# ---------------------------------------------------------------------------
# a. the two products alone, on every case
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(sg.CASES), ids=sg.case_id)
def test_fields_product(gpu, case):
    """Measured (MI355X) when first run, max |V - V_ref| / sum a over the traps,
    with a_in ones and set: 5.4e-10 .. 6.9e-10 on 1080 x 1920 with 5 and 100
    traps, 1.4e-9 .. 7.933e-9 on the seven other cases of 1024 pixels or more
    (relative to |V_ref| itself at most 1.3e-7), 4.3e-8 .. 7.703e-8 on 2 x 2 and
    3 x 33, where one float32 rounding weighs 1 / sum a. All far below the cap
    of 1e-6, so each group has its own 10x gate."""
    _check_info(gpu, case)
    h, w, m = case
    (ys, xs, zs, _), _, phase, _ = _warm(case)
    py, px = sr.tables(h, w, ys, xs, zs)
    for ain in (None, incoming_gauss(h, w)):
        want = sr.fields(phase, py, px, ain)
        sum_a = float(h * w) if ain is None else float(ain.astype(np.float64).sum())
        floor = float(np.min(np.abs(want))) / sum_a
        assert floor >= V_FLOOR, f"min |V_ref| = {floor:.3e} sum a: not a hologram-like field, pick another seed"
        got = gpu.spots_fields(phase, ys, xs, zs, ain)[0]
        dev = float(np.max(np.abs(got - want))) / sum_a
        rel = float(np.max(np.abs(got - want) / np.abs(want)))
        print(f"[spots geometry fields] {h}x{w} {m} traps, a_in {'set' if ain is not None else 'ones'}: "
              f"max |V - V_ref| / sum a = {dev:.3e} (min |V_ref| / sum a = {floor:.3e}, max relative {rel:.3e})")
        assert dev <= FIELDS_TOL
        assert dev <= (FIELDS_GATE if h * w >= 1024 else FIELDS_GATE_TINY)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(sg.CASES), ids=sg.case_id)
def test_superposition_product(gpu, case):
    """The coefficients are the reference's a_T w V / |V| of the same warm
    state. Measured (MI355X) when first run: phase rms 4.8e-8 .. 2.2e-7 with up
    to 33 traps, 4.5e-7 with 100, 8.8e-7 .. 1.340e-6 with 1000 and more (it
    grows with the trap count, the summed index). 10x the largest is above the
    1e-5 bar, so the bar is the gate."""
    _check_info(gpu, case)
    h, w, m = case
    (ys, xs, zs, inten), _, phase, wt = _warm(case)
    py, px = sr.tables(h, w, ys, xs, zs)
    v = sr.fields(phase, py, px)
    c = np.sqrt(inten) * wt.astype(np.float64) * v / np.abs(v)
    got = gpu.spots_superpose((h, w), c, ys, xs, zs)[0]
    rms = orc.phase_rms(got, sr.superpose(c, py, px))
    print(f"[spots geometry superpose] {h}x{w} {m} traps: phase rms {rms:.3e}")
    assert got.dtype == np.float32 and got.shape == (h, w)
    assert rms <= PHASE_RMS_TOL
    assert rms <= SUPERPOSE_GATE


# ---------------------------------------------------------------------------
# b. the loop from a warm start
# ---------------------------------------------------------------------------
def _run(gpu, shape, lists, loops, feedback=1.0, ain=None, phase=None, weights=None, case=None):
    """One run of a fresh handle, read twice: lists = [(ys, xs, zs, intensity)]
    per hologram; the second run starts from the same phase and weights."""
    h, w = shape
    cols = [np.stack([li[k] for li in lists]) for k in range(4)]
    with gpu.Spots(len(lists), h, w, cols[0].shape[1], ain is not None, loops) as sp:
        sp.set_traps(*cols)
        if case is not None:
            _check_info(gpu, case, sp)
        if ain is not None:
            sp.set_ain(ain)
        sp.set_feedback(feedback)
        sp.set_phase(phase)
        sp.set_weights(weights)
        sp.run(loops)
        first = sp.read()
        sp.run(loops)
        return first, sp.read()


LOOP = [
    # case, feedback, a_in
    ((1080, 1920, 5), 1.0, False),
    ((1080, 1920, 100), 0.5, False),
    ((512, 530, 1024), 1.0, True),
    ((2048, 71, 1024), 1.0, False),
    ((257, 97, 1023), 1.0, False),
]
MORE = 5


@pytest.mark.gpu
@pytest.mark.parametrize("case,feedback,with_ain", LOOP, ids=[sg.case_id(c[0]) for c in LOOP])
def test_loop_warm_start(gpu, case, feedback, with_ain):
    """10 reference iterations; the phase and the weights rounded to float32
    go to both sides, which run 5 further iterations (contracting for these
    five lists: a 1e-6 rms change of the start ends at or below 4.3e-7 rms in
    phase and 2.4e-7 in the weights, checked in float64). Measured (MI355X)
    when first run, over these five: phase rms 1.7e-7 .. 1.208e-6 of the 1e-5
    bar, max |dw| 3.3e-8 .. 8.701e-7 of 5e-6, per-trap intensities within
    8.6e-8 .. 1.885e-6 relative, the four statistics (efficiency relative, the
    others absolute) within 8.0e-8 .. 1.185e-6; the largest of each on 257 x 97
    with 1023 traps. 10x the last two is above their cap of 1e-5, so the cap is
    their gate."""
    h, w, m = case
    li, ain, ph0, w0 = _warm(case, feedback, with_ain)
    want = sr.spots_reference((h, w), *li, loops=MORE, feedback=feedback, ain=ain, initial_phase=ph0,
                              initial_weights=w0)
    got, again = _run(gpu, (h, w), [li], MORE, feedback, ain, ph0[None], w0[None], case)
    phase, v, stats, wt = got
    assert stats.shape == (1, MORE, 4)
    rms = orc.phase_rms(phase[0], want[0])
    dw = float(np.max(np.abs(wt[0].astype(np.float64) - want[3])))
    di = float(np.max(np.abs(np.abs(v[0]) ** 2 / np.abs(want[1]) ** 2 - 1)))
    ds = np.abs(stats[0] - want[2])
    ds[:, 0] /= want[2][:, 0]  # the efficiency relative, the others (uniformity, min r, max r ~ 1) absolute
    ds = float(ds.max())
    print(f"[spots geometry loop] {sg.case_id(case)} p={feedback} a_in {'set' if with_ain else 'ones'} +{MORE}: "
          f"phase rms {rms:.3e}, max |dw| {dw:.3e}, intensities max rel {di:.3e}, statistics max dev {ds:.3e}")
    assert rms <= PHASE_RMS_TOL
    assert dw <= WEIGHT_TOL
    assert di <= INTENSITY_RTOL
    assert ds <= STATS_TOL
    for a, b in zip(got, again):  # a second run on the same handle
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------
# c. bit-for-bit identities at a split geometry
# ---------------------------------------------------------------------------
SPLIT = [(2048, 71, 1024), (1080, 1920, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPLIT, ids=sg.case_id)
def test_batch_of_two_is_two_runs(gpu, case):
    """Hologram k of a batch of 2 equals the same list run alone, and a second
    run on the same handle equals the first; from a caller's phase, so that
    the batch of the panel passes spot_phase_kernel's grid twice."""
    h, w, m = case
    lists = [sr.trap_list(h, w, m, s) for s in (_seed(case), _seed(case) + 1)]
    rng = np.random.default_rng(3)
    ph = np.stack([_warm(case)[2], rng.uniform(-np.pi, np.pi, (h, w)).astype(np.float32)])
    w0 = rng.uniform(0.8, 1.2, (2, m)).astype(np.float32)
    both, again = _run(gpu, (h, w), lists, 3, 1.0, None, ph, w0)
    for a, b in zip(both, again):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(both[1][0], both[1][1])
    for k in range(2):
        one, _ = _run(gpu, (h, w), lists[k:k + 1], 3, 1.0, None, ph[k:k + 1], w0[k:k + 1], case)
        for a, b in zip(both, one):
            np.testing.assert_array_equal(a[k], b[0])
    # hologram 0 started warm: its fields are the reference's, so both holograms are right, not merely equal
    want = sr.spots_reference((h, w), *lists[0], loops=1, initial_phase=ph[0], initial_weights=w0[0])
    with gpu.Spots(2, h, w, m, False, 1) as sp:
        sp.set_traps(*[np.stack([li[k] for li in lists]) for k in range(4)])
        sp.set_phase(ph)
        sp.set_weights(w0)
        sp.run(1)
        v = sp.read()[1]
    dev = float(np.max(np.abs(v[0] - want[1]))) / (h * w)
    print(f"[spots geometry batch] {sg.case_id(case)}: hologram 0 of 2, max |V - V_ref| / sum a = {dev:.3e}")
    assert dev <= FIELDS_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPLIT, ids=sg.case_id)
def test_same_list_is_one_run(gpu, case):
    """3 frames of one list at 3, 2 and 2 iterations are one run of 7."""
    h, w, m = case
    li = sr.trap_list(h, w, m, _seed(case))
    cols = [np.stack([np.stack([li[k]])] * 3) for k in range(4)]  # [F][B][M]
    mask = np.random.default_rng(11).uniform(0, 2 * np.pi, (h, w))
    with gpu.Spots(1, h, w, m, False, 7) as sp:
        sp.set_traps(*li)
        _check_info(gpu, case, sp)
        sp.run(7)
        phase, v, stats, wt = sp.read()
        sp.sequence(*cols, loops_first=3, loops=2, tol=0.0, mask=mask, ct2pi=200, rule=gpu.QUANT_ASTYPE, frames=True,
                    phases=True)
        fr, ph, sv, ss, sw, it = sp.sequence_read(phases=True)
    assert fr.shape == (3, 1, h, w) and fr.dtype == np.uint8 and ss.shape == (3, 1, 3, 4)
    np.testing.assert_array_equal(it[:, 0], [3, 2, 2])
    np.testing.assert_array_equal(ph[2], phase)
    np.testing.assert_array_equal(sv[2], v)
    np.testing.assert_array_equal(sw[2], wt)
    np.testing.assert_array_equal(np.concatenate([ss[0], ss[1][:, :2], ss[2][:, :2]], axis=1), stats)
    assert np.all(ss[1:, :, 2:] == 0)
    np.testing.assert_array_equal(fr, gpu.quantize(ph.astype(np.float64), mask, 200, gpu.QUANT_ASTYPE))
    assert len(np.unique(fr)) > 100  # real levels, not a constant
    assert not np.array_equal(ph[0], ph[2])


STOP_CASE, STOP_TOL, STOP_ITERS = (2048, 71, 1024), 0.0265, [7, 5]
STOP_MARGIN = 1e-3  # 100x the cap of the statistics gate: rounding cannot move a stop


@pytest.mark.gpu
def test_tolerance_stop_at_a_split_geometry(gpu):
    """A moving list of 1024 traps on 2048 x 71, 10 iterations at most for the
    first frame and 6 for the second: tol lies between two uniformities of the
    reference chain, at least STOP_MARGIN from every one of them, so the device
    must stop every frame where the reference does."""
    h, w, m = STOP_CASE
    traj = ssr.trajectory(h, w, m, _seed(STOP_CASE), 2)
    ref = ssr.sequence_reference((h, w), traj, 10, 6, STOP_TOL)
    assert [f[4] for f in ref] == STOP_ITERS
    assert ssr.tol_margin(ref, STOP_TOL) >= STOP_MARGIN
    cols = [np.stack([li[k] for li in traj])[:, None] for k in range(4)]
    with gpu.Spots(1, h, w, m, False, 10) as sp:
        sp.sequence(*cols, loops_first=10, loops=6, tol=STOP_TOL, frames=False, phases=True)
        _check_info(gpu, STOP_CASE, sp)
        _, ph, v, stats, wt, iters = sp.sequence_read(frames=False, phases=True)
    print(f"[spots geometry stop] {sg.case_id(STOP_CASE)}: iterations per frame {iters[:, 0].tolist()}, "
          f"reference {STOP_ITERS}")
    np.testing.assert_array_equal(iters[:, 0], STOP_ITERS)
    assert stats.shape == (2, 1, 10, 4)
    for f, n in enumerate(STOP_ITERS):
        assert np.all(stats[f, 0, n:] == 0) and np.all(stats[f, 0, :n, 0] > 0)
        assert np.all(stats[f, 0, :n - 1, 1] > STOP_TOL)
        assert stats[f, 0, n - 1, 1] <= STOP_TOL or n == (10 if f == 0 else 6)
        du = float(np.max(np.abs(stats[f, 0, :n, 1] - ref[f][2][:, 1])))
        print(f"[spots geometry stop] frame {f}: uniformity {stats[f, 0, 0, 1]:.3e} -> {stats[f, 0, n - 1, 1]:.3e}, "
              f"max deviation from the reference {du:.3e}")
