"""Image sequences (slm_plan_sequence): the device-resident chain equals, bit
for bit, the host loop callers write with the existing API --

    for f: set_target(targets[f]) (MRAF: set_region(regions[f]));
           f > 0: set_phase(phase of frame f - 1);
           run(loops_first if f == 0 else loops, tol, checked = tol > 0); read();
           frame = quantize(float64(phase), mask, ct2pi, rule)

-- on every engine GS, weighted GS and MRAF run on, with resume, the tolerance
stop, grown buffers, the plan's state afterwards, the refusals, and the Python
surface (algorithms.run_sequence, generate_hologram_sequence --chain)."""
import numpy as np
import pytest
from PIL import Image

import plan_sequence_cases as cases
from spatial_light_modulator_module_amd import _lib
from spatial_light_modulator_module_amd import algorithms as alg
from spatial_light_modulator_module_amd._lib import ALGO_GD, ALGO_GS, ALGO_GSW, ALGO_MRAF, QUANT_ASTYPE, QUANT_PIL

pytestmark = pytest.mark.gpu

eq = np.testing.assert_array_equal


def as_batches(t):
    return t[:, None] if t.ndim == 3 else t


def new_plan(algo, targets, max_loops, ain=None, setup=None):
    _, b, h, w = targets.shape
    tt = _lib.TGT_U8 if targets.dtype == np.uint8 else _lib.TGT_F32
    plan = _lib.Plan(algo, b, h, w, tt, ain is not None, max_loops)
    if ain is not None:
        plan.set_ain(ain)
    if setup:
        setup(plan)
    return plan


def host_loop(plan, targets, regions=None, loops_first=6, loops=3, tol=0.0, quant=((None, 256.0, QUANT_PIL),),
              prev=None):
    """The definition: one dict per frame. `quant`: the (mask, ct2pi, rule)
    variants the frames are wanted for. prev: continue from that phase (every
    frame is then a frame f > 0)."""
    out = []
    for f in range(len(targets)):
        plan.set_target(targets[f])
        if regions is not None:
            plan.set_region(regions[f])
        if prev is not None:
            plan.set_phase(prev)
        n = loops_first if prev is None else loops
        plan.run(n, tol, tol > 0)
        phase, e, stats, iters = plan.read()
        eff = plan.read_efficiency() if plan.algo == ALGO_MRAF else None
        out.append({"phase": phase, "e": e, "stats": stats, "iters": iters, "eff": eff, "loops": n,
                    "frames": [_lib.quantize(phase.astype(np.float64), m, c, r) for m, c, r in quant]})
        prev = phase
    return out


def chain(plan, targets, regions=None, loops_first=6, loops=3, tol=0.0, quant=(None, 256.0, QUANT_PIL),
          resume=False):
    mask, ct2pi, rule = quant
    plan.sequence(targets, regions, loops_first=loops_first, loops=loops, tol=tol, resume=resume, mask=mask,
                  ct2pi=ct2pi, rule=rule, frames=True, phases=True, expected=True)
    mraf = plan.algo == ALGO_MRAF
    frames, phases, e, stats, eff, iters = plan.sequence_read(frames=True, phases=True, expected=True, stats=True,
                                                              efficiency=mraf, iters=True)
    return {"frames": frames, "phases": phases, "e": e, "stats": stats, "eff": eff, "iters": iters}


def executed(iters, loops):
    return [loops if k < 0 else int(k) for k in iters]


def assert_chain_is_host_loop(got, want, variant=0):
    assert len(got["phases"]) == len(want)
    for f, w in enumerate(want):
        eq(got["phases"][f], w["phase"], err_msg=f"phase of frame {f}")
        eq(got["e"][f], w["e"], err_msg=f"E of frame {f}")
        eq(got["iters"][f], w["iters"], err_msg=f"iters of frame {f}")
        eq(got["frames"][f], w["frames"][variant], err_msg=f"uint8 frame {f}")
        for b, n in enumerate(executed(w["iters"], w["loops"])):  # the rows the run wrote
            eq(got["stats"][f, b, :n], w["stats"][b, :n], err_msg=f"statistics of frame {f}, hologram {b}")
            if w["eff"] is not None:
                eq(got["eff"][f, b, :n], w["eff"][b, :n], err_msg=f"efficiency of frame {f}, hologram {b}")


def assert_same_sequence(a, b, loops_of):
    for key in ("frames", "phases", "e", "iters"):
        eq(a[key], b[key], err_msg=key)
    for f in range(len(a["phases"])):
        for h, n in enumerate(executed(a["iters"][f], loops_of(f))):
            eq(a["stats"][f, h, :n], b["stats"][f, h, :n])
            if a["eff"] is not None:
                eq(a["eff"][f, h, :n], b["eff"][f, h, :n])


def check_case(algo, targets, regions=None, ain=None, setup=None, loops_first=6, loops=3, tol=0.0):
    targets = as_batches(targets)
    regions = None if regions is None else as_batches(regions)
    max_loops = max(loops_first, loops)
    with new_plan(algo, targets, max_loops, ain, setup) as plan:
        want = host_loop(plan, targets, regions, loops_first, loops, tol)
    with new_plan(algo, targets, max_loops, ain, setup) as plan:
        got = chain(plan, targets, regions, loops_first, loops, tol)
    assert_chain_is_host_loop(got, want)
    return got, want


# ---- 1. the chain equals the host loop ------------------------------------------------------------------
def test_gs_u8_64_every_quantisation(gpu):
    t = as_batches(cases.trap_grid(4, 64, 64))
    mask = np.random.default_rng(3).uniform(0, 2 * np.pi, (64, 64))
    variants = [(m, c, r) for r in (QUANT_PIL, QUANT_ASTYPE) for m in (None, mask) for c in (256.0, 255.0)]
    with new_plan(ALGO_GS, t, 6) as plan:
        want = host_loop(plan, t, quant=variants)
    for k, v in enumerate(variants):
        with new_plan(ALGO_GS, t, 6) as plan:
            got = chain(plan, t, quant=v)
        assert_chain_is_host_loop(got, want, k)
        assert len(np.unique(got["frames"])) > 100
    assert np.any(got["phases"][0] != got["phases"][3])


def test_gs_f32_64x768(gpu):
    got, _ = check_case(ALGO_GS, cases.trap_grid(4, 64, 768, np.float32))
    assert np.any(got["phases"][0] != got["phases"][3])


def test_gs_u8_128x256_ain_batch2(gpu):
    t = cases.batch_of_two(cases.trap_grid(4, 128, 256))
    got, _ = check_case(ALGO_GS, t, ain=cases.gaussian_ain(128, 256))
    assert np.any(got["phases"][:, 0] != got["phases"][:, 1])


def test_weighted_gs_u8_64(gpu):
    check_case(ALGO_GSW, cases.trap_grid(4, 64, 64), setup=lambda p: p.set_feedback(1.0))


def test_mraf_u8_128x256_regions_per_frame(gpu):
    t, r = cases.mraf_frames(4, 128, 256)
    got, _ = check_case(ALGO_MRAF, t, r, setup=lambda p: p.set_mixing(0.4))
    assert np.all(got["eff"][:, :, :3] > 0)


def test_mraf_64_region_in_force(gpu):
    t, r = cases.mraf_frames(4, 64, 64)
    t = as_batches(t)

    def setup(p):
        p.set_mixing(0.4)
        p.set_region(r[:1])

    with new_plan(ALGO_MRAF, t, 6, setup=setup) as plan:
        want = host_loop(plan, t)
    with new_plan(ALGO_MRAF, t, 6, setup=setup) as plan:
        got = chain(plan, t, None)
    assert_chain_is_host_loop(got, want)


# ---- 2. the any-size back ends ----------------------------------------------------------------------------
@pytest.mark.parametrize("h, w, dtype, forced, engines", [
    (97, 101, np.uint8, False, ("bluestein",)),
    (60, 100, np.uint8, False, ("mixed-radix", "radix-c128")),
    (64, 64, np.uint8, True, ("radix-c128",)),
    (600, 800, np.float32, False, ("radix-c64",)),
])
def test_any_size_back_ends(gpu, monkeypatch, h, w, dtype, forced, engines):
    if forced:
        monkeypatch.setenv("SLM_ENGINE", "float64")
    t = as_batches(cases.trap_grid(3, h, w, dtype))
    with new_plan(ALGO_GS, t, 4) as plan:
        assert plan.generic_info()["engine"] in engines
        want = host_loop(plan, t, loops_first=4, loops=2)
    with new_plan(ALGO_GS, t, 4) as plan:
        got = chain(plan, t, loops_first=4, loops=2)
    assert_chain_is_host_loop(got, want)


# ---- 3. frame 0 starts -------------------------------------------------------------------------------------
def test_frame0_starts(gpu):
    t = as_batches(cases.trap_grid(2, 64, 64))
    phi = np.random.default_rng(4).uniform(-np.pi, np.pi, (1, 64, 64)).astype(np.float32)
    with new_plan(ALGO_GS, t, 6) as plan:  # the caller's start
        plan.set_target(t[0])
        plan.set_phase(phi)
        plan.run(6)
        warm = plan.read()[0]
        plan.set_phase(None)
        plan.run(6)
        cold = plan.read()[0]
    assert np.any(warm != cold)
    with new_plan(ALGO_GS, t, 6, setup=lambda p: p.set_phase(phi)) as plan:
        eq(chain(plan, t)["phases"][0], warm)
    with new_plan(ALGO_GS, t, 6) as plan:
        eq(chain(plan, t)["phases"][0], cold)


# ---- 4. resume ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [ALGO_GS, ALGO_MRAF])
def test_resume_is_the_uncut_sequence(gpu, algo):
    if algo == ALGO_MRAF:
        t, r = cases.mraf_frames(6, 64, 64)
        t, r = as_batches(t), as_batches(r)
    else:
        t, r = as_batches(cases.trap_grid(6, 64, 64)), None
    with new_plan(algo, t, 6) as plan:
        whole = chain(plan, t, r)
    with new_plan(algo, t, 6) as plan:
        a = chain(plan, t[:2], None if r is None else r[:2])
        b = chain(plan, t[2:], None if r is None else r[2:], resume=True)
    cut = {k: (None if a[k] is None else np.concatenate([a[k], b[k]])) for k in a}
    assert_same_sequence(cut, whole, lambda f: 6 if f == 0 else 3)


# ---- 5. the tolerance stop --------------------------------------------------------------------------------
def test_tolerance_stop(gpu):
    t, tol, n = cases.tolerance_targets(), cases.tolerance(), cases.TOL_LOOPS
    got, want = check_case(ALGO_GS, t, loops_first=n, loops=n, tol=tol)
    ran = np.array([executed(w["iters"], n) for w in want])
    print(f"[tolerance] tol {tol:.4f}: iterations per (frame, hologram) {ran.tolist()}")
    assert np.any(ran < n), "no (frame, hologram) stopped early"
    assert np.any(got["iters"] < 0), "no (frame, hologram) ran its full count"


# ---- 6. grown buffers --------------------------------------------------------------------------------------
def test_grown_buffers(gpu):
    t = as_batches(cases.trap_grid(5, 64, 64))
    with new_plan(ALGO_GS, t, 6) as plan:
        plan.sequence(t[:2], loops_first=6, loops=3)
        plan.sequence_read()
        grown = chain(plan, t)
    with new_plan(ALGO_GS, t, 6) as plan:
        fresh = chain(plan, t)
    assert_same_sequence(grown, fresh, lambda f: 6 if f == 0 else 3)


# ---- 7. the plan after a sequence -------------------------------------------------------------------------
def test_state_after_a_sequence(gpu):
    t = as_batches(cases.trap_grid(3, 64, 64))
    phi = np.random.default_rng(6).uniform(-np.pi, np.pi, (1, 64, 64)).astype(np.float32)
    with new_plan(ALGO_GS, t, 6, setup=lambda p: p.set_phase(phi)) as plan:
        plan.sequence(t, loops_first=6, loops=3)
        with pytest.raises(_lib.SlmError) as err:
            plan.read()
        assert err.value.code == _lib.ERR_STATE
        plan.run(5)
        after = plan.read()
    with new_plan(ALGO_GS, t, 6, setup=lambda p: p.set_phase(phi)) as plan:
        plan.set_target(t[-1])
        plan.run(5)
        fresh = plan.read()
    eq(after[0], fresh[0])
    eq(after[1], fresh[1])
    eq(after[2][:, :5], fresh[2][:, :5])
    eq(after[3], fresh[3])


# ---- 8. refusals -------------------------------------------------------------------------------------------
def raw_sequence(plan, targets, regions=None, n_frames=None, loops_first=3, loops=3, tol=0.0, resume=0, ct2pi=256.0,
                 rule=QUANT_PIL, want=(1, 0, 0)):
    """slm_plan_sequence itself: (return code, message)."""
    t = np.ascontiguousarray(targets)
    r = None if regions is None else np.ascontiguousarray(regions, dtype=np.uint8)
    rc = plan._lib.slm_plan_sequence(plan.handle, len(t) if n_frames is None else n_frames, _lib.ptr(t), _lib.ptr(r),
                                     loops_first, loops, float(tol), resume, None, float(ct2pi), rule, *want)
    if rc == 0:
        plan._seq = (len(t), max(loops_first, loops))  # what Plan.sequence_read sizes its arrays by
    return rc, _lib.last_error()


def test_refusals_of_arguments(gpu):
    t = as_batches(cases.trap_grid(3, 64, 64))
    with new_plan(ALGO_GS, t, 4) as plan:
        for bad in ({"n_frames": 0}, {"n_frames": -1}, {"loops": 0}, {"loops": 5}, {"loops_first": 0},
                    {"loops_first": 5}, {"tol": -1.0}, {"tol": float("nan")}, {"tol": float("inf")}, {"rule": 2},
                    {"rule": -1}, {"ct2pi": 0.0}, {"ct2pi": -256.0}, {"ct2pi": float("nan")},
                    {"ct2pi": float("inf")}):
            rc, msg = raw_sequence(plan, t, **bad)
            assert rc == _lib.ERR_ARG, (bad, rc, msg)
        assert raw_sequence(plan, t)[0] == 0  # the plan is still usable
        plan.sequence_read()


def test_refusal_of_an_mraf_frame_without_support(gpu):
    t, r = cases.mraf_frames(4, 64, 64)
    t, r = cases.batch_of_two(t), cases.batch_of_two(r)
    r[2, 1] = 0
    r[2, 1, 63, 63] = 1  # a region, but no target light in it
    assert t[2, 1, 63, 63] == 0
    with new_plan(ALGO_MRAF, t, 4) as plan:
        rc, msg = raw_sequence(plan, t, r)
        assert rc == _lib.ERR_ARG and "frame 2" in msg and "hologram 1" in msg, (rc, msg)
        r[2, 1] = r[1, 1]
        assert raw_sequence(plan, t, r)[0] == 0


def test_refusals_of_state(gpu):
    t = as_batches(cases.trap_grid(3, 64, 64))
    state = _lib.ERR_STATE
    with new_plan(ALGO_GD, t, 4) as plan:
        assert raw_sequence(plan, t)[0] == state
    with _lib.Plan(ALGO_GS, 1, 64, 64, _lib.TGT_U8, True, 4) as plan:  # has_ain, no set_ain
        assert raw_sequence(plan, t)[0] == state
        plan.set_ain(cases.gaussian_ain(64, 64))
        assert raw_sequence(plan, t)[0] == 0
    with new_plan(ALGO_GS, t, 4) as plan:
        assert raw_sequence(plan, t, regions=np.ones_like(t))[0] == state  # regions belong to MRAF
        with pytest.raises(_lib.SlmError) as err:  # nothing to read yet
            plan.sequence_read()
        assert err.value.code == state
        assert raw_sequence(plan, t, resume=1)[0] == state  # nothing to resume
        assert raw_sequence(plan, t)[0] == 0
        assert raw_sequence(plan, t, resume=1)[0] == 0
        for touch in (lambda: plan.set_target(t[0]), lambda: plan.set_phase(None), lambda: plan.run(2),
                      lambda: plan.set_precision(plan.precision)):
            assert raw_sequence(plan, t)[0] == 0
            touch()
            rc, msg = raw_sequence(plan, t, resume=1)
            assert rc == state, msg
        assert raw_sequence(plan, t)[0] == 0  # frames kept; phases and E not
        for ask in ({"frames": False, "phases": True}, {"frames": False, "expected": True},
                    {"frames": False, "efficiency": True}):
            with pytest.raises(_lib.SlmError) as err:
                plan.sequence_read(**ask)
            assert err.value.code == state, ask
        assert raw_sequence(plan, t, want=(0, 1, 0))[0] == 0
        with pytest.raises(_lib.SlmError) as err:
            plan.sequence_read(frames=True)
        assert err.value.code == state
    tm, rm = cases.mraf_frames(3, 64, 64)
    with new_plan(ALGO_MRAF, as_batches(tm), 4) as plan:
        assert raw_sequence(plan, as_batches(tm))[0] == state  # neither regions nor a region in force
        assert raw_sequence(plan, as_batches(tm), as_batches(rm))[0] == 0
        for touch in (lambda: plan.set_mixing(0.5), lambda: plan.set_region(rm[:1])):
            touch()
            assert raw_sequence(plan, as_batches(tm), as_batches(rm), resume=1)[0] == state
            assert raw_sequence(plan, as_batches(tm), as_batches(rm))[0] == 0
        assert raw_sequence(plan, as_batches(tm))[0] == 0  # the last frame's region is now in force
    with new_plan(ALGO_GSW, t, 4) as plan:
        assert raw_sequence(plan, t)[0] == 0
        plan.set_feedback(0.5)
        assert raw_sequence(plan, t, resume=1)[0] == state


# ---- 9. the Python surface -------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm, algo", [("gerchberg_saxton", ALGO_GS), ("weighted_gerchberg_saxton", ALGO_GSW),
                                             ("mraf", ALGO_MRAF)])
def test_run_sequence_is_the_call_it_wraps(gpu, algorithm, algo):
    if algo == ALGO_MRAF:
        t, r = cases.mraf_frames(3, 64, 64)
    else:
        t, r = cases.trap_grid(3, 64, 64), None
    mask = np.random.default_rng(8).uniform(0, 2 * np.pi, (64, 64))
    phases, frames, errs, norm, emax, e = alg.run_sequence(t, 5, 2, algorithm, feedback=0.7, mixing=0.3, regions=r,
                                                           mask=mask, ct2pi=255, rule=QUANT_ASTYPE,
                                                           return_expected=True)
    alg.clear_plans()

    def setup(p):
        if algo == ALGO_GSW:
            p.set_feedback(0.7)
        if algo == ALGO_MRAF:
            p.set_mixing(0.3)

    with new_plan(algo, as_batches(t), 5, setup=setup) as plan:
        want = chain(plan, as_batches(t), None if r is None else as_batches(r), loops_first=5, loops=2,
                     quant=(mask, 255.0, QUANT_ASTYPE))
    assert phases.shape == (3, 1, 64, 64) and frames.dtype == np.uint8
    eq(phases, want["phases"])
    eq(frames, want["frames"])
    eq(e, want["e"])
    for f in range(3):
        n = 5 if f == 0 else 2
        assert errs[f][0] == list(want["stats"][f, 0, :n, 3])
        assert emax[f, 0] == want["stats"][f, 0, n - 1, 0]
    sup = as_batches(t) if r is None else np.where(as_batches(r) != 0, as_batches(t), 0)
    eq(norm, sup.reshape(3, 1, -1).max(axis=2))


def test_cli_chain(gpu, tmp_path, monkeypatch):
    from spatial_light_modulator_module_amd import generate_hologram_sequence as ghs

    monkeypatch.chdir(tmp_path)
    d = tmp_path / "images" / "moving_traps" / "walk"
    d.mkdir(parents=True)
    t = cases.trap_grid(5, 96, 128)
    for i, f in enumerate(t):
        Image.fromarray(f).save(d / f"{i}.png")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SLM_GPUS"):
        monkeypatch.delenv(k, raising=False)
    errors = ghs.cli(["walk", "-v", "c", "-ct2pi", "255", "-loops", "4", "--chain"], plot=False)
    plain = ghs.cli(["walk", "-v", "p", "-ct2pi", "255", "-loops", "4"], plot=False)
    assert sorted(errors) == sorted(plain) == [0, 1, 2, 3, 4]
    phases, _, errs, _, _ = alg.run_sequence(t, 4, 4)
    for i in range(5):
        chained = np.load(tmp_path / "holograms" / "walk_c_holograms" / f"{i}.npy")
        eq(chained, alg.hologram_from(phases[i, 0]))
        assert chained.dtype == np.float64 and errors[i] == errs[i][0]
        cold = np.load(tmp_path / "holograms" / "walk_p_holograms" / f"{i}.npy")
        assert np.array_equal(chained, cold) == (i == 0), i
