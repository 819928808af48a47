"""Warm-start phase parity (SURVEY.md 8c protocol) at both arithmetic
precisions and at sizes beyond the committed goldens.

Protocol: start from the reference's phase after `warm` iterations and compare
with the reference's phase `span` iterations later (wrapped rms, bar 1e-5,
north_star). Goldens (256^2) come from the reference itself; larger sizes use
the faithful float64 restatement (oracle/gs_gd_oracle.py), pinned to those
goldens by tests/test_oracle_golden.py, run over several host threads
(pocketfft's per-line transforms are the same bits at any thread count).

Spans: 200 iterations up to 2048^2. At 4096^2 the protocol is chaotic enough
that complex64 state itself ends near the bar after 200 iterations (measured
1.06e-5 with float64 butterflies, 1.6e-5 with float32; 8.2e-7 / 3.1e-6 after
100), so 4096^2 is gated at 100 iterations (SURVEY.md 8c allows either; the
measurement lives in DESIGN.md section 5 and tools/precision_large.py).
"""
import os

import numpy as np
import pytest
import scipy.fft as sfft

from oracle import goldens
from oracle import gs_gd_oracle as orc

PHASE_RMS_TOL = 1e-5
WORKERS = min(16, os.cpu_count() or 1)  # the GPU box gives a process a 16-CPU share


def _gpu_warm_run(lib, t, phi_w, span, precision):
    """precision None: the plan's default (float32; float64 butterflies for uint8 targets)"""
    tt = lib.TGT_U8 if t.dtype == np.uint8 else lib.TGT_F32
    with lib.Plan(lib.ALGO_GS, 1, t.shape[0], t.shape[1], tt, False, span) as p:
        if precision is not None:
            p.set_precision(precision)
        p.set_target(t[None])
        p.set_phase(np.asarray(phi_w, np.float32)[None])
        p.run(span)
        ph, _, stats, _ = p.read(expected=False)
    return ph[0], stats[0, :span, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g1_gs_u8_256.npz", "g2_gs_f32_256.npz"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_reference_goldens_both_precisions(gpu, golden_dir, name, prec):
    g = goldens.load(os.path.join(golden_dir, name))
    precision = gpu.PRECISION_F32 if prec == "f32" else gpu.PRECISION_F64
    ph, err = _gpu_warm_run(gpu, g["target"], g["phi30"], 200, precision)
    rms = orc.phase_rms(ph, g["phi230"])
    print(f"[parity] {name} {prec} warm-start 30+200: phase rms {rms:.3e}")
    assert rms < PHASE_RMS_TOL
    np.testing.assert_allclose(err, g["err230"][30:], rtol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("n,span,u8,seed", [(1024, 200, True, 1024), (1024, 200, True, 1025), (1024, 200, True, 1026),
                                            (1024, 200, False, 1024), (1024, 200, False, 1234),
                                            (1024, 200, False, 1235), (2048, 100, False, 2048)])
def test_warm_start_parity_large(gpu, n, span, u8, seed):
    """(1024, 200, float32 target) is the bench headline itself (BASELINE.json
    configs[1]), gated on three targets: default_rng(1024) and the bench's own
    first two targets (bench.targets: default_rng(1234 + b), b = 0, 1). Its
    plan must be the one bench.py times -- narrow 1024 plan (key 11) on both
    axes, 2-column tiles, the narrow layout pair (8-wide X, 2-wide Y panels),
    i.e. col_kernel<11, 2, GS_MAIN, f32 target, f32, narrow> -- on the
    wave-shuffle transform pair (fft_shuffle.hpp) in both kernels, so the gate
    covers the exact instantiation the roofline is quoted on.

    uint8 targets (the CLI's input dtype, src/generate_hologram.py:102-110)
    on three targets: the plan's default there -- float64 butterflies since
    r06 -- is held to 8e-6 (float32 measured up to 7.7e-6 of the 1e-5 bar,
    profiles/r06/u8_margin.txt), float32 and float64 each to the bar."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (n, n)).astype(np.uint8) if u8 else rng.uniform(0, 255, (n, n)).astype(np.float32)
    with sfft.set_workers(WORKERS):
        phi_w, _, _ = orc.gerchberg_saxton_faithful(t, 30)
        ref, _, ref_err = orc.gerchberg_saxton_faithful(t, span, initial_phase=phi_w)
    if n == 1024 and not u8:
        with gpu.Plan(gpu.ALGO_GS, 1, n, n, gpu.TGT_F32, False, span) as p:
            info = p.info()
        assert (info["row_plan"], info["col_plan"], info["col_cw"], info["layout"], info["precision"],
                info["engine"]) == (11, 11, 2, (8, 2), "f32", ("shuffle", "shuffle")), info
    if u8:
        with gpu.Plan(gpu.ALGO_GS, 1, n, n, gpu.TGT_U8, False, span) as p:
            assert p.info()["precision"] == "f64", p.info()
    runs = [("f64", gpu.PRECISION_F64), ("f32", gpu.PRECISION_F32)] + ([("default", None)] if u8 else [])
    for prec, precision in runs:
        ph, err = _gpu_warm_run(gpu, t, phi_w, span, precision)
        rms = orc.phase_rms(ph, ref)
        print(f"[parity] {n}^2 {'u8' if u8 else 'f32'} target (seed {seed}), {prec}: warm-start 30+{span}: "
              f"phase rms {rms:.3e}")
        assert rms < (8e-6 if prec == "default" else PHASE_RMS_TOL)
        np.testing.assert_allclose(err, ref_err, rtol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1234, 1235])
def test_headline_on_the_float64_engine(gpu, monkeypatch, seed):
    """The headline configuration (GS 1024^2, +200 from the oracle's 30-iteration
    state, the bench's own targets) on $SLM_ENGINE=float64 -- complex128 state
    and float64 arithmetic, as the reference (the complex128 radix-plan kernels,
    radix_c128.hpp) -- lands ~30x inside the 1e-5
    bar that the float32 plans meet with ~2x margin (measured 3.9e-7 /
    3.1e-7: the iteration is chaotic, so even float64 rounding differences
    from pocketfft grow over 200 iterations)."""
    t = np.random.default_rng(seed).uniform(0, 255, (1024, 1024)).astype(np.float32)
    with sfft.set_workers(WORKERS):
        phi_w, _, _ = orc.gerchberg_saxton_faithful(t, 30)
        ref, _, ref_err = orc.gerchberg_saxton_faithful(t, 200, initial_phase=phi_w)
    monkeypatch.setenv("SLM_ENGINE", "float64")
    with gpu.Plan(gpu.ALGO_GS, 1, 1024, 1024, gpu.TGT_F32, False, 200) as p:
        assert p.engine() == ("radix-c128", "radix-c128"), p.engine()
    ph, err = _gpu_warm_run(gpu, t, phi_w, 200, gpu.PRECISION_F64)
    rms = orc.phase_rms(ph, ref)
    print(f"[parity] 1024^2 f32 target (seed {seed}), float64 engine: warm-start 30+200: phase rms {rms:.3e}")
    assert rms < 1e-6
    np.testing.assert_allclose(err, ref_err, rtol=1e-5)
