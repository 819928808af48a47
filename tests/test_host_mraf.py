"""MRAF without a device: the NumPy reference the GPU tests compare against
is GS at m = 1 on a full region, smooths a drawn shape and contracts from a
warm start; the default signal region, the CLI flags and the refusals that
come before any device call."""
import argparse

import numpy as np
import pytest

from gsw_reference import uniformity
from mraf_reference import mraf_reference, shapes, start_phase
from oracle import gs_gd_oracle as orc


def test_reference_is_gs_at_full_mixing_on_a_full_region():
    """m = 1 with R all ones against the pinned GS oracle, both on the same
    float64 a_T = sqrt(T), 10 iterations from the shared start phase."""
    t = shapes(64, 64)[0].astype(np.float64)
    ph0 = start_phase(t.shape)
    ph_o, e_o, err_o = orc.gerchberg_saxton_faithful(t, 10, initial_phase=ph0)
    ph, e, err, eff = mraf_reference(t, np.ones(t.shape, np.uint8), 10, 1.0, initial_phase=ph0, a_t=np.sqrt(t))
    rms = orc.phase_rms(ph, ph_o)
    print(f"[mraf] reference at m = 1 against the GS oracle: phase rms {rms:.3e}")
    assert rms <= 1e-10  # float64 rounding, amplified by ten iterations from a random phase
    np.testing.assert_allclose(err, err_o, rtol=1e-10)
    np.testing.assert_allclose(e * (t.max() / e.max()), e_o, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(eff, 1.0, rtol=1e-12)  # the full region holds all the light (Parseval)


@pytest.mark.parametrize("h,w", [(64, 64), (128, 256)])
def test_reference_smoothness_and_contraction(h, w):
    t, r = shapes(h, w)
    ph0 = start_phase(t.shape)
    _, e_gs, _, _ = mraf_reference(t, np.ones_like(r), 60, 1.0, initial_phase=ph0)
    _, e_m, _, eff = mraf_reference(t, r, 60, 0.4, initial_phase=ph0)
    u_gs, u_m = uniformity(e_gs, t), uniformity(e_m, t)
    print(f"[mraf] reference {h}x{w}, 60 iterations: u GS {u_gs:.3e}, MRAF {u_m:.3e}, efficiency {eff[-1]:.4f}")
    assert u_gs >= 0.1
    assert u_m <= 0.01
    assert 0.40 <= eff[-1] <= 0.48
    # a 1e-7 perturbation of the 10-iteration warm start does not grow over 20 iterations
    warm = mraf_reference(t, r, 10, 0.4, initial_phase=ph0)[0]
    kick = 1e-7 * np.random.default_rng(6).standard_normal(t.shape)
    kick *= 1e-7 / np.sqrt(np.mean(kick ** 2))
    a = mraf_reference(t, r, 20, 0.4, initial_phase=warm)[0]
    b = mraf_reference(t, r, 20, 0.4, initial_phase=warm + kick)[0]
    grown = orc.phase_rms(a, b)
    print(f"[mraf] reference {h}x{w}: a 1e-7 rms kick of the warm start is {grown:.3e} after 20 iterations")
    assert grown <= 1e-7


def test_signal_region_dilates_without_wrapping():
    from spatial_light_modulator_module_amd import algorithms as alg

    t = np.zeros((8, 8), np.uint8)
    t[0, 0] = 1   # a corner: the square is clipped, nothing appears at the far edges
    t[4, 5] = 9
    want1 = np.zeros((8, 8), np.uint8)
    want1[0:2, 0:2] = 1
    want1[3:6, 4:7] = 1
    np.testing.assert_array_equal(alg.signal_region(t, 1), want1)
    np.testing.assert_array_equal(alg.signal_region(t, 0), (t > 0).astype(np.uint8))
    want2 = np.zeros((8, 8), np.uint8)
    want2[0:3, 0:3] = 1
    want2[2:7, 3:8] = 1
    got = alg.signal_region(t, 2)
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, want2)
    assert alg.signal_region(t, 50).all()  # a margin beyond the image
    assert not alg.signal_region(np.zeros((8, 8)), 3).any()
    np.testing.assert_array_equal(alg.signal_region(np.stack([t, t]), 1), np.stack([want1, want1]))  # batches
    with pytest.raises(ValueError):
        alg.signal_region(t, -1)


def test_hologram_cli_parser():
    from spatial_light_modulator_module_amd import generate_hologram as gh

    p = gh.build_parser()
    a = p.parse_args(["disc.png"])
    assert a.algorithm == "gerchberg_saxton" and a.mixing == 0.4 and a.region is None and a.region_margin == 8
    a = p.parse_args(["disc.png", "-alg", "mraf", "--mixing", "0.6", "--region", "disc_region.png",
                      "--region_margin", "3", "-l", "7"])
    assert a.algorithm == "mraf" and a.mixing == 0.6 and a.region == "disc_region.png" and a.region_margin == 3
    sep = " " * 8
    assert gh.make_hologram_name(a, "disc") == f"disc{sep}_mraf{sep}{sep}_loops7{sep}"
    a = p.parse_args(["disc.png", "-l", "7"])  # the drop-in's name is what it was
    assert gh.make_hologram_name(a, "disc") == f"disc{sep}_gerchberg_saxton{sep}{sep}_loops7{sep}"
    with pytest.raises(SystemExit):
        p.parse_args(["disc.png", "-alg", "mraf", "--mixing", "half"])


def _namespace(**kw):
    ns = argparse.Namespace(incomming_intensity="uniform", tolerance=0.0, max_loops=5, gif=False, print_info=False,
                            plot_error=False)
    vars(ns).update(kw)
    return ns


def test_mraf_refusals_come_before_any_device_call(monkeypatch):
    from spatial_light_modulator_module_amd import _lib
    from spatial_light_modulator_module_amd import algorithms as alg

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(_lib, "Plan", no_device)
    monkeypatch.setattr(alg, "get_plan", no_device)
    t, r = shapes(64, 64)
    for shape in ((1080, 1920), (97, 101)):
        big = np.zeros(shape, np.uint8)
        big[5:9, 5:9] = 200
        with pytest.raises(ValueError, match="64, 128, 256, 512, 1024, 2048, 4096.*768"):
            alg.mraf(big, _namespace())
        with pytest.raises(ValueError, match="fused engine only"):
            alg.run_mraf(big[None], np.ones_like(big)[None], 5)
    for m in (0.0, -0.1, 1.0001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="mixing"):
            alg.run_mraf(t[None], r[None], 5, mixing=m)
        with pytest.raises(ValueError, match="mixing"):
            alg.mraf(t, _namespace(mixing=m))
    with pytest.raises(ValueError, match="do not match"):
        alg.run_mraf(t[None], r[None, :32], 5)
    with pytest.raises(ValueError, match="does not match"):
        alg.mraf(t, _namespace(signal_region=r[:, :32]))
    empty = np.zeros_like(r)
    away = np.zeros_like(r)
    away[50:60, 50:60] = 1  # a region that misses the pattern
    for bad in (empty, away):
        with pytest.raises(ValueError, match="hologram 0 holds no pixel with T > 0"):
            alg.run_mraf(t[None], bad[None], 5)
    with pytest.raises(ValueError, match="hologram 1 holds no pixel"):
        alg.run_mraf(np.stack([t, t]), np.stack([r, away]), 5)
    monkeypatch.setenv("SLM_ENGINE", "float64")
    with pytest.raises(ValueError, match="SLM_ENGINE=float64"):
        alg.run_mraf(t[None], r[None], 5)
