"""Weighted Gerchberg-Saxton without a device: the NumPy reference the GPU
tests compare against does what it is for (uniform trap intensities), and the
CLIs take the new algorithm without changing any default or file name."""
import argparse

import numpy as np
import pytest

from gsw_reference import gsw_reference, traps, uniformity


@pytest.mark.parametrize("h,w,nt,seed", [(128, 128, 16, 7), (256, 256, 40, 8)])
def test_reference_uniformity(h, w, nt, seed):
    t = traps(h, w, nt, seed, False)
    phi0 = np.random.default_rng(0).uniform(0, 2 * np.pi, (h, w))
    _, e_gs, _, g_gs = gsw_reference(t, 60, 0.0, initial_phase=phi0)
    _, e_w, _, g_w = gsw_reference(t, 60, 1.0, initial_phase=phi0)
    u_gs, u_w = uniformity(e_gs, t), uniformity(e_w, t)
    print(f"[gsw] reference {h}x{w} {nt} traps, 60 iterations: u GS {u_gs:.3e}, GSW {u_w:.3e}")
    assert np.all(g_gs == 1.0)  # feedback 0 leaves the weights alone: plain GS
    assert u_w <= 0.005 and u_w <= u_gs / 5
    assert abs(g_w[t > 0].mean() - 1) < 1e-12 and np.all(g_w[t == 0] == 1.0)


def test_hologram_cli_parser():
    from spatial_light_modulator_module_amd import generate_hologram as gh

    p = gh.build_parser()
    a = p.parse_args(["traps.png"])
    assert a.algorithm == "gerchberg_saxton" and a.feedback == 1.0
    a = p.parse_args(["traps.png", "-alg", "weighted_gerchberg_saxton", "--feedback", "0.5", "-l", "7"])
    assert a.algorithm == "weighted_gerchberg_saxton" and a.feedback == 0.5
    sep = " " * 8
    assert gh.make_hologram_name(a, "traps") == f"traps{sep}_weighted_gerchberg_saxton{sep}{sep}_loops7{sep}"
    # the names of the reference's two algorithms are what they were
    a = p.parse_args(["traps.png", "-l", "7"])
    assert gh.make_hologram_name(a, "traps") == f"traps{sep}_gerchberg_saxton{sep}{sep}_loops7{sep}"
    a = p.parse_args(["traps.png", "-alg", "gradient_descent", "-l", "7", "-q"])
    assert gh.make_hologram_name(a, "traps") == (f"traps_quarter{sep}_gradient_descent{sep}"
                                                 f"_lr0.005_mr1_unsettle0{sep}_loops7{sep}")
    with pytest.raises(SystemExit):
        p.parse_args(["traps.png", "-alg", "nonsense"])


def test_sequence_cli_parser():
    from spatial_light_modulator_module_amd import generate_hologram_sequence as ghs

    p = ghs.build_parser()
    a = p.parse_args(["walk", "-ct2pi", "255"])
    assert a.algorithm == "gerchberg_saxton" and a.feedback == 1.0 and a.max_loops == 5
    a = p.parse_args(["walk", "-ct2pi", "255", "-alg", "weighted_gerchberg_saxton", "--feedback", "0.75"])
    assert a.algorithm == "weighted_gerchberg_saxton" and a.feedback == 0.75
    with pytest.raises(SystemExit):
        p.parse_args(["walk", "-ct2pi", "255", "-alg", "gradient_descent"])


def test_weighted_gs_refuses_shapes_off_the_fused_engine(monkeypatch):
    """The shape check comes before any device call."""
    from spatial_light_modulator_module_amd import algorithms as alg

    ns = argparse.Namespace(incomming_intensity="uniform", tolerance=0.0, max_loops=5, gif=False, print_info=False,
                            plot_error=False)
    for shape in ((1080, 1920), (97, 101)):
        with pytest.raises(ValueError, match="64, 128, 256, 512, 1024, 2048, 4096.*768"):
            alg.weighted_gerchberg_saxton(np.zeros(shape, np.uint8), ns)
    monkeypatch.setenv("SLM_ENGINE", "float64")
    with pytest.raises(ValueError, match="SLM_ENGINE=float64"):
        alg.run_gsw(np.zeros((1, 64, 64), np.uint8), 5)
