"""Float64 NumPy reference of a trap trajectory (the "trap trajectories" block
of include/slm_hip.h): the chain of frames written as calls to
spots_reference.spots_reference, including the tolerance stop, and the
trajectory its tests share. Test infrastructure only: the package has no CPU path."""
import numpy as np

import spots_reference as sr


def trajectory(h, w, m, seed, n_frames):
    """n_frames lists (ys, xs, zs, intensity): trap_list(h, w, m, seed) with
    every trap drifting at its own constant velocity (|v| <= 0.3 far-field
    pixels per frame on each axis), the defocus growing 5 % per frame, the
    intensities constant."""
    ys, xs, zs, inten = sr.trap_list(h, w, m, seed)
    rng = np.random.default_rng(7)
    vy = rng.uniform(-0.3, 0.3, m)
    vx = rng.uniform(-0.3, 0.3, m)
    return [(ys + f * vy, xs + f * vx, zs * (1 + 0.05 * f), inten) for f in range(n_frames)]


def frame_reference(shape, li, loops, tol, feedback, ain, phase, weights):
    """One frame: at most `loops` iterations on the list li from phase and
    weights (None = the default start / ones). With tol > 0 the first iteration
    whose incoming uniformity is <= tol is the last. Returns (phase, V, stats
    [iters][4], weights, iters)."""
    out = sr.spots_reference(shape, *li, loops=loops, feedback=feedback, ain=ain, initial_phase=phase,
                             initial_weights=weights)
    n = loops
    if tol > 0:
        hit = np.nonzero(out[2][:, 1] <= tol)[0]
        if hit.size and hit[0] + 1 < loops:
            n = int(hit[0]) + 1
            out = sr.spots_reference(shape, *li, loops=n, feedback=feedback, ain=ain, initial_phase=phase,
                                     initial_weights=weights)
    return out + (n,)


def sequence_reference(shape, lists, loops_first, loops, tol=0.0, feedback=1.0, ain=None, initial_phase=None,
                       initial_weights=None, resume=False):
    """The chain: frame 0 at most loops_first iterations from the given start
    (with resume it is an ordinary later frame and the start is the state a
    previous chain ended with), frame f > 0 at most `loops` from the phase and
    weights of frame f-1. Returns one (phase, V, stats, weights, iters) per frame."""
    phase, weights, frames = initial_phase, initial_weights, []
    for f, li in enumerate(lists):
        n = loops_first if f == 0 and not resume else loops
        fr = frame_reference(shape, li, n, tol, feedback, ain, phase, weights)
        frames.append(fr)
        phase, weights = fr[0], fr[3]
    return frames


def tol_margin(frames, tol):
    """The smallest distance of any uniformity value of the chain from tol."""
    return min(float(np.min(np.abs(fr[2][:, 1] - tol))) for fr in frames)
