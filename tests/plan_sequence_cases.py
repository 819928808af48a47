"""Targets the image-sequence tests share (slm_plan_sequence): a grid of
single-pixel traps that moves one pixel per frame, drawn MRAF shapes that
drift with their region, and the tolerance of the stop test with its float64
oracle chain. Test infrastructure only: the package has no CPU path."""
import functools

import numpy as np

from mraf_reference import shapes
from oracle import gs_gd_oracle as orc

GRID = (3, 4)  # traps per column, per row


def grid_positions(h, w, f):
    """(ys, xs) of the 3 x 4 traps in frame f: the grid moves one pixel to the
    right per frame."""
    ys = [h // 8 + i * (h // 5) for i in range(GRID[0])]
    xs = [w // 10 + j * (w // 6) + f for j in range(GRID[1])]
    return ys, xs


def max_frames(h, w):
    """Frames for which every trap stays inside the image."""
    return w - grid_positions(h, w, 0)[1][-1]


def trap_grid(n_frames, h, w, dtype=np.uint8):
    """[n_frames][h][w]: single-pixel traps of 255 on the moving grid."""
    assert n_frames <= max_frames(h, w)
    out = np.zeros((n_frames, h, w), np.uint8)
    for f in range(n_frames):
        ys, xs = grid_positions(h, w, f)
        out[f][np.ix_(ys, xs)] = 255
    return out.astype(dtype)


def batch_of_two(frames):
    """[F][2][h][w]: hologram 1 is the same sequence rolled by (5, 9)."""
    return np.stack([frames, np.roll(frames, (5, 9), axis=(1, 2))], axis=1)


def mraf_frames(n_frames, h, w):
    """(targets, regions), both uint8 [n_frames][h][w]: mraf_reference.shapes
    rolled by (f, 2 f) in frame f, the region with the target."""
    t, r = shapes(h, w)
    return (np.stack([np.roll(t, (f, 2 * f), axis=(0, 1)) for f in range(n_frames)]),
            np.stack([np.roll(r, (f, 2 * f), axis=(0, 1)) for f in range(n_frames)]))


def gaussian_ain(h, w):
    y, x = np.mgrid[:h, :w]
    return np.exp(-(((y - h / 2) / (0.45 * h)) ** 2 + ((x - w / 2) / (0.45 * w)) ** 2)).astype(np.float32)


# ---- the tolerance-stop case: GS uint8 128 x 256, batch 2, F = 5, loops 8 / 8 ----
TOL_SHAPE = (128, 256)
TOL_FRAMES = 5
TOL_LOOPS = 8
TOL_PAIR = 3  # tol lies between errors 3 and 4 of frame 0, hologram 0


def tolerance_targets():
    """[F][2][h][w]: hologram 0 the trap grid, whose error falls through the
    tolerance within a few iterations of every frame; hologram 1 the drifting
    shapes as plain GS targets, whose error stays two orders of magnitude
    above it (extended shapes), so it runs every frame's full count."""
    return np.stack([trap_grid(TOL_FRAMES, *TOL_SHAPE), mraf_frames(TOL_FRAMES, *TOL_SHAPE)[0]], axis=1)


def oracle_chain(targets, loops_first, loops, tol):
    """The float64 oracle of the chain for [F][B][h][w] targets: error lists
    [F][B], each frame warm-started from the phase of the frame before it and
    stopped by `while error > tol`."""
    f_n, b_n = targets.shape[:2]
    errs = [[None] * b_n for _ in range(f_n)]
    for b in range(b_n):
        phase = None
        for f in range(f_n):
            phase, _, e = orc.gerchberg_saxton_faithful(targets[f, b], loops_first if f == 0 else loops, tol,
                                                        initial_phase=phase)
            errs[f][b] = [float(v) for v in e]
    return errs


@functools.lru_cache(maxsize=None)
def tolerance():
    """The geometric mean of two neighbouring values of frame 0's float64 error
    curve (hologram 0) that differ by more than 1 %."""
    e = oracle_chain(tolerance_targets()[:1], TOL_LOOPS, TOL_LOOPS, 0.0)[0][0]
    a, b = e[TOL_PAIR], e[TOL_PAIR + 1]
    assert abs(a - b) > 0.01 * max(a, b), (a, b)
    return float(np.sqrt(a * b))
