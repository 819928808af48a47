#!/usr/bin/env python3
"""Kernel time of the zoomed far field (slm_farfield_zoom_timed: HIP events
around the tables, the field pass and each of the two products with its fold,
printed in total and per class) at 1080 x 1920
for windows of 64^2, 256^2 and 1024^2 samples at 1/8 pixel, next to the
matrix-core bound of its two products (8 H W nxp + 8 H nyp nxp FLOP at
157.3 TFLOP/s), and of the route that existed before it: the 256^2 window's
samples as trap lists of 1024 points each through the trap lists' fields
product (slm_spots_run_timed, the fields and update classes of one iteration
per list; its table launches are not in that figure).

    python tools/zoom_timing.py [--shape 1080x1920] [--windows 64,256,1024] [--list-window 256] [--reps 5]

With --handle it times the preview of a trap trajectory's frames instead:
`--frames` uint8 frames of one Spots.sequence at the same shape, per window
(a) what --expected did before the resident zoom, sequence_read of the frames
plus one farfield_zoom call over all of them, as wall time, and (b) run_spots
plus read on a _lib.Zoom handle, as wall time, with the HIP-event kernel time
per class of a timed handle next to it.

    python tools/zoom_timing.py --handle [--frames 32] [--shape ...] [--windows ...] [--reps 5]

Every figure is the median of `reps` runs after one warm-up.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatial_light_modulator_module_amd import _lib  # noqa: E402

MFMA_F32_FLOPS = 157.3e12
PITCH = 0.125


def window(n):
    return (-n * PITCH / 2, -n * PITCH / 2), PITCH, (n, n)


def zoom_us(phase, n, reps):
    origin, pitch, size = window(n)
    runs = np.array([_lib.farfield_zoom(phase, origin, pitch, size, timed=True)[1] for _ in range(reps + 1)])[1:]
    return float(np.median(runs.sum(axis=1))), np.median(runs, axis=0)


def list_route_us(phase, n, reps):
    """The n x n window through Spots in lists of 1024 points: (microseconds, lists)."""
    h, w = phase.shape
    origin, pitch, size = window(n)
    ys = np.repeat(origin[0] + np.arange(n) * pitch, n)
    xs = np.tile(origin[1] + np.arange(n) * pitch, n)
    lists = [(ys[s:s + 1024], xs[s:s + 1024]) for s in range(0, n * n, 1024)]
    runs = []
    with _lib.Spots(1, h, w, 1024, False, 1) as sp:
        sp.set_phase(phase[None])
        for rep in range(reps + 1):
            total = 0.0
            for y, x in lists:
                sp.set_traps(y, x)
                us = sp.run_timed(1)
                total += us[_lib.SPOTS_KERNEL_FIELDS] + us[_lib.SPOTS_KERNEL_UPDATE]
            runs.append(total)
    return float(np.median(runs[1:])), len(lists)


def wall_ms(fn, reps):
    runs = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        runs.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(runs[1:]))


def handle_mode(h, w, windows, n_frames, reps):
    """The frames of one trajectory, previewed by the one-shot from the host and by the handle in place."""
    m, ct2pi = 8, 256
    rng = np.random.default_rng(2)
    start = rng.uniform(-3.0, 3.0, (m, 2))
    step = rng.uniform(-0.02, 0.02, (m, 2))
    traj = np.stack([start + f * step for f in range(n_frames)])[:, None]  # [F][1][M][2]
    ys, xs = np.ascontiguousarray(traj[..., 0]), np.ascontiguousarray(traj[..., 1])
    print(f"resident zoom at {h} x {w}: {n_frames} uint8 frames of a {m}-trap trajectory, pitch {PITCH}; wall time "
          f"in ms and HIP-event kernel time in us, median of {reps} after one warm-up", flush=True)
    with _lib.Spots(1, h, w, m, False, 10) as sp:
        sp.sequence(ys, xs, loops_first=10, loops=2, ct2pi=ct2pi)
        sp.sequence_read()
        for n in windows:
            origin, pitch, size = window(n)

            def one_shot():
                frames = sp.sequence_read(fields=False, stats=False, weights=False, iters=False)[0]
                return _lib.farfield_zoom(frames[:, 0], origin, pitch, size, ct2pi=ct2pi)

            with _lib.Zoom(n_frames, h, w, size) as zm, _lib.Zoom(n_frames, h, w, size, timed=True) as tz:
                def resident():
                    zm.run_spots(sp, 0, n_frames, ct2pi)
                    return zm.read()

                for z in (zm, tz):
                    z.set_window(origin, pitch, size)
                same = np.array_equal(one_shot(), resident())
                a, b = wall_ms(one_shot, reps), wall_ms(resident, reps)
                per = []
                for _ in range(reps + 1):
                    tz.run_spots(sp, 0, n_frames, ct2pi)
                    per.append(tz.read()[1])
                per = np.median(np.array(per[1:]), axis=0)
                info = zm.info()
            classes = "  ".join(f"{name} {t:9.1f}" for name, t in zip(_lib.ZOOM_KERNEL_CLASS_NAMES, per))
            print(f"window {n:4d}^2: (a) sequence_read + farfield_zoom {a:9.2f} ms | (b) run_spots + read {b:9.2f} ms "
                  f"| ratio {a / b:6.1f} | kernels {per.sum():9.1f} us = {per.sum() / n_frames:7.1f} us per frame "
                  f"({classes}) | groups {info['groups']} bands {info['bands']} split launches "
                  f"{info['split_launches']} | same bits: {same}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1080x1920")
    ap.add_argument("--windows", default="64,256,1024")
    ap.add_argument("--list-window", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--handle", action="store_true", help="time the resident zoom on a trajectory's frames instead")
    ap.add_argument("--frames", type=int, default=32, help="--handle: frames of the trajectory")
    o = ap.parse_args()
    h, w = (int(v) for v in o.shape.split("x"))
    _lib.init(0)
    if o.handle:
        handle_mode(h, w, [int(v) for v in o.windows.split(",")], o.frames, o.reps)
        return
    phase = np.random.default_rng(1).uniform(-np.pi, np.pi, (h, w)).astype(np.float32)
    print(f"zoomed far field at {h} x {w}, pitch {PITCH}; kernel time by HIP events, median of {o.reps} after one "
          "warm-up", flush=True)
    zoom = {}
    for n in (int(v) for v in o.windows.split(",")):
        zoom[n], per = zoom_us(phase, n, o.reps)
        npad = -(-n // 32) * 32
        flop = 8.0 * h * w * npad + 8.0 * h * npad * npad
        bound = flop / MFMA_F32_FLOPS * 1e6
        classes = "  ".join(f"{name} {t:8.1f}" for name, t in zip(_lib.ZOOM_KERNEL_CLASS_NAMES, per))
        print(f"window {n:4d}^2: {zoom[n]:10.1f} us ({classes}) | {flop / 1e9:7.2f} GFLOP, matrix-core bound "
              f"{bound:8.1f} us ({100 * bound / zoom[n]:4.1f} % reached, {flop / zoom[n] / 1e6:6.1f} TFLOP/s)",
              flush=True)
    n = o.list_window
    t_list, count = list_route_us(phase, n, o.reps)
    t_zoom = zoom[n] if n in zoom else zoom_us(phase, n, o.reps)[0]
    print(f"window {n:4d}^2 as {count} trap lists of 1024 points (fields + update kernels): {t_list:10.1f} us | "
          f"zoom {t_zoom:10.1f} us | ratio {t_list / t_zoom:6.1f}", flush=True)


if __name__ == "__main__":
    main()
