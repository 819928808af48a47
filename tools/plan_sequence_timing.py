#!/usr/bin/env python3
"""Image sequences: the device-resident chain (Plan.sequence) against the host
loop written with the API that existed before it, on a grid of 12 single-pixel
traps that moves one pixel per frame.

    python tools/plan_sequence_timing.py [--side both|host|chain] [--frames 32] [--loops 5] [--reps 5]
                                         [--cases 768x1024:u8:gs,768x1024:u8:gsw,1024x1024:f32:gs,1080x1920:u8:gs]

Wall clock, median of `reps` after one warm-up (with minimum and maximum, the
run-to-run spread), microseconds per frame, of three ways to get the uint8
frames of the sequence:

  chain      Plan.sequence(...) + sequence_read(frames): one upload, one
             enqueued chain, one download of 1 B per pixel and frame
  host warm  per frame set_target, set_phase(previous phase), run, read(phase),
             hologram_from, quantize: the loop the chain is defined by
  host cold  the same without set_phase: every frame from ifft2(a_T), what
             generate_hologram_sequence does per frame today

`--side host` uses nothing the chain added, so it runs unchanged on the commit
before it: that is how the baseline is taken. "device" is the chain's time on
the GPU alone (slm_plan_mark around the enqueue). The last column block is the
error after `loops` iterations of frames 1 .. F-1, chained against cold, as the
median over those frames and the number of frames where the chain is lower.
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatial_light_modulator_module_amd import _lib  # noqa: E402
from spatial_light_modulator_module_amd.algorithms import hologram_from  # noqa: E402

ALGOS = {"gs": _lib.ALGO_GS, "gsw": _lib.ALGO_GSW}


def trap_grid(n_frames, h, w, dtype):
    """tests/plan_sequence_cases.py's grid: 3 x 4 traps of 255, one pixel to the right per frame."""
    out = np.zeros((n_frames, 1, h, w), np.uint8)
    ys = [h // 8 + i * (h // 5) for i in range(3)]
    for f in range(n_frames):
        out[f, 0][np.ix_(ys, [w // 10 + j * (w // 6) + f for j in range(4)])] = 255
    return out.astype(dtype)


def spread(fn, reps):
    fn()  # warm-up
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        runs.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(runs)), float(min(runs)), float(max(runs))


def host_loop(plan, targets, loops, warm):
    """(frames, final error per frame) through the existing API."""
    prev, frames, errs = None, [], []
    plan.set_phase(None)
    for t in targets:
        plan.set_target(t)
        if warm and prev is not None:
            plan.set_phase(prev)
        plan.run(loops)
        prev, _, stats, _ = plan.read(expected=False)
        frames.append(_lib.quantize(hologram_from(prev), None, 256.0, _lib.QUANT_PIL))
        errs.append(stats[0, loops - 1, 3])
    return frames, np.array(errs)


def commit():
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        out = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        return out.stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", default="both", choices=["both", "host", "chain"])
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="768x1024:u8:gs,768x1024:u8:gsw,1024x1024:f32:gs,1080x1920:u8:gs")
    ap.add_argument("--label", default=None, help="what to print as the commit (default: git rev-parse)")
    o = ap.parse_args()
    _lib.init(0)
    fr, loops = o.frames, o.loops
    print(f"image sequences on {_lib.load().slm_version().decode()}, commit {o.label or commit()}, side {o.side}: "
          f"{fr} frames, {loops} iterations per frame, tol 0, uint8 frames out; wall clock, median [min .. max] of "
          f"{o.reps} after one warm-up; microseconds per frame", flush=True)
    for case in o.cases.split(","):
        shape, dt, alg = case.split(":")
        h, w = (int(v) for v in shape.split("x"))
        dtype, tt = (np.uint8, _lib.TGT_U8) if dt == "u8" else (np.float32, _lib.TGT_F32)
        t = trap_grid(fr, h, w, dtype)
        line = f"{shape} {dt} {alg}:"
        with _lib.Plan(ALGOS[alg], 1, h, w, tt, False, loops) as plan:
            e_chain = None
            if o.side != "host":
                def chain():
                    plan.set_phase(None)
                    plan.sequence(t, loops_first=loops, loops=loops, frames=True)
                    return plan.sequence_read(frames=True, stats=True, iters=False)

                med, lo, hi = spread(chain, o.reps)
                plan.set_phase(None)
                plan.mark(0)
                plan.sequence(t, loops_first=loops, loops=loops, frames=True)
                plan.mark(1)
                dev = plan.marked_ms() * 1e3 / fr
                e_chain = chain()[3][:, 0, loops - 1, 3]
                line += f" chain {med / fr:8.1f} [{lo / fr:8.1f} .. {hi / fr:8.1f}] (device {dev:7.1f}) |"
            if o.side != "chain":
                warm = spread(lambda: host_loop(plan, t, loops, True), o.reps)
                cold = spread(lambda: host_loop(plan, t, loops, False), o.reps)
                line += (f" host warm {warm[0] / fr:8.1f} [{warm[1] / fr:8.1f} .. {warm[2] / fr:8.1f}] | host cold "
                         f"{cold[0] / fr:8.1f} [{cold[1] / fr:8.1f} .. {cold[2] / fr:8.1f}] |")
                if o.side == "both":
                    line += f" host warm / chain {warm[0] / med:5.2f} | host cold / chain {cold[0] / med:5.2f} |"
                e_cold = host_loop(plan, t, loops, False)[1]
                e_warm = e_chain if e_chain is not None else host_loop(plan, t, loops, True)[1]
                line += (f" error after {loops} iterations, frames 1..{fr - 1}: chained median "
                         f"{np.median(e_warm[1:]):.4g}, cold median {np.median(e_cold[1:]):.4g}, chained lower in "
                         f"{int(np.sum(e_warm[1:] < e_cold[1:]))} of {fr - 1}")
        print(line, flush=True)


if __name__ == "__main__":
    main()
