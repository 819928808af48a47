#!/usr/bin/env python3
"""Per-iteration kernel time of spot-based weighted GS on trap lists
(slm_spots_run_timed: HIP events around every launch), per kernel class, at
1080 x 1920 and 1024^2 with 16, 64, 256 and 1024 traps unless told otherwise.

    python tools/spots_timing.py [--iters 50] [--reps 5] [--shapes 1080x1920,1024x1024] [--traps 16,64,256,1024]

Prints the median over `reps` timed runs of the time per iteration, next to the
two bounds of the MI355X: the matrix cores (16 H W Mp FLOP at 157.3 TFLOP/s,
float32 MFMA) and the memory (the bytes every iteration has to move at least
once, at 8 TB/s): the field read by the fields kernel and written by the
superposition, each table once per kernel, and the partial sums. At 1024^2 the
FFT-based weighted GS plan (SLM_ALGO_GSW) is timed on the same device for
context.

    python tools/spots_timing.py --sequence [--frames 50] [--loops 4] [--reps 5] [--shapes ...] [--traps 16,64,256]

times a trajectory of `frames` frames at `loops` iterations each (tol = 0, uint8
frames wanted) two ways, as wall clock, median of `reps` after one warm-up:
the device-resident sequence (Spots.sequence + sequence_read of the frames) and
the host loop it replaces (move_traps.trap_array_frame per frame with
initial_phase / initial_weights = the previous frame's). Both produce frames
for the same trajectory. Where the sequence's time goes: "output" is what
reading the frames back adds over reading the iteration counts alone,
"iterations" what `loops` iterations cost in the chain (the difference between
a sequence at 2 `loops` and one at `loops` iterations per frame, frames not
read), "tables + rest" what remains: the table launch per frame, the
coordinate upload and the host's share of the launches.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatial_light_modulator_module_amd import _lib  # noqa: E402

MFMA_F32_FLOPS = 157.3e12
HBM_BYTES_PER_S = 8e12


def trap_list(h, w, m):
    rng = np.random.default_rng(1)
    return (rng.uniform(-h / 4, h / 4, m), rng.uniform(-w / 4, w / 4, m),
            rng.uniform(-1, 1, m) * 4 * np.pi / (h * h + w * w), rng.uniform(0.5, 1.0, m))


def fft_gsw_us(h, w, iters, reps):
    rng = np.random.default_rng(1)
    t = np.zeros((h, w), np.float32)
    t.flat[rng.choice(h * w, 40, replace=False)] = rng.integers(60, 256, 40)
    with _lib.Plan(_lib.ALGO_GSW, 1, h, w, _lib.TGT_F32, False, iters) as p:
        p.set_target(t[None])
        p.run(iters)
        p.sync()
        runs = []
        for _ in range(reps):
            us, cnt = p.run_timed(iters)
            runs.append(sum(us[c] / max(cnt[c], 1) for c in (_lib.KERNEL_COL_MAIN, _lib.KERNEL_ROW_MAIN)))
    return float(np.median(runs))


def trajectory(h, w, m, frames):
    ys, xs, zs, inten = trap_list(h, w, m)
    rng = np.random.default_rng(7)
    vy, vx = rng.uniform(-0.3, 0.3, m), rng.uniform(-0.3, 0.3, m)
    f = np.arange(frames, dtype=np.float64)[:, None]
    return ys + f * vy, xs + f * vx, zs * (1 + 0.05 * f), np.broadcast_to(inten, (frames, m)).copy()


def wall_us(fn, reps):
    import time

    fn()  # warm-up
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        runs.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(runs))


def sequence_mode(o):
    from spatial_light_modulator_module_amd import move_traps

    fr, loops = o.frames, o.loops
    print(f"trap trajectories: {fr} frames, {loops} iterations per frame, tol 0, uint8 frames; wall clock, median of "
          f"{o.reps} after one warm-up; microseconds per frame", flush=True)
    for spec in o.shapes.split(","):
        h, w = (int(v) for v in spec.split("x"))
        for m in (int(v) for v in o.traps.split(",")):
            ys, xs, zs, inten = trajectory(h, w, m, fr)
            with _lib.Spots(1, h, w, m, False, 2 * loops) as sp:
                def seq(read_frames=True, n=loops):
                    sp.sequence(ys[:, None], xs[:, None], zs[:, None], inten[:, None], loops_first=n, loops=n,
                                tol=0.0, frames=True)
                    return sp.sequence_read(frames=read_frames, fields=False, stats=False, weights=False)

                t_seq = wall_us(seq, o.reps) / fr
                t_noread = wall_us(lambda: seq(False), o.reps) / fr
                t_it = wall_us(lambda: seq(False, 2 * loops), o.reps) / fr - t_noread

            def host_loop():
                holo = wt = None
                for f in range(fr):
                    holo, _, _, _, wt = move_traps.trap_array_frame((h, w), ys[f], xs[f], zs[f], inten[f], loops=loops,
                                                                    initial_phase=holo, initial_weights=wt)

            t_host = wall_us(host_loop, o.reps) / fr
            move_traps.clear_spots()
            print(f"{spec} M {m:4d}: sequence {t_seq:9.1f} us per frame (iterations {t_it:8.1f}, output "
                  f"{t_seq - t_noread:8.1f}, tables + rest {t_noread - t_it:8.1f}) | host loop {t_host:9.1f} us per "
                  f"frame | ratio {t_host / t_seq:5.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="1080x1920,1024x1024")
    ap.add_argument("--traps", default="16,64,256,1024")
    ap.add_argument("--sequence", action="store_true", help="time trap trajectories against the host loop")
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--loops", type=int, default=4)
    o = ap.parse_args()
    _lib.init(0)
    if o.sequence:
        if o.traps == ap.get_default("traps"):
            o.traps = "16,64,256"
        return sequence_mode(o)
    for spec in o.shapes.split(","):
        h, w = (int(v) for v in spec.split("x"))
        for m in (int(v) for v in o.traps.split(",")):
            with _lib.Spots(1, h, w, m, False, o.iters) as sp:
                sp.set_traps(*trap_list(h, w, m))
                sp.run(o.iters)
                sp.read(fields=False, stats=False, weights=False)
                runs = np.array([sp.run_timed(o.iters) / o.iters for _ in range(o.reps)])
                info = sp.info()
            f, u, s = np.median(runs, axis=0)
            total = float(np.median(runs.sum(axis=1)))
            mp = info["padded_traps"]
            mfma_us = 16.0 * h * w * mp / MFMA_F32_FLOPS * 1e6
            table = 8 * (h + w) * mp
            nbytes = 2 * (8 * h * w + table) + 2 * 16 * info["partials"] * mp
            mem_us = nbytes / HBM_BYTES_PER_S * 1e6
            print(f"{spec} M {m:4d} (Mp {mp:4d}, {info['partials']:4d} partials of {info['cols_per_partial']:4d} "
                  f"columns): fields {f:8.2f} us  update {u:6.2f} us  superpose {s:8.2f} us  total {total:8.2f} us "
                  f"per iteration | matrix-core bound {mfma_us:7.2f} us ({100 * mfma_us / total:4.1f} % reached, "
                  f"{16.0 * h * w * mp / total / 1e6:6.1f} TFLOP/s) | {nbytes / 1e6:6.1f} MB at least, "
                  f"memory bound {mem_us:5.2f} us ({nbytes / total / 1e3:5.0f} GB/s of 8000)", flush=True)
        if _lib.load().slm_supported_length(h) and _lib.load().slm_supported_length(w):
            print(f"{spec} FFT-based weighted GS plan (SLM_ALGO_GSW, float32, column + row pass): "
                  f"{fft_gsw_us(h, w, o.iters, o.reps):.2f} us per iteration, whatever the trap count", flush=True)


if __name__ == "__main__":
    main()
