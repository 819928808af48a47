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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="1080x1920,1024x1024")
    ap.add_argument("--traps", default="16,64,256,1024")
    o = ap.parse_args()
    _lib.init(0)
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
