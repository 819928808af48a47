#!/usr/bin/env python3
"""Per-iteration kernel time of GS and MRAF plans (slm_plan_run_timed: HIP
events around every launch), column and row pass, at 1 x 1024^2 (float32
target) and 1 x 768 x 1024 (uint8 target, the CLI's shape) unless told otherwise.

    python tools/mraf_timing.py [--iters 50] [--reps 5] [--shapes 1024x1024:f32,768x1024:u8]

Prints the median over `reps` timed runs of the mean time per launch. The
target is a filled ellipse and a rectangle, the region a rectangle around them.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatial_light_modulator_module_amd import _lib  # noqa: E402


def drawn_target(h, w, dtype):
    y, x = np.mgrid[:h, :w]
    cy, cx = h // 4, w // 4
    t = np.zeros((h, w), np.uint8)
    t[((y - cy) / (h / 10)) ** 2 + ((x - cx) / (w / 7)) ** 2 <= 1] = 200
    t[cy + h // 8: cy + h // 8 + h // 12, cx - w // 10: cx + w // 8] = 120
    r = np.zeros((h, w), np.uint8)
    r[cy - h // 6: cy + h // 4 + 2, cx - w // 5: cx + w // 5] = 1
    return t.astype(dtype)[None], r[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="1024x1024:f32,768x1024:u8")
    o = ap.parse_args()
    _lib.init(0)
    for spec in o.shapes.split(","):
        shape, kind = spec.split(":")
        h, w = (int(v) for v in shape.split("x"))
        dtype, tt = (np.uint8, _lib.TGT_U8) if kind == "u8" else (np.float32, _lib.TGT_F32)
        t, r = drawn_target(h, w, dtype)
        res = {}
        for name, algo in (("gs", _lib.ALGO_GS), ("mraf", _lib.ALGO_MRAF)):
            with _lib.Plan(algo, 1, h, w, tt, False, o.iters) as p:
                p.set_target(t)
                if algo == _lib.ALGO_MRAF:
                    p.set_region(r)
                p.run(o.iters)
                p.sync()
                runs = []
                for _ in range(o.reps):
                    us, cnt = p.run_timed(o.iters)
                    runs.append([us[c] / max(cnt[c], 1) for c in (_lib.KERNEL_COL_MAIN, _lib.KERNEL_ROW_MAIN)])
                col, row = np.median(np.array(runs), axis=0)
                res[name] = (col, row)
                info = p.info()
                print(f"{shape} {kind} {name:4s} {info['precision']} engine {info['engine'][0]}: col {col:7.2f} us "
                      f"({p.kernel_bytes(_lib.KERNEL_COL_MAIN) / col / 1e3:5.0f} GB/s)  row {row:7.2f} us  "
                      f"col + row {col + row:7.2f} us per iteration", flush=True)
        (c0, r0), (c1, r1) = res["gs"], res["mraf"]
        print(f"{shape} {kind} mraf / gs: col {c1 / c0:.3f}x, col + row {(c1 + r1) / (c0 + r0):.3f}x", flush=True)


if __name__ == "__main__":
    main()
