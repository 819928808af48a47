#!/usr/bin/env python3
"""SHA-256 digests of what the one-shot zoomed far field (slm_farfield_zoom)
and a small trap-list run (slm_spots_run / slm_spots_read) return, one line per
case, so that two builds of the library can be compared bit for bit:

    python tools/zoom_digest.py > digest_a.txt     # build A
    python tools/zoom_digest.py > digest_b.txt     # build B ($SLM_LIB_PATH picks a library)
    diff digest_a.txt digest_b.txt

A zoom line is the digest over the intensity bytes followed by the field bytes.
The cases are those the GPU tests hold bit for bit or to the reference: the
five batched cases of tests/test_gpu_zoom_handle.py (BITWISE), the six shapes
of tests/test_gpu_zoom.py (PARITY) with a_in and z = 2e-4, and the window whose
chunk results exceed the 64 MB cap, so that it runs in two bands. The trap-list
line is a 45 x 70 hologram with 5 traps after 6 iterations: phase, fields and
statistics.
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spatial_light_modulator_module_amd import _lib  # noqa: E402

ORIGIN, PITCH = (-3.375, 2.625), 0.125  # dyadic: y0 + j dy is exact

# (label, (H, W), windows, B, uint8 ct2pi or None, a_in, z): tests/test_gpu_zoom_handle.py
BITWISE = [
    ("nothing-a-multiple-of-32", (45, 70), [(33, 70)], 3, None, True, 2e-4),
    ("three-chunks-in-product-1", (130, 600), [(70, 90)], 2, None, False, 2e-4),
    ("three-chunks-in-product-2", (600, 45), [(70, 90)], 2, None, False, 2e-4),
    ("both-forms-of-product-1", (1056, 300), [(8, 40), (8, 4096)], 2, None, False, 2e-4),
    ("uint8-levels", (130, 264), [(33, 70)], 3, 200, True, 1e-4),
]
# (H, W), (ny, nx): tests/test_gpu_zoom.py
PARITY = [((45, 70), (33, 70)), ((64, 64), (1, 1)), ((64, 64), (32, 32)), ((130, 264), (96, 40)),
          ((64, 4096), (40, 40)), ((4096, 64), (40, 40))]
BANDED = ((1056, 300), (1300, 1300))  # 5 chunks x 1312 x 1312 x 8 B = 68.9 MB of chunk results


def gauss(h, w):
    """A wide Gaussian on a 0.2 pedestal, float32."""
    y = (np.arange(h)[:, None] - h / 2) / (0.35 * h)
    x = (np.arange(w)[None, :] - w / 2) / (0.35 * w)
    return (0.2 + np.exp(-(y ** 2 + x ** 2))).astype(np.float32)


def sha(*arrays):
    d = hashlib.sha256()
    for a in arrays:
        d.update(np.ascontiguousarray(a).tobytes())
    return d.hexdigest()


def zoom_line(label, holos, origin, pitch, size, z, ain, ct2pi):
    inten, field = _lib.farfield_zoom(holos, origin, pitch, size, z=z, ain=ain, ct2pi=ct2pi, return_field=True)
    assert inten.dtype == np.float32 and field.dtype == np.complex128
    print(f"{sha(inten, field)}  zoom {label} window {size[0]}x{size[1]}", flush=True)


def main():
    _lib.init(0)
    for label, (h, w), sizes, b, ct2pi, with_ain, z in BITWISE:
        rng = np.random.default_rng(5)
        holos = (rng.integers(0, 256, (b, h, w), dtype=np.uint8) if ct2pi
                 else rng.uniform(-np.pi, np.pi, (b, h, w)).astype(np.float32))
        for size in sizes:
            zoom_line(f"bitwise {label} {b}x{h}x{w}", holos, ORIGIN, PITCH, size, z, gauss(h, w) if with_ain else None,
                      ct2pi)
    for (h, w), size in PARITY:
        phase = np.random.default_rng(3 + h + w).uniform(-np.pi, np.pi, (h, w)).astype(np.float32)
        zoom_line(f"parity {h}x{w}", phase, (-h / 8 + 0.3125, w / 16 - 1.71), PITCH, size, 2e-4, gauss(h, w), None)
    (h, w), size = BANDED
    phase = np.random.default_rng(23).uniform(-np.pi, np.pi, (h, w)).astype(np.float32)
    zoom_line(f"banded {h}x{w}", phase, ORIGIN, PITCH, size, 2e-4, None, None)

    h, w, m, loops = 45, 70, 5, 6
    ys = np.array([[-9.5, -6.0, 7.25, 10.5, 0.5]])
    xs = np.array([[-14.25, 11.5, -8.0, 15.75, 2.25]])
    with _lib.Spots(1, h, w, m, False, loops) as sp:
        sp.set_traps(ys, xs)
        sp.run(loops)
        phase, fields, stats, _ = sp.read()
    print(f"{sha(phase, fields, stats)}  spots {h}x{w} {m} traps {loops} loops: phase, fields, stats", flush=True)


if __name__ == "__main__":
    main()
