"""Trap-trajectory CLI (no reference counterpart): holograms for a moving list
of traps at fractional positions, one chain on the device per trajectory.

    python -m spatial_light_modulator_module_amd.generate_trap_sequence <name> -v V -ct2pi N [-loops 4] [-first 30]
        [-tol 0] [--feedback 1] [--shape 1080x1920] [-ii PATH] [-p]
        [--expected [--follow] [--oversample 8] [--margin 4] [--expected_z 0]]

The reference reaches moving traps in two steps: generate_traps_image_sequence.py
rasterises the positions into images (whole pixels), generate_hologram_sequence.py
runs GS once per image. Here the trajectory itself is the input:
``images/moving_traps/<name>.npy`` is a float array [F][M][2..4] of y, x, then
the defocus z (radians per pixel^2, move_traps.lens_to_z), then the target
intensity, per frame and trap. The frames run as move_traps.trap_array_sequence:
frame 0 at most ``-first`` iterations, every later frame at most ``-loops`` from
the field the frame before ended with, each stopping early once its uniformity
is <= ``-tol``.

Output is the layout generate_hologram_sequence writes, so display_holograms
plays it: ``holograms/<name>_<V>_holograms/<i>.npy`` (float64, hologram_from);
with ``-p`` also the quantised SLM frames as
``images/moving_traps/<name>_<V>_preview/<i>.png``. With ``--expected`` the far
field those uint8 frames produce is written too, as
``images/moving_traps/<name>_<V>_expected/<i>.png``: one window for the whole
trajectory (move_traps.trap_window: every position +- ``--margin`` far-field
pixels, ``--oversample`` samples per pixel, in the plane of ``--expected_z``),
or with ``--follow`` one window per frame around that frame's traps, all of one
size (move_traps.trap_windows). The frames do not leave the device for it: they
are previewed where the sequence left them (trap_array_sequence's ``expected``,
the resident zoom), each image scaled to its own brightest sample. Single GPU
only.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import move_traps
from .algorithms import hologram_from, incoming_amplitude


def parse_shape(text: str):
    """"1080x1920" -> (1080, 1920)."""
    try:
        h, w = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"--shape takes HEIGHTxWIDTH, got {text!r}")
    if h < 2 or w < 2:
        raise argparse.ArgumentTypeError(f"--shape sides must be at least 2, got {text!r}")
    return h, w


def load_trajectory(path):
    """The [F][M][2..4] file as (ys, xs, zs or None, intensity or None), each [F][M]."""
    t = np.load(path)
    if t.ndim != 3 or not 2 <= t.shape[2] <= 4 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{path}: a trajectory is a float array [F][M][2..4] (y, x, z, intensity), got {t.shape}")
    t = t.astype(np.float64)
    return (t[:, :, 0], t[:, :, 1], t[:, :, 2] if t.shape[2] > 2 else None,
            t[:, :, 3] if t.shape[2] > 3 else None)


def output_dirs(name, version):
    """(holograms directory, preview directory), as generate_hologram_sequence names them."""
    return f"holograms/{name}_{version}_holograms", f"images/moving_traps/{name}_{version}_preview"


def expected_dir(name, version):
    """Where --expected writes the zoomed far field of every frame."""
    return f"images/moving_traps/{name}_{version}_expected"


def generate_trap_sequence(args):
    """Runs the trajectory and writes its files; returns the per-frame
    uniformity curves (list of F lists, one value per executed iteration)."""
    ys, xs, zs, inten = load_trajectory(f"images/moving_traps/{args.name}.npy")
    dest_holograms, dest_preview = output_dirs(args.name, args.version)
    os.makedirs(dest_holograms, exist_ok=True)
    if args.preview:
        os.makedirs(dest_preview, exist_ok=True)
    ain = incoming_amplitude(args, args.shape)
    expected = None
    if args.expected:
        expected = dict(margin=args.margin, oversample=args.oversample, z=args.expected_z,
                        follow=getattr(args, "follow", False))
    res = move_traps.trap_array_sequence(args.shape, ys, xs, zs, inten, loops_first=args.first, loops=args.max_loops,
                                         tol=args.tolerance, feedback=args.feedback, ain=ain,
                                         ct2pi=args.correspond_to2pi, holograms=True, expected=expected)
    curves = []
    for i in range(len(res.frames)):
        sys.stdout.write(f"\rcreating {i}. hologram ")
        np.save(f"{dest_holograms}/{i}.npy", hologram_from(res.holograms[i]))
        if args.preview:
            from PIL import Image

            Image.fromarray(res.frames[i]).save(f"{dest_preview}/{i}.png")
        curves.append([float(u) for u in res.stats[i][:int(res.iters[i]), 1]])
    if args.expected:
        write_expected(args, res.expected)
    return curves


def write_expected(args, inten):
    """--expected: what the uint8 frames produce (the zoomed far field
    trap_array_sequence computed from them on the device), each written as an
    8-bit image scaled to its own brightest sample."""
    from PIL import Image

    dest = expected_dir(args.name, args.version)
    os.makedirs(dest, exist_ok=True)
    for i, img in enumerate(inten.astype(np.float64)):
        peak = img.max() or 1.0  # a dark frame stays dark
        Image.fromarray(np.floor(255.0 * img / peak).astype(np.uint8)).save(f"{dest}/{i}.png")  # uint8 2-D: mode L


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                description="Holograms for a moving list of traps (spot-based weighted GS on MI355X).")
    p.add_argument("name", type=str, help="trajectory images/moving_traps/<name>.npy, float [F][M][2..4]")
    p.add_argument("-v", "--version", type=str, required=True,
                   help="suffix distinguishing versions of the same sequence")
    p.add_argument("-ct2pi", "--correspond_to2pi", metavar="INT", required=True, type=int,
                   help="value of pixel corresponding to 2pi phase shift")
    p.add_argument("-loops", "--max_loops", metavar="INT", default=4, type=int,
                   help="iterations per frame after the first, at most")
    p.add_argument("-first", "--first", metavar="INT", default=30, type=int,
                   help="iterations of the first frame, at most")
    p.add_argument("-tol", "--tolerance", metavar="FLOAT", default=0.0, type=float,
                   help="a frame stops once its uniformity std(r) is at or under this (0 = never)")
    p.add_argument("--feedback", metavar="FLOAT", default=1.0, type=float, help="weight feedback exponent")
    p.add_argument("--shape", metavar="HxW", default=(1080, 1920), type=parse_shape,
                   help="panel shape")
    p.add_argument("-ii", "--incomming_intensity", metavar="PATH", type=str, default="uniform",
                   help="incomming intensity image or 'uniform'")
    p.add_argument("-p", "--preview", action="store_true", help="also write the quantised frames as images")
    p.add_argument("--expected", action="store_true",
                   help="also write the far field each quantised frame produces around the traps, as images")
    p.add_argument("--follow", action="store_true",
                   help="--expected: one window per frame around that frame's traps instead of one for the trajectory")
    p.add_argument("--oversample", metavar="INT", default=8, type=int,
                   help="--expected: samples per far-field pixel")
    p.add_argument("--margin", metavar="PX", default=4.0, type=float,
                   help="--expected: far-field pixels shown around the outermost trap positions")
    p.add_argument("--expected_z", metavar="Z", default=0.0, type=float,
                   help="--expected: defocus of the previewed plane, radians per pixel^2")
    return p


def cli(argv=None):
    args = build_parser().parse_args(argv)
    curves = generate_trap_sequence(args)
    print()
    return curves


if __name__ == "__main__":
    cli()
