"""Trap-sequence CLI, drop-in for src/generate_hologram_sequence.py.

    python -m spatial_light_modulator_module_amd.generate_hologram_sequence <source_dir> -v V -ct2pi N [-loops 5] [-p]

The reference runs gerchberg_saxton once per frame (src/generate_hologram_sequence.py:10-31);
frames are independent, so here they run as batches of holograms in one plan
(one launch pair per GS iteration for the whole batch), and under a
one-process-per-GPU launcher (torch.distributed.run or any that sets RANK /
WORLD_SIZE / MASTER_ADDR / MASTER_PORT) each rank takes a contiguous shard of
the frames (parallel.shard_range) and writes its own .npy files: no collective
touches the data path; only the per-frame error lists travel, over the
torch-free control plane (parallel.Group). Without a launcher, $SLM_GPUS (a
device count, "all", or a comma-separated device list) runs each batch over
several GPUs from this one process instead (slm_gs_multi).
Output files, names and stdout lines are the reference's.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import parallel
from . import _lib
from .algorithms import (_check_shape, _iterations_allowed, _print_loops, expected_from, hologram_from,
                         incoming_amplitude, run_gs, run_gs_multi, run_gsw, run_sequence)

SEQ_BATCH = int(os.environ.get("SLM_SEQ_BATCH", "64"))  # frames per GPU launch batch
SEQ_CHAIN = int(os.environ.get("SLM_SEQ_CHAIN", "256"))  # frames per enqueued chain (--chain)


def _load_frame(source_dir_path, i):
    from PIL import Image

    return np.array(Image.open(f"{source_dir_path}/{i}.png"))


def _runs(indices, frames, ends):
    """Split an index list into runs of equal shape and dtype; ends(run, i)
    tells whether frame i may not join `run` for another reason."""
    run = []
    for i in indices:
        if run and (ends(run, i) or frames[i].shape != frames[run[0]].shape
                    or frames[i].dtype != frames[run[0]].dtype):
            yield run
            run = []
        run.append(i)
    if run:
        yield run


def _batches(indices, frames):
    """Split an index list into runs of equal shape and dtype, at most SEQ_BATCH long."""
    return _runs(indices, frames, lambda run, i: len(run) == SEQ_BATCH)


def _chains(indices, frames):
    """Split an index list into runs of consecutive frames of equal shape and dtype."""
    return _runs(indices, frames, lambda run, i: i != run[-1] + 1)


def _ain_for(args, frame):
    """What gerchberg_saxton does before its loop, for the frames of frame's shape."""
    _check_shape(frame)
    ain = incoming_amplitude(args, frame.shape)
    if not _iterations_allowed(args):
        raise UnboundLocalError("local variable 'expected_outcome' referenced before assignment")
    return ain


def _write_frames(args, dest_dirs, idx, phase, e, errs, norm, emax):
    """The reference's lines and files for frames idx, from run_gs's result
    for them; returns their error evolutions."""
    from PIL import Image

    for k, i in enumerate(idx):
        sys.stdout.write(f"\rcreating {i}. hologram ")
        _print_loops(len(errs[k]), args.max_loops)
        np.save(f"{dest_dirs[0]}/{i}.npy", hologram_from(phase[k]))
        if args.preview:
            expected = expected_from(e[k], norm[k], emax[k])
            Image.fromarray(expected).convert("L").save(f"{dest_dirs[1]}/{i}.png")
    return dict(zip(idx, errs))


def _chained(args, mine, frames, dest_dirs):
    """--chain: this rank's frames as device-resident chains (run_sequence):
    every frame after the first of a run starts from the phase of the frame
    before it. A run longer than SEQ_CHAIN goes in pieces, each continued from
    the last phase of the piece before it, which is the uncut chain."""
    algorithm = getattr(args, "algorithm", "gerchberg_saxton")
    feedback = float(getattr(args, "feedback", 1.0))
    errors = {}
    for run in _chains(mine, frames):
        ain = _ain_for(args, frames[run[0]])
        last = None
        for at in range(0, len(run), SEQ_CHAIN):
            idx = run[at:at + SEQ_CHAIN]
            stack = np.stack([frames[i] for i in idx])
            phase, _, errs, norm, emax, e = run_sequence(stack, args.max_loops, args.max_loops, algorithm,
                                                         args.tolerance, ain, last, feedback, return_expected=True)
            last = phase[-1]
            # a frame of the chain is a batch of one hologram
            errors.update(_write_frames(args, dest_dirs, idx, phase[:, 0], e[:, 0], [x[0] for x in errs],
                                        norm[:, 0], emax[:, 0]))
    return errors


def multi_devices(nranks):
    """Devices for one-process multi-GPU batches ($SLM_GPUS), or None."""
    spec = os.environ.get("SLM_GPUS", "").strip()
    if not spec or nranks > 1:
        return None
    if "," in spec:
        devs = [int(d) for d in spec.split(",") if d.strip()]
    else:
        devs = list(range(_lib.device_count() if spec == "all" else int(spec)))
    return devs if len(devs) > 1 else None


def generate_hologram_sequence(args, rank=None, nranks=None):
    """src/generate_hologram_sequence.py:10-31. Returns the per-frame error
    evolutions of the frames this rank computed (dict frame -> list)."""
    if rank is None:
        rank, nranks, _ = parallel.world()
    dest_dirs = (f"holograms/{args.source_dir}_{args.version}_holograms",
                 f"images/moving_traps/{args.source_dir}_{args.version}_preview")
    for dest_dir in dest_dirs:
        os.makedirs(dest_dir, exist_ok=True)
    source_dir_path = f"images/moving_traps/{args.source_dir}"
    n_files = len(os.listdir(source_dir_path))
    mine = list(parallel.shard_range(n_files, nranks, rank))
    frames = {i: _load_frame(source_dir_path, i) for i in mine}
    errors = {}
    if getattr(args, "chain", False):
        return _chained(args, mine, frames, dest_dirs)
    devices = multi_devices(nranks)
    for idx in _batches(mine, frames):
        stack = np.stack([frames[i] for i in idx])
        ain = _ain_for(args, stack[0])
        # -alg weighted_gerchberg_saxton (no reference counterpart): the same batches, weighted GS
        feedback = (float(getattr(args, "feedback", 1.0))
                    if getattr(args, "algorithm", "gerchberg_saxton") == "weighted_gerchberg_saxton" else None)
        if devices:
            result = run_gs_multi(stack, args.max_loops, devices, args.tolerance, ain, feedback)
        elif feedback is not None:
            result = run_gsw(stack, args.max_loops, feedback, args.tolerance, ain)
        else:
            result = run_gs(stack, args.max_loops, args.tolerance, ain)
        errors.update(_write_frames(args, dest_dirs, idx, *result))
    return errors


def plot_error_evolution(err_evl_list):
    """src/generate_hologram_sequence.py:34-39."""
    import matplotlib.pyplot as plt

    for i, err_evl in enumerate(err_evl_list):
        plt.plot(err_evl, label=i)
    plt.legend()
    plt.show()


def build_parser():
    """Argument set of src/generate_hologram_sequence.py:52-103."""
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                description="Transform a sequence of trap images into holograms (GS on MI355X).")
    p.add_argument("source_dir", type=str, help="directory of trap images inside images/moving_traps")
    p.add_argument("-v", "--version", type=str, help="suffix distinguishing versions of the same sequence")
    p.add_argument("-ii", "--incomming_intensity", metavar="PATH", type=str, default="uniform",
                   help="incomming intensity image or 'uniform'")
    p.add_argument("-ct2pi", "--correspond_to2pi", metavar="INT", required=True, type=int,
                   help="value of pixel corresponding to 2pi phase shift")
    p.add_argument("-tol", "--tolerance", metavar="FLOAT", default=0, type=float,
                   help="algorithm stops when error descends under tolerance")
    p.add_argument("-loops", "--max_loops", metavar="INT", default=5, type=int,
                   help="algorithm performs no more than max_loops loops")
    p.add_argument("-p", "--preview", action="store_true", help="also write expected images")
    p.add_argument("-alg", "--algorithm", default="gerchberg_saxton",
                   choices=["gerchberg_saxton", "weighted_gerchberg_saxton"],
                   help="algorithm (weighted_gerchberg_saxton evens out the trap intensities)")
    p.add_argument("--feedback", metavar="FLOAT", default=1.0, type=float,
                   help="weight feedback exponent of weighted_gerchberg_saxton")
    p.add_argument("--chain", action="store_true",
                   help="run consecutive frames as one device-resident chain, each frame starting from the phase of "
                        "the frame before it (no reference counterpart)")
    return p


def cli(argv=None, plot=True):
    args = build_parser().parse_args(argv)
    args.gif = False
    args.plot_error = False
    args.print_info = False
    rank, nranks, _ = parallel.world()
    errors = generate_hologram_sequence(args, rank, nranks)
    if nranks > 1:
        # error lists are host objects; the phases went to disk
        with parallel.Group.from_env() as group:
            gathered = group.all_gather(errors)
        errors = {k: v for part in gathered for k, v in part.items()}
    print()
    if plot and rank == 0:
        plot_error_evolution([errors[i] for i in sorted(errors)])
    return errors


if __name__ == "__main__":
    cli()
