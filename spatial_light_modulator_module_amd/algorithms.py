"""Drop-in replacement for src/algorithms.py's hot path, running on MI355X.

``gerchberg_saxton(demanded_output, args)`` and
``gradient_descent(demanded_output, args)`` keep the reference signatures
(src/algorithms.py:10, :60), read the same ``args`` attributes, print the same
progress lines, mutate ``args.learning_rate`` the same way, raise the same
exceptions and return the same ``(hologram, expected_outcome,
error_evolution)`` triple (float64 arrays and a list of np.float64). All
iteration arithmetic runs in libslm_hip.so; this module only prepares inputs
(dtype rules, initial guesses) and formats results.

Engines and the cost model (see DESIGN.md sections 1, 3 and 5):

* image sides both in SUPPORTED_LENGTHS (2^k from 64 to 4096, and 768): the
  fused FFT kernels, two launches per iteration, loop state in complex64 in
  HBM; float32 butterflies, twiddles and projections for float32 targets
  (GS 1024^2: ~0.017 ms per iteration), float64 butterflies for uint8 GS
  targets (the CLI's input; ~0.019 ms) -- Plan.set_precision or
  $SLM_PRECISION=f32|f64 overrides. Phases match the float64 reference to
  <= 1e-5 rms under the warm-start protocol of SURVEY.md 8c, not bitwise;
* $SLM_ENGINE=float64 on such sides: the complex128 radix-plan kernels
  (complex128 state, float64 arithmetic, the reference's own dtypes; GS
  4096^2 ~0.5 ms, GD 1024^2 ~0.05 ms per iteration);
* 13-smooth SLM panel sides (600, 800, 1000, 1080, 1152, 1200, 1280, 1536,
  1920, and 2^k / 768 on the other axis): the radix kernels on mixed-E
  Stockham plans -- float32 GS targets in complex64 with the float32 engine's
  numerics (GS 1080 x 1920: ~0.043 ms per iteration), uint8 GS, GD and
  float64 runs in complex128 (GS ~0.061, GD ~0.082 ms);
* any other shape whose sides factor into 2, 3, 5, 7, 11, 13: the float64
  mixed-radix kernels, complex128 state, two launches per iteration (~0.08 ms
  per iteration at 2 Mpixel);
* a side with a larger prime factor (97, 1272 = 8 * 3 * 53, ...): float64
  1-D line transforms along rows and transposed columns, Bluestein's chirp-z
  for that side -- O(N log N), several launches per transform.

A float64 target is carried as float32 on the device, with its max and sum of
squares (the error's constant terms) kept exact in float64.

Beyond the reference: ``weighted_gerchberg_saxton(demanded_output, args)`` and
``run_gsw`` run GS with a per-pixel weight feedback that evens out trap
intensities ("Weighted GS"), on the fused kernels' shapes
only. Nothing of the drop-in changes with it. ``mraf(demanded_output, args)``
and ``run_mraf`` run GS with a signal region (mixed-region amplitude freedom,
for smooth extended shapes; DESIGN.md section 3, "MRAF"), on the same shapes.
"""
from __future__ import annotations

import collections
import os
import sys
import warnings

import numpy as np

from . import _lib
from ._lib import ALGO_GD, ALGO_GS, ALGO_GSW, ALGO_MRAF, TGT_F32, TGT_U8

# ---------------------------------------------------------------------------
# input preparation (reference dtype rules)
# ---------------------------------------------------------------------------


def _side_supported(n: int) -> bool:
    """One line is one workgroup's LDS (8192 complex128): a 13-smooth side up
    to 8192 transforms directly, any other side by chirp-z over a length
    >= 2n - 1, so up to 4096."""
    if n <= 4096:
        return True
    if n > 8192:
        return False
    for p in (2, 3, 5, 7, 11, 13):
        while n % p == 0:
            n //= p
    return n == 1


def _check_shape(t: np.ndarray):
    """(h, w) with every side up to 4096, or up to 8192 where the side has no
    prime factor above 13 (the reference takes any shape,
    src/algorithms.py:20-27): sides in SUPPORTED_LENGTHS run the fused FFT
    kernels, every other shape the float64 any-size engine (csrc/generic.hip:
    mixed-radix kernels for 13-smooth sides, chirp-z line transforms
    otherwise, whose line must fit one workgroup's LDS)."""
    if t.ndim != 2:
        # the reference unpacks `w, l = demanded_output.shape` (src/algorithms.py:20)
        raise ValueError(f"too many values to unpack (expected 2): target has shape {t.shape}")
    h, w = t.shape
    if h < 1 or w < 1:
        raise ValueError(f"empty target of shape {t.shape}")
    for n in (h, w):
        if not _side_supported(n):
            raise ValueError(f"unsupported target shape {t.shape}: a side over 4096 with a prime factor above 13, "
                             f"or any side over 8192, does not fit the GPU transforms (side {n})")
    return h, w


def target_for_device(demanded_output) -> tuple[np.ndarray, int]:
    """uint8 targets keep numpy's float16 amplitude rule (sqrt(uint8) -> float16,
    src/algorithms.py:21); everything else is carried as float32."""
    t = np.asarray(demanded_output)
    if t.dtype == np.uint8:
        return np.ascontiguousarray(t), TGT_U8
    return np.ascontiguousarray(t, dtype=np.float32), TGT_F32


def _needs_exact_stats(t) -> bool:
    """True for target dtypes that float32 does not hold exactly (float64, wide integers)."""
    return not (t.dtype in (np.uint8, np.float32, np.float16) or (t.dtype.kind in "iu" and t.dtype.itemsize <= 2))


def _exact_target_stats(plan, t):
    """A target that float32 does not hold exactly (float64, wide integers)
    keeps norm = np.amax(T) (src/algorithms.py:23) and sum T^2 (error_f's
    constant term, :161-162) in float64; the cross term sum E*T uses the
    float32 device copy (relative effect <= 2^-24 per pixel)."""
    if not _needs_exact_stats(t):
        return
    tf = t.astype(np.float64).reshape(plan.batch, -1)
    plan.set_target_stats(tf.max(axis=1), np.einsum("ij,ij->i", tf, tf))


def incoming_amplitude(args, shape) -> np.ndarray | None:
    """sqrt of the incoming intensity (src/algorithms.py:14-19); None = uniform."""
    if args.incomming_intensity == "uniform":
        return None
    from PIL import Image

    intensity = np.array(Image.open(args.incomming_intensity))
    amp = np.sqrt(intensity)
    if amp.shape != tuple(shape):
        raise ValueError(f"operands could not be broadcast together with shapes {amp.shape} {tuple(shape)}")
    return np.ascontiguousarray(amp, dtype=np.float32)


def random_unit_draws(seed, count):
    """The stdlib ``random`` stream of src/algorithms.py:117 (random.seed(seed);
    random.random() ...): NumPy's legacy MT19937 seeded with init_by_array([seed])
    produces the same doubles."""
    return np.random.RandomState([seed]).random_sample(count)


def make_initial_guess(initial_guess_type, incomming_amplitude, demanded_output, seed):
    """Host-side initial guesses of src/algorithms.py:115-158. Returns a complex
    field, or None for "fourier" (computed on the GPU from the target)."""
    h, w = np.asarray(demanded_output).shape
    s = h * w
    if initial_guess_type == "random":
        return np.exp(1j * 2 * np.pi * random_unit_draws(seed, s)).reshape(h, w)
    if initial_guess_type == "old":
        u = random_unit_draws(seed, 2 * s).reshape(s, 2)
        return (np.sqrt(u[:, 0]) + 1j * np.sqrt(u[:, 1])).reshape(h, w)
    if initial_guess_type == "unnormed":
        u = random_unit_draws(seed, 2 * s).reshape(s, 2)
        return ((u[:, 0] + 1j * u[:, 1]).reshape(h, w) - 0.5) * 2
    if initial_guess_type == "zeros":
        return (np.exp(1j * 2 * np.pi * random_unit_draws(seed, s)) / 100).reshape(h, w)
    if initial_guess_type == "ones":
        return np.ones((h, w)) + 1j * np.zeros((h, w))
    if initial_guess_type == "fourier":
        return None
    raise ValueError("unknown type of initial guess")


def learning_rates(lr, max_loops, unsettle):
    """Per-iteration learning rate and the value left in args.learning_rate after
    k iterations (src/algorithms.py:103-104)."""
    rates = np.empty(max(max_loops, 0), dtype=np.float64)
    after = np.empty(max(max_loops, 0) + 1, dtype=np.float64)
    after[0] = lr
    for i in range(max_loops):
        rates[i] = lr
        if unsettle and (i + 1) % int(round(max_loops / (unsettle + 1))) == 0:
            lr *= 2
        after[i + 1] = lr
    return rates, after


# ---------------------------------------------------------------------------
# plan cache
# ---------------------------------------------------------------------------
_PLANS: "collections.OrderedDict[tuple, _lib.Plan]" = collections.OrderedDict()
_MAX_PLANS = int(os.environ.get("SLM_PLAN_CACHE", "4"))


def get_plan(algo, batch, h, w, tgt_type, has_ain, max_loops) -> _lib.Plan:
    key = (algo, batch, h, w, tgt_type, bool(has_ain), max_loops)
    plan = _PLANS.pop(key, None)
    if plan is None:
        while len(_PLANS) >= _MAX_PLANS:
            _PLANS.popitem(last=False)[1].close()
        plan = _lib.Plan(algo, batch, h, w, tgt_type, has_ain, max_loops)
    _PLANS[key] = plan
    return plan


def clear_plans():
    while _PLANS:
        _PLANS.popitem()[1].close()
    _lib.release_caches()  # slm_fft2_c128's per-shape engines (move_traps.update_hologram)


# ---------------------------------------------------------------------------
# batch engine
# ---------------------------------------------------------------------------
def _stop_index(err, tol):
    """first iteration i with not (err_i > tol); None if every test passed."""
    bad = ~(np.asarray(err) > tol)
    return int(np.argmax(bad)) if bad.any() else None


def _run(plan, loops, tol, *white_attention):
    """Run a prepared plan and read it back: (phase, e, stats, iters, checked).
    tol > 0 runs with device checks. Any other run is speculative and
    unchecked: "while error > tolerance" is rechecked on the host, and a
    hologram that should have stopped early is rerun with device checks."""
    checked = tol > 0
    plan.run(loops, tol, checked, *white_attention)
    phase, e, stats, iters = plan.read()
    if not checked and any(_stop_index(stats[k, :loops, 3], tol) not in (None, loops - 1)
                           for k in range(plan.batch)):
        plan.run(loops, tol, True, *white_attention)
        phase, e, stats, iters = plan.read()
        checked = True
    return phase, e, stats, iters, checked


def _errors(stats, iters, loops, checked):
    """Statistics to results: per hologram the errors of the iterations it
    ran (iters[k] of them where a checked run stopped it, else all `loops`) and
    the max E of the last of them, which scales expected_outcome."""
    errs, maxes = [], []
    for k in range(len(iters)):
        n = int(iters[k]) if checked and iters[k] >= 0 else loops
        errs.append([np.float64(v) for v in stats[k, :n, 3]])
        maxes.append(stats[k, n - 1, 0])
    return errs, np.array(maxes)


def _collect(plan, loops, run):
    """run_gs's return values from _run's; the norm is the one the plan holds."""
    phase, e, stats, iters, checked = run
    errs, maxes = _errors(stats, iters, loops, checked)
    return phase, e, errs, plan.target_stats()[0], maxes


def run_gs(targets, loops, tol=0.0, ain=None, initial_phase=None):
    """GS on a batch [B][H][W] (uint8 or float). Returns phase float32 [B][H][W],
    |C|^2 float32 [B][H][W], errors list per hologram, norm [B], max E used
    for expected_outcome [B]."""
    t = np.asarray(targets)
    tdev, tt = target_for_device(t)
    b, h, w = tdev.shape
    plan = get_plan(ALGO_GS, b, h, w, tt, ain is not None, loops)
    plan.set_target(tdev)
    _exact_target_stats(plan, t)
    if ain is not None:
        plan.set_ain(ain)
    plan.set_phase(initial_phase)
    return _collect(plan, loops, _run(plan, loops, tol))


_FUSED_ONLY = ("{} runs on the fused engine only: both sides of the target must be one of "
               "64, 128, 256, 512, 1024, 2048, 4096 (powers of two) or 768, and $SLM_ENGINE=float64 must not be set")
_GSW, _MRAF = "weighted Gerchberg-Saxton", "MRAF"
GSW_SHAPES, MRAF_SHAPES = _FUSED_ONLY.format(_GSW), _FUSED_ONLY.format(_MRAF)


def _fused_only(name, h, w, unsupported=None):
    """Weighted GS and MRAF (`name`) are built into the fused engine's column
    pass; the any-size engines (other sides, $SLM_ENGINE=float64) refuse them.
    Checked before any device call; `unsupported` is the engine's own refusal,
    which is reported as the same error."""
    if (unsupported is not None or h not in _lib.SUPPORTED_LENGTHS or w not in _lib.SUPPORTED_LENGTHS
            or os.environ.get("SLM_ENGINE") == "float64"):
        raise ValueError(f"{_FUSED_ONLY.format(name)} (got {h} x {w})") from unsupported


def _fused_plan(name, algo, b, h, w, tt, has_ain, loops):
    """get_plan for an algorithm that only the fused engine runs."""
    try:
        return get_plan(algo, b, h, w, tt, has_ain, loops)
    except _lib.SlmError as e:
        if e.code == _lib.ERR_UNSUPPORTED:
            _fused_only(name, h, w, e)
        raise


def run_gsw(targets, loops, feedback=1.0, tol=0.0, ain=None, initial_phase=None, initial_weights=None,
            return_weights=False):
    """Weighted GS (no reference counterpart; include/slm_hip.h) on a batch
    [B][H][W]: run_gs's arguments and return values, the feedback exponent p of
    g *= (a_T / |C|)^p, optional initial weights [B][H][W] and, with
    return_weights, the weights after the run (mean 1 over the support T > 0,
    1 off it) appended to the result."""
    t = np.asarray(targets)
    tdev, tt = target_for_device(t)
    b, h, w = tdev.shape
    _fused_only(_GSW, h, w)
    feedback = float(feedback)
    if not (np.isfinite(feedback) and feedback >= 0):
        raise ValueError(f"feedback must be a finite number >= 0, got {feedback}")
    plan = _fused_plan(_GSW, ALGO_GSW, b, h, w, tt, ain is not None, loops)
    plan.set_target(tdev)
    _exact_target_stats(plan, t)
    if ain is not None:
        plan.set_ain(ain)
    plan.set_feedback(feedback)
    plan.set_phase(initial_phase)
    try:
        plan.set_weights(initial_weights)
    except _lib.SlmError as e:
        if e.code == _lib.ERR_ARG:
            raise ValueError("initial weights must be positive and finite wherever the target is > 0") from e
        raise
    out = _collect(plan, loops, _run(plan, loops, tol))
    return out + (plan.read_weights(),) if return_weights else out


def signal_region(target, margin=8):
    """The default MRAF signal region: the support T > 0 dilated by a square
    of `margin` pixels each way, clipped at the edges (no wrap). uint8, 1 =
    signal; the last two axes are the image."""
    margin = int(margin)
    if margin < 0:
        raise ValueError(f"region margin must be >= 0, got {margin}")
    sup = np.asarray(target) > 0
    h, w = sup.shape[-2:]
    rows = np.zeros_like(sup)
    for d in range(-min(margin, h - 1), min(margin, h - 1) + 1):
        rows[..., max(d, 0):h + min(d, 0), :] |= sup[..., max(-d, 0):h - max(d, 0), :]
    out = np.zeros_like(sup)
    for d in range(-min(margin, w - 1), min(margin, w - 1) + 1):
        out[..., max(d, 0):w + min(d, 0)] |= rows[..., max(-d, 0):w - max(d, 0)]
    return out.astype(np.uint8)


def _check_mixing(mixing):
    if not (np.isfinite(mixing) and 0 < mixing <= 1):
        raise ValueError(f"mixing must be in (0, 1], got {mixing}")


def _check_support(sr, tdev, where=""):
    """Every hologram of a batch (sr and tdev are [B][H][W]) needs a target
    pixel inside its signal region; `where` names the batch in the message."""
    for k in range(len(tdev)):
        if not np.any(sr[k] & (tdev[k] > 0)):
            raise ValueError(f"{where}the signal region of hologram {k} holds no pixel with T > 0")


def run_mraf(targets, regions, loops, mixing=0.4, tol=0.0, ain=None, initial_phase=None, return_efficiency=False):
    """MRAF, mixed-region amplitude freedom (no reference counterpart;
    include/slm_hip.h), on a batch [B][H][W]: GS whose amplitude constraint
    m kappa a_T holds on the signal region `regions` != 0 only, (1 - m) C being
    kept elsewhere. run_gs's return values, with the error, norm and max E
    taken over the region; with return_efficiency the efficiency sum_sr E / P
    per iteration (a list per hologram, as the errors) is appended. T outside
    the region is ignored, except by the cold start, which is GS's own."""
    t = np.asarray(targets)
    tdev, tt = target_for_device(t)
    if tdev.ndim != 3:
        raise ValueError(f"targets must be [B][H][W], got shape {tdev.shape}")
    b, h, w = tdev.shape
    _fused_only(_MRAF, h, w)
    mixing = float(mixing)
    _check_mixing(mixing)
    r = np.asarray(regions)
    if r.shape != tdev.shape:
        raise ValueError(f"regions of shape {r.shape} do not match targets of shape {tdev.shape}")
    sr = r != 0
    _check_support(sr, tdev)
    if ain is not None and np.asarray(ain).shape != (h, w):
        raise ValueError(f"ain of shape {np.asarray(ain).shape} does not match {(h, w)}")
    if initial_phase is not None and np.asarray(initial_phase).shape != tdev.shape:
        raise ValueError(f"initial_phase of shape {np.asarray(initial_phase).shape} does not match {tdev.shape}")
    plan = _fused_plan(_MRAF, ALGO_MRAF, b, h, w, tt, ain is not None, loops)
    plan.set_target(tdev)
    plan.set_region(sr)
    if ain is not None:
        plan.set_ain(ain)
    plan.set_mixing(mixing)
    plan.set_phase(initial_phase)
    phase, e, stats, iters, checked = _run(plan, loops, tol)
    eff = plan.read_efficiency()
    errs, maxes = _errors(stats, iters, loops, checked)
    norm = np.array([np.float64(tdev[k][sr[k]].max()) for k in range(b)])
    out = phase, e, errs, norm, maxes
    if return_efficiency:
        out += ([[np.float64(v) for v in eff[k, :len(errs[k])]] for k in range(b)],)
    return out


SEQUENCE_ALGORITHMS = {"gerchberg_saxton": ALGO_GS, "weighted_gerchberg_saxton": ALGO_GSW, "mraf": ALGO_MRAF}


def _sequence_inputs(targets, loops_first, loops, algorithm, tol, ain, initial_phase, feedback, mixing, regions,
                     mask):
    """run_sequence's argument checks (host only): the device targets
    [F][B][H][W], their type, the algorithm code and the regions as 0 / 1."""
    if algorithm not in SEQUENCE_ALGORITHMS:
        raise ValueError(f"unknown sequence algorithm {algorithm!r}: one of {sorted(SEQUENCE_ALGORITHMS)}")
    algo = SEQUENCE_ALGORITHMS[algorithm]
    tdev, tt = target_for_device(targets)
    if tdev.ndim == 3:
        tdev = tdev[:, None]
    if tdev.ndim != 4 or tdev.shape[0] < 1 or tdev.shape[1] < 1:
        raise ValueError(f"targets must be [F][H][W] or [F][B][H][W] with at least one frame, got shape "
                         f"{np.asarray(targets).shape}")
    f, b, h, w = tdev.shape
    _check_shape(tdev[0, 0])
    for name, n in (("loops_first", loops_first), ("loops", loops)):
        if int(n) != n or n < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {n}")
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError(f"tol must be finite and >= 0, got {tol}")
    if algo == ALGO_GSW:
        _fused_only(_GSW, h, w)
        if not (np.isfinite(feedback) and feedback >= 0):
            raise ValueError(f"feedback must be a finite number >= 0, got {feedback}")
    sr = None
    if algo == ALGO_MRAF:
        _fused_only(_MRAF, h, w)
        _check_mixing(mixing)
        if regions is None:
            raise ValueError("an MRAF sequence needs the signal regions of its frames")
        sr = np.asarray(regions) != 0
        if sr.ndim == 3:
            sr = sr[:, None]
        if sr.shape != tdev.shape:
            raise ValueError(f"regions of shape {np.asarray(regions).shape} do not match targets of shape "
                             f"{np.asarray(targets).shape}")
        for i in range(f):
            _check_support(sr[i], tdev[i], f"frame {i}: ")
    elif regions is not None:
        raise ValueError("regions apply to algorithm 'mraf' only")
    if ain is not None and np.asarray(ain).shape != (h, w):
        raise ValueError(f"ain of shape {np.asarray(ain).shape} does not match {(h, w)}")
    if initial_phase is not None and np.asarray(initial_phase).size != b * h * w:
        raise ValueError(f"initial_phase of shape {np.asarray(initial_phase).shape} does not match {(b, h, w)}")
    if mask is not None and np.asarray(mask).shape != (h, w):
        raise ValueError(f"mask of shape {np.asarray(mask).shape} does not match {(h, w)}")
    return tdev, tt, algo, sr


def run_sequence(targets, loops_first, loops, algorithm="gerchberg_saxton", tol=0.0, ain=None, initial_phase=None,
                 feedback=1.0, mixing=0.4, regions=None, mask=None, ct2pi=256, rule=_lib.QUANT_PIL,
                 return_expected=False):
    """A sequence of image targets [F][H][W] or [F][B][H][W] (moving traps drawn
    as pictures) as one device-resident chain (slm_plan_sequence): frame 0
    starts from initial_phase or cold and runs loops_first iterations, every
    later frame starts from the phase of the frame before it and runs loops;
    tol > 0 stops a frame on the device. algorithm is "gerchberg_saxton",
    "weighted_gerchberg_saxton" (feedback) or "mraf" (mixing, regions of the
    targets' shape). Returns phases float32 [F][B][H][W], the quantised uint8
    frames [F][B][H][W] (slm_quantize's mask, ct2pi and rule), the errors as a
    list per frame of a list per hologram, norm [F][B] and the max E used for
    expected_outcome [F][B]; with return_expected |C|^2 float32 [F][B][H][W] is
    appended. Targets other than uint8 are carried as float32, with norm and the
    error's constant term taken from that copy."""
    tdev, tt, algo, sr = _sequence_inputs(targets, loops_first, loops, algorithm, tol, ain, initial_phase, feedback,
                                          mixing, regions, mask)
    f, b, h, w = tdev.shape
    loops_first, loops = int(loops_first), int(loops)
    plan = get_plan(algo, b, h, w, tt, ain is not None, max(loops_first, loops))
    if ain is not None:
        plan.set_ain(ain)
    if algo == ALGO_GSW:
        plan.set_feedback(float(feedback))
    if algo == ALGO_MRAF:
        plan.set_mixing(float(mixing))
    plan.set_phase(initial_phase)
    plan.sequence(tdev, sr, loops_first=loops_first, loops=loops, tol=tol, mask=mask, ct2pi=ct2pi, rule=rule,
                  frames=True, phases=True, expected=return_expected)
    frames, phases, e, stats, _, iters = plan.sequence_read(frames=True, phases=True, expected=return_expected)
    errs, maxes = [], []
    for i in range(f):
        frame_errs, frame_maxes = _errors(stats[i], iters[i], loops if i else loops_first, tol > 0)
        errs.append(frame_errs)
        maxes.append(frame_maxes)
    if sr is None:
        norm = tdev.reshape(f, b, -1).max(axis=2).astype(np.float64)
    else:
        norm = np.where(sr, tdev, 0).reshape(f, b, -1).max(axis=2).astype(np.float64)
    out = phases, frames, errs, norm, np.array(maxes)
    return out + (e,) if return_expected else out


def run_gs_multi(targets, loops, devices, tol=0.0, ain=None, feedback=None):
    """run_gs's contract over several GPUs from this one process
    (slm_gs_multi: contiguous shards, one host thread / plan per device).
    With a feedback exponent the shards run weighted GS (run_gsw's contract,
    slm_gsw_multi).
    slm_gs_multi takes the error's constant terms from its float32 copy of the
    target, so frames that float32 does not hold exactly (float64, wide
    integers) go through run_gs, which keeps them in float64 (the two paths
    then report the same error_evolution)."""
    t = np.asarray(targets)
    if _needs_exact_stats(t):
        if len(set(int(d) for d in devices)) > 1:
            warnings.warn(f"{t.dtype} targets are not exact in float32: the batch runs on this process's one "
                          f"GPU (run_gs) so the error keeps its float64 terms; `devices` {list(devices)} is "
                          "ignored -- pass uint8 or float32 frames to shard them", RuntimeWarning, stacklevel=2)
        return run_gs(t, loops, tol, ain) if feedback is None else run_gsw(t, loops, feedback, tol, ain)
    tdev, _ = target_for_device(t)
    if feedback is not None:
        _fused_only(_GSW, *tdev.shape[1:])
    phase, e, stats, iters = _lib.gs_multi(tdev, loops, devices, tol=tol, ain=ain, feedback=feedback)
    norm = t.reshape(t.shape[0], -1).max(axis=1).astype(np.float64)  # np.amax(demanded_output)
    errs, maxes = _errors(stats, iters, loops, True)  # the shards' iters count at every tolerance
    return phase, e, errs, norm, maxes


def run_gd(targets, loops, rates, white_attention, tol=0.0, ain=None, initial_field=None, return_field=False):
    t = np.asarray(targets)
    tdev, tt = target_for_device(t)
    b, h, w = tdev.shape
    plan = get_plan(ALGO_GD, b, h, w, tt, ain is not None, loops)
    plan.set_target(tdev)
    _exact_target_stats(plan, t)
    if ain is not None:
        plan.set_ain(ain)
    plan.set_field(initial_field)
    plan.set_lr(np.asarray(rates, np.float32)[:loops])
    out = _collect(plan, loops, _run(plan, loops, tol, white_attention))
    return out + (plan.read_field(),) if return_field else out


def hologram_from(phase):
    """float32 device phase -> float64 hologram in np.angle's range [-pi, pi]
    (float32(pi) rounds above pi; the clip moves such values by < 1e-7)."""
    return np.clip(phase.astype(np.float64), -np.pi, np.pi)


def expected_from(e, norm, emax):
    """expected_outcome = |C|^2 * norm / max|C|^2 in float64 (src/algorithms.py:36-37)."""
    out = e.astype(np.float64)
    out *= norm / np.float64(emax)
    return out


# ---------------------------------------------------------------------------
# reference-compatible entry points
# ---------------------------------------------------------------------------
def _print_loops(n, max_loops):
    sys.stdout.write("".join(f"\rloop {i}/{max_loops}" for i in range(1, n + 1)))
    print()


def printout(error, loop_num, error_evol, plot_error):
    """src/algorithms.py:165-172."""
    print(f"error: {error}")
    print(f"number of loops: {loop_num}")
    if plot_error:
        import matplotlib.pyplot as plt

        plt.plot(error_evol)
        plt.xlabel("loop number")
        plt.ylabel("error")
        plt.show()


def _iterations_allowed(args):
    # `while error > args.tolerance and i < args.max_loops` with error = tol + 1
    tol = args.tolerance
    return args.max_loops > 0 and (tol + 1) > tol


def _no_iterations(args, variable):
    """Where the reference's loop body never runs, its report and its failure
    on `variable`, which only the body assigns."""
    if _iterations_allowed(args):
        return
    print()
    if args.print_info:
        print()
        printout(args.tolerance + 1, 0, [], args.plot_error)
    raise UnboundLocalError(f"local variable '{variable}' referenced before assignment")


def _chunks(args, chunk, kind="gs"):
    """The iterations of an entry point: (phase, expected outcome, errors).
    chunk(n, at, last) runs n iterations from iteration `at` and returns its
    run_*'s result; `last` is the result of the chunk before, which holds the
    state to continue from, or None at the start. A plain run is one chunk. GIF
    frames need intermediate states: a GIF run goes in warm-started chunks
    that end on every frame iteration."""
    loops, tol = args.max_loops, args.tolerance
    error_evolution, out, i = [], None, 0
    while i < loops:
        if not args.gif:
            n = loops
        else:
            n = 1 if i % args.gif_skip == 0 else min(args.gif_skip - i % args.gif_skip, loops - i)
        out = chunk(n, i, out)
        phase, e, errs, norm, emax = out[:5]
        error_evolution += errs[0]
        i += len(errs[0])
        expected = expected_from(e[0], norm[0], emax[0])
        if args.gif and (i - 1) % args.gif_skip == 0:
            _gif_frame(args, kind, (out[5] if kind == "gd" else phase)[0], expected, i - 1)
        if len(errs[0]) < n or not (error_evolution[-1] > tol):
            break
    return phase, expected, error_evolution


def _report(args, phase, expected, error_evolution):
    """The reference's lines after its loop, and its return triple."""
    n = len(error_evolution)
    _print_loops(n, args.max_loops)
    if args.print_info:
        print()
        printout(error_evolution[-1], n, error_evolution, args.plot_error)
    return hologram_from(phase[0]), expected, error_evolution


def _gif_frame(args, kind, phase, expected, i):
    """add_gif_image (src/algorithms.py:52-57) for GS; the GD frame of
    src/algorithms.py:94-101 (complex_to_real_phase of x/|x|, :175-176) when
    `phase` is the GD field."""
    from PIL import Image

    if args.gif_type == "h":
        if kind == "gd":
            ang = np.angle(phase.astype(np.complex128))
        else:
            ang = hologram_from(phase)
        img = Image.fromarray((ang + np.pi) * args.correspond_to2pi / (2 * np.pi)
                              if kind == "gs" else (ang + np.pi) / (2 * np.pi) * args.correspond_to2pi)
    elif args.gif_type == "i":
        img = Image.fromarray(expected)
    else:
        return
    img.convert("L").save(f"{args.gif_source_dir}/{i // args.gif_skip}.png")


def gerchberg_saxton(demanded_output, args):
    """Classical Gerchberg-Saxton (far field) on the GPU; drop-in for
    src/algorithms.py:10-49."""
    t = np.asarray(demanded_output)
    _check_shape(t)
    ain = incoming_amplitude(args, t.shape)
    tol = args.tolerance
    _no_iterations(args, "expected_outcome")

    def chunk(n, at, last):  # the GS state is angle(A) only
        return run_gs(t[None], n, tol, ain, initial_phase=None if last is None else last[0])

    return _report(args, *_chunks(args, chunk))


def weighted_gerchberg_saxton(demanded_output, args):
    """Weighted Gerchberg-Saxton (far field) on the GPU: GS with a per-pixel
    weight feedback g *= (a_T / |C|)^p on the target's support, which evens out
    the trap intensities plain GS leaves unequal. No reference counterpart;
    the return triple, the printed lines and the exceptions are
    gerchberg_saxton's. Reads ``args.feedback`` (the exponent p, default 1)."""
    t = np.asarray(demanded_output)
    h, w = _check_shape(t)
    _fused_only(_GSW, h, w)
    feedback = float(getattr(args, "feedback", 1.0))
    ain = incoming_amplitude(args, t.shape)
    tol = args.tolerance
    _no_iterations(args, "expected_outcome")

    def chunk(n, at, last):  # a GIF run hands the weights on as well as the phase
        phase, weights = (None, None) if last is None else (last[0], last[5])
        return run_gsw(t[None], n, feedback, tol, ain, phase, weights, return_weights=args.gif)

    return _report(args, *_chunks(args, chunk))


def mraf(demanded_output, args):
    """MRAF (mixed-region amplitude freedom, Pasienski and DeMarco 2008) on the
    GPU, for extended flat shapes, on which GS ends in speckle: the amplitude
    is imposed on a signal region around the pattern only and left free
    elsewhere. No reference counterpart; the return triple, the printed lines
    and the exceptions are gerchberg_saxton's, with the error and the expected
    outcome's scale taken over the region. Reads ``args.mixing`` (m, default
    0.4), ``args.signal_region`` (an array, nonzero = signal, or None) and, with
    None, ``args.region_margin`` (default 8): the region is then
    signal_region(target, margin)."""
    t = np.asarray(demanded_output)
    _check_shape(t)
    mixing = float(getattr(args, "mixing", 0.4))
    region = getattr(args, "signal_region", None)
    if region is None:
        region = signal_region(t, getattr(args, "region_margin", 8))
    region = np.asarray(region)
    if region.shape != t.shape:
        raise ValueError(f"signal region of shape {region.shape} does not match the target's {t.shape}")
    ain = incoming_amplitude(args, t.shape)
    tol = args.tolerance
    _no_iterations(args, "expected_outcome")

    def chunk(n, at, last):  # the MRAF state is angle(A) only, as GS's
        return run_mraf(t[None], region[None], n, mixing, tol, ain, initial_phase=None if last is None else last[0])

    return _report(args, *_chunks(args, chunk))


def gradient_descent(demanded_output, args):
    """Gradient descent on the unconstrained complex field (far field) on the
    GPU; drop-in for src/algorithms.py:60-112."""
    t = np.asarray(demanded_output)
    _check_shape(t)
    ain = incoming_amplitude(args, t.shape)
    amp_host = np.ones(t.shape) if ain is None else ain.astype(np.float64)
    field = make_initial_guess(args.initial_guess, amp_host, t, args.random_seed)
    tol = args.tolerance
    if args.print_info:
        print("computing hologram")
    _no_iterations(args, "output")
    if args.unsettle and int(round(args.max_loops / (args.unsettle + 1))) == 0:
        raise ZeroDivisionError("integer division or modulo by zero")
    rates, after = learning_rates(args.learning_rate, args.max_loops, args.unsettle)
    x0 = None if field is None else field[None]

    def chunk(n, at, last):
        """The GD state is the complex field x, read back after each chunk of a
        GIF run (slm_plan_read_field) and handed to the next with the matching
        slice of the learning-rate schedule."""
        return run_gd(t[None], n, rates[at:at + n], float(args.white_attention), tol, ain,
                      x0 if last is None else last[5], return_field=args.gif)

    phase, output, error_evolution = _chunks(args, chunk, "gd")
    args.learning_rate = float(after[len(error_evolution)]) if args.unsettle else args.learning_rate
    return _report(args, phase, output, error_evolution)
