"""Trap holograms for the optical-tweezers loop, drop-in for the compute of
src/move_traps.py (the keyboard / Tk window plumbing around it is out of scope,
DESIGN.md section 7).

* ``update_hologram(black_image, coords, which)`` — src/move_traps.py:64-68:
  the phase of ``ifft2`` of a blank image with one 255-valued pixel, float64,
  computed on the GPU by slm_trap_frames (closed form of the single-pixel
  inverse DFT, exact integer phase index; no transform needed); an image that
  already holds traps takes the float64 device transform (slm_fft2_c128).
* ``hologram_frame(hologram, mask, mask_flag, ct2pi)`` — the quantisation of
  display_hologram, src/move_traps.py:135-139, as the uint8 frame handed to the
  SLM window.
* ``trap_frame(shape, coords, which, mask, mask_flag, ct2pi)`` — both fused in
  one launch: what a key press of the trap-moving loop costs.
* ``trap_array_hologram`` / ``trap_array_frame`` — no reference counterpart:
  the hologram of a whole list of traps (fractional positions, a defocus per
  trap, uniform or chosen intensities) by spot-based weighted GS on the GPU
  (slm_spots_*), on any panel shape.
* ``trap_array_sequence`` — no reference counterpart either: a whole
  trajectory of such a list (F frames of the same M traps, moved) as one chain
  on the device (slm_spots_sequence). Each frame starts from the previous
  frame's field and weights, may stop once its uniformity meets a tolerance,
  and leaves the device as the uint8 SLM frame. The reference's route to moving
  traps (generate_traps_image_sequence.py, then GS per rasterised frame) rounds
  the positions to whole pixels; this one keeps them fractional.
* ``trap_window`` / ``expected_outcome`` — no reference counterpart: the far
  field a hologram, or the uint8 frame sent to the panel, produces around a set
  of trap positions, sampled between the FFT bins in a chosen focal plane
  (slm_farfield_zoom). What show_expected_outcome's |fft2|^2 cannot show of a
  trap at a fractional position.
* ``trap_windows`` / ``trap_array_sequence(expected=...)`` — the same preview
  for every frame of a trajectory, from the uint8 frames where the sequence
  left them on the device (the resident zoom, slm_zoom_*): one window for the
  trajectory or one per frame that follows the traps, the sequence's
  correction mask taken off if asked.
"""
from __future__ import annotations

import collections

import numpy as np

from . import _lib
from . import constants


def _trap_index(black_image: np.ndarray, coords, which):
    h, w = black_image.shape
    y, x = int(coords[which][0]), int(coords[which][1])
    if not (-h <= y < h and -w <= x < w):  # numpy indexing rules of black_image[y][x]
        raise IndexError(f"index ({y}, {x}) is out of bounds for an image of shape {(h, w)}")
    return y % h, x % w


def update_hologram(black_image: np.ndarray, coords, which) -> np.ndarray:
    """src/move_traps.py:64-68: angle(ifft2(image with the trap pixel at 255)),
    float64; the pixel under the trap is left at 0 afterwards, as the reference
    leaves it. A blank image (the reference's loop, src/move_traps.py:16) takes
    the closed form (slm_trap_frames, exact phase index). Any other image runs
    the device's float64 inverse 2-D transform (slm_fft2_c128), as the
    reference's float64 ifft2 does (tests/test_frames.py)."""
    black_image = np.asarray(black_image)
    if black_image.ndim != 2:
        raise ValueError("black_image must be a 2-D image")
    y, x = _trap_index(black_image, coords, which)
    if not np.count_nonzero(black_image):
        phase, _ = _lib.trap_frames(black_image.shape, [y], [x], frame=False)
        black_image[y][x] = 0
        return phase[0]
    black_image[y][x] = 255
    # float64 on the device, as the reference's ifft2 of the float64 image (unscaled:
    # the 1/(h w) leaves angles alone)
    field = _lib.fft2_c128(black_image.astype(np.complex128), inverse=True)
    black_image[y][x] = 0
    return np.angle(field)


def hologram_frame(hologram: np.ndarray, mask, mask_flag: bool, ct2pi) -> np.ndarray:
    """uint8 SLM levels of display_hologram (src/move_traps.py:135-139):
    ((hologram [+ mask]) % 2pi * ct2pi / 2pi).astype(uint8)."""
    return _lib.quantize(np.asarray(hologram, dtype=np.float64), mask if mask_flag else None, ct2pi,
                         _lib.QUANT_ASTYPE)


# ---------------------------------------------------------------------------
# trap lists: the multi-trap counterpart of update_hologram (no reference
# counterpart; slm_spots_* in include/slm_hip.h)
# ---------------------------------------------------------------------------
_SPOTS: "collections.OrderedDict[tuple, _lib.Spots]" = collections.OrderedDict()
_MAX_SPOTS = 4


def _get_spots(batch, h, w, n_traps, has_ain, loops) -> _lib.Spots:
    """Spots handles are cached per (B, H, W, max_traps, has_ain), max_traps
    being the trap count rounded up to a multiple of 32."""
    max_traps = min(_lib.SPOTS_MAX_TRAPS, -(-n_traps // 32) * 32)
    key = (batch, h, w, max(max_traps, n_traps), bool(has_ain))
    sp = _SPOTS.pop(key, None)
    if sp is not None and sp.max_loops < loops:
        sp.close()
        sp = None
    if sp is None:
        while len(_SPOTS) >= _MAX_SPOTS:
            _SPOTS.popitem(last=False)[1].close()
        sp = _lib.Spots(batch, h, w, key[3], has_ain, max(loops, 64))
    _SPOTS[key] = sp
    return sp


def clear_spots() -> None:
    """Closes the cached Spots handles, and the zoom handles that preview their frames."""
    while _ZOOMS:
        _ZOOMS.popitem()[1].close()
    while _SPOTS:
        _SPOTS.popitem()[1].close()


# resident zoom handles of trap_array_sequence(expected=...), per (frames per run, H, W)
_ZOOMS: "collections.OrderedDict[tuple, _lib.Zoom]" = collections.OrderedDict()
_MAX_ZOOMS = 2


def _get_zoom(count, h, w, size) -> _lib.Zoom:
    key = (count, h, w)
    zm = _ZOOMS.pop(key, None)
    if zm is not None and (zm.max_size[0] < size[0] or zm.max_size[1] < size[1]):
        zm.close()
        zm = None
    if zm is None:
        while len(_ZOOMS) >= _MAX_ZOOMS:
            _ZOOMS.popitem(last=False)[1].close()
        zm = _lib.Zoom(count, h, w, size)
    _ZOOMS[key] = zm
    return zm


def lens_to_z(focal_length: float) -> float:
    """The defocus z (radians per pixel^2) of a lens of this focal length in
    metres: the paraxial form of generate_hologram.lens(),
    -pi px_distance^2 / (wavelength f)."""
    return -np.pi * constants.px_distance ** 2 / (constants.wavelength * float(focal_length))


def trap_array_hologram(shape, ys, xs, zs=None, intensity=None, loops=30, feedback=1.0, ain=None,
                        initial_phase=None, initial_weights=None):
    """Weighted GS on a list of traps (spot form, slm_spots_*): positions ys, xs
    in far-field pixels (fractions and negative values allowed), defocus zs in
    radians per pixel^2 (lens_to_z), target intensities. One list [M], or a
    batch [B][M] of lists for B holograms. Returns (hologram float64 as
    update_hologram's, per-trap intensities |V_m|^2 of the last iteration, the
    statistics [loops][4] = (efficiency, uniformity, min, max of the
    normalised intensities) and the weights); with a batch input every result
    has the leading axis B."""
    h, w = int(shape[0]), int(shape[1])
    y = np.asarray(ys, dtype=np.float64)
    single = y.ndim < 2
    y = np.atleast_2d(y)
    b, m = y.shape

    def per_trap(v, name):
        if v is None:
            return None
        v = np.atleast_2d(np.asarray(v, dtype=np.float64))
        if v.shape != (b, m):
            raise ValueError(f"{name} has shape {v.shape}, the trap lists {(b, m)}")
        return v

    sp = _get_spots(b, h, w, m, ain is not None, int(loops))
    sp.set_traps(y, per_trap(xs, "xs"), per_trap(zs, "zs"), per_trap(intensity, "intensity"))
    if ain is not None:
        sp.set_ain(ain)
    sp.set_feedback(feedback)
    sp.set_phase(None if initial_phase is None else np.asarray(initial_phase).reshape(b, h, w))
    sp.set_weights(None if initial_weights is None else per_trap(initial_weights, "initial_weights"))
    sp.run(int(loops))
    phase, v, stats, weights = sp.read()
    holo, inten = phase.astype(np.float64), v.real ** 2 + v.imag ** 2
    if single:
        return holo[0], inten[0], stats[0], weights[0]
    return holo, inten, stats, weights


def trap_array_frame(shape, ys, xs, zs=None, intensity=None, loops=30, feedback=1.0, ain=None, initial_phase=None,
                     initial_weights=None, mask=None, mask_flag: bool = True, ct2pi=256):
    """trap_array_hologram plus hologram_frame's quantisation: returns
    (hologram, frame uint8, intensities, statistics, weights)."""
    holo, inten, stats, weights = trap_array_hologram(shape, ys, xs, zs, intensity, loops, feedback, ain,
                                                      initial_phase, initial_weights)
    frame = hologram_frame(holo, mask, mask_flag and mask is not None, ct2pi)
    return holo, frame, inten, stats, weights


SequenceResult = collections.namedtuple("SequenceResult", "frames holograms intensities stats iters weights expected",
                                        defaults=(None,))
SequenceResult.__doc__ = """What trap_array_sequence returns, every field with a leading [F] (one
trajectory) or [F][B] (a batch): frames uint8 [H][W], holograms float64 [H][W]
or None, intensities |V_m|^2 [M], stats [max(loops_first, loops)][4] (rows past
iters are 0), iters (iterations each frame ran), weights [M], expected float32
[ny][nx] (the zoomed far field of each frame) or None."""


def _expected_options(expected, ys, xs):
    """trap_array_sequence's expected=dict(...) as (origins [F][2] or one (y0, x0),
    pitch, size, z, mask_off); ValueError on anything it cannot take."""
    if not isinstance(expected, dict):
        raise ValueError(f"expected is a dict of margin, oversample, z, follow and mask_off, got {expected!r}")
    unknown = set(expected) - {"margin", "oversample", "z", "follow", "mask_off"}
    if unknown:
        raise ValueError(f"expected has unknown keys {sorted(unknown)}")
    z = float(expected.get("z", 0.0))
    if not np.isfinite(z):
        raise ValueError(f"expected: z must be finite, got {z}")
    margin, oversample = expected.get("margin", 4.0), expected.get("oversample", 8)
    if expected.get("follow", False):
        origins, pitch, size = trap_windows(ys.reshape(ys.shape[0], -1), xs.reshape(xs.shape[0], -1), margin,
                                            oversample)
    else:
        origins, pitch, size = trap_window(ys, xs, margin, oversample)
    return origins, pitch, size, z, bool(expected.get("mask_off", False))


def _expected_from_device(sp, b, h, w, f, options, ain, mask, ct2pi):
    """The zoomed far field [F][B][ny][nx] of the frames the sequence left on the
    device, through a cached resident zoom handle: at most 1024 frames per run,
    a per-frame window (the same for a frame's B holograms) when following."""
    origins, pitch, size, z, mask_off = options
    total = f * b
    per_run = min(total, _lib.ZOOM_MAX_BATCH)
    zm = _get_zoom(per_run, h, w, size)
    zm.set_ain(ain)
    zm.set_mask(mask if mask_off else None)
    follow = np.ndim(origins) == 2
    if not follow:
        zm.set_window(origins, pitch, size, z)
    out = np.empty((total,) + tuple(size), np.float32)
    for first in range(0, total, per_run):
        count = min(per_run, total - first)
        if follow:
            o = np.repeat(np.asarray(origins, np.float64), b, axis=0)[first:first + count]
            zm.set_window(np.concatenate([o, np.repeat(o[-1:], per_run - count, axis=0)]), pitch, size, z)
        zm.run_spots(sp, first, count, ct2pi)
        out[first:first + count] = zm.read()
    return out.reshape((f, b) + tuple(size))


def _sequence_arrays(ys, xs, zs, intensity, initial_weights):
    """The trajectory as [F][B][M] arrays (None where not given), and whether
    it was one trajectory [F][M]; ValueError on any shape mismatch."""
    y = np.asarray(ys, dtype=np.float64)
    if y.ndim not in (2, 3) or y.size == 0:
        raise ValueError(f"ys has shape {y.shape}: a trajectory is [F][M], a batch of them [F][B][M]")
    single = y.ndim == 2
    if single:
        y = y[:, None, :]

    def like(v, name, dtype=np.float64):
        if v is None:
            return None
        v = np.asarray(v, dtype=dtype)
        if single and v.ndim == 2:
            v = v[:, None, :]
        if v.shape != y.shape:
            raise ValueError(f"{name} has shape {np.shape(v)}, the trajectory {np.shape(ys)}")
        return v

    x = like(xs, "xs")
    if x is None:
        raise ValueError("xs is required")
    z, inten = like(zs, "zs"), like(intensity, "intensity")
    w0 = None
    if initial_weights is not None:
        w0 = np.atleast_2d(np.asarray(initial_weights, dtype=np.float64))
        if w0.shape != y.shape[1:]:
            raise ValueError(f"initial_weights has shape {w0.shape}, the trap lists {y.shape[1:]}")
    return y, x, z, inten, w0, single


def trap_array_sequence(shape, ys, xs, zs=None, intensity=None, loops_first=30, loops=4, tol=0.0, feedback=1.0,
                        ain=None, initial_phase=None, initial_weights=None, mask=None, mask_flag: bool = True,
                        ct2pi=256, holograms=False, resume=False, expected=None) -> SequenceResult:
    """A trajectory of a trap list as one chain on the device
    (slm_spots_sequence): ys, xs, zs, intensity are [F][M], or [F][B][M] for B
    trajectories at once; trap m of frame f is trap m of frame f-1, moved.
    Frame 0 runs at most loops_first iterations from initial_phase (or the
    default start) and initial_weights (or ones); every later frame at most
    `loops` from the field and weights the frame before ended with. With
    tol > 0 a frame ends with the first iteration whose incoming uniformity
    std(r) is <= tol. Each frame is quantised on the device as hologram_frame
    does. resume=True continues the last sequence of the cached handle for this
    shape and trap count: its frame 0 is an ordinary later frame, feedback and
    a_in stay the handle's, and initial_phase / initial_weights must be None.
    Returns a SequenceResult; holograms (float64, as update_hologram's) only
    with holograms=True. expected=dict(margin=4.0, oversample=8, z=0.0,
    follow=False, mask_off=False) adds result.expected, the zoomed far field of
    every uint8 frame (as expected_outcome gives it, bit for bit when no mask is
    taken off), computed from the frames where the sequence left them on the
    device: on the whole trajectory's trap_window, or with follow=True on each
    frame's own window of trap_windows (one common size); mask_off=True takes
    the sequence's own mask off again, so that the preview shows the traps and
    not the aberration the mask is there to cancel."""
    h, w = int(shape[0]), int(shape[1])
    y, x, z, inten, w0, single = _sequence_arrays(ys, xs, zs, intensity, initial_weights)
    f, b, m = y.shape
    options = None if expected is None else _expected_options(expected, y, x)
    if initial_phase is not None and np.size(initial_phase) != b * h * w:
        raise ValueError(f"initial_phase has {np.size(initial_phase)} entries, {b} holograms of {h} x {w} need "
                         f"{b * h * w}")
    use_mask = mask is not None and mask_flag
    if use_mask and np.shape(mask) != (h, w):
        raise ValueError(f"the mask has shape {np.shape(mask)}, the holograms {(h, w)}")
    n_loops = max(int(loops_first), int(loops))
    if resume:
        if initial_phase is not None or initial_weights is not None:
            raise ValueError("a resumed sequence starts from the previous one: no initial_phase or initial_weights")
        max_traps = max(min(_lib.SPOTS_MAX_TRAPS, -(-m // 32) * 32), m)
        sp = _SPOTS.get((b, h, w, max_traps, ain is not None))
        if sp is None or sp._seq is None or sp._seq[1] != m or sp.max_loops < n_loops:
            raise ValueError("resume=True needs a cached handle that holds a sequence of this shape and trap count")
    else:
        sp = _get_spots(b, h, w, m, ain is not None, n_loops)
        if ain is not None:
            sp.set_ain(ain)
        sp.set_feedback(feedback)
        sp.set_phase(None if initial_phase is None else np.asarray(initial_phase).reshape(b, h, w))
    try:
        sp.sequence(y, x, z, inten, w0, loops_first, loops, tol, resume, mask if use_mask else None, ct2pi,
                    _lib.QUANT_ASTYPE, frames=True, phases=bool(holograms))
    except _lib.SlmError as e:
        if resume and e.code == _lib.ERR_STATE:
            raise ValueError(f"resume=True: {e}") from e
        raise
    frames, phases, v, stats, weights, iters = sp.sequence_read(phases=bool(holograms))
    holo = phases.astype(np.float64) if holograms else None
    inten_out = v.real ** 2 + v.imag ** 2
    exp = None
    if options is not None:
        exp = _expected_from_device(sp, b, h, w, f, options, ain, mask if use_mask else None, ct2pi)
    if single:
        return SequenceResult(frames[:, 0], None if holo is None else holo[:, 0], inten_out[:, 0], stats[:, 0],
                              iters[:, 0], weights[:, 0], None if exp is None else exp[:, 0])
    return SequenceResult(frames, holo, inten_out, stats, iters, weights, exp)


def trap_window(ys, xs, margin=4.0, oversample=8):
    """The far-field window that shows every given trap position (any shape:
    one list, a batch, a whole trajectory): the bounding box of the positions
    widened by `margin` far-field pixels on every side, sampled at 1/oversample
    of a pixel, the origin snapped outwards to a multiple of the pitch so that
    every whole bin inside is a sample point. Returns (origin, pitch, size) as
    farfield_zoom takes them. Pure host code."""
    oversample = int(oversample)
    margin = float(margin)
    if oversample < 1:
        raise ValueError(f"oversample must be a positive whole number, got {oversample}")
    if not (np.isfinite(margin) and margin >= 0):
        raise ValueError(f"margin must be finite and >= 0, got {margin}")
    origin, size = [], []
    for name, v in (("ys", ys), ("xs", xs)):
        v = np.asarray(v, dtype=np.float64)
        if v.size == 0 or not np.all(np.isfinite(v)):
            raise ValueError(f"{name} must hold at least one position, all finite")
        first = int(np.floor((v.min() - margin) * oversample))  # in samples from bin 0
        last = int(np.ceil((v.max() + margin) * oversample))
        n = last - first + 1
        if n > _lib.ZOOM_MAX_SAMPLES:
            raise ValueError(f"the window along {name} would have {n} samples, above {_lib.ZOOM_MAX_SAMPLES}: lower "
                             f"oversample ({oversample}) or margin ({margin}), or preview fewer traps at once")
        origin.append(first / oversample)
        size.append(n)
    return (origin[0], origin[1]), (1.0 / oversample, 1.0 / oversample), (size[0], size[1])


def trap_windows(ys, xs, margin=4.0, oversample=8):
    """A window per frame of a trajectory ys, xs [F][M] that follows the traps:
    frame f gets trap_window's box around its own traps, the origin snapped to
    the pitch as there, and all frames share the largest size among them (a
    smaller frame's window grows at its far edges). Returns (origins [F][2],
    pitch, size). Pure host code."""
    y, x = np.asarray(ys, dtype=np.float64), np.asarray(xs, dtype=np.float64)
    if y.ndim != 2 or y.shape != x.shape or y.size == 0:
        raise ValueError(f"a trajectory is ys, xs [F][M], got shapes {y.shape} and {x.shape}")
    boxes = [trap_window(y[f], x[f], margin, oversample) for f in range(y.shape[0])]
    origins = np.array([box[0] for box in boxes], dtype=np.float64)
    size = (max(box[2][0] for box in boxes), max(box[2][1] for box in boxes))
    return origins, boxes[0][1], size


def expected_outcome(hologram_or_frame, window, z=0.0, ain=None, ct2pi=None):
    """The far-field intensity a hologram (floating phase, [H][W] or
    [B][H][W]) or a uint8 SLM frame (with its ct2pi) produces on `window` =
    (origin, pitch, size), as trap_window returns it, in the focal plane of the
    defocus z: _lib.farfield_zoom, float32 [..][ny][nx]. A frame is previewed as
    it is displayed: no correction mask is taken off."""
    origin, pitch, size = window
    return _lib.farfield_zoom(hologram_or_frame, origin, pitch, size, z=z, ain=ain, ct2pi=ct2pi)


def trap_frame(shape, coords, which, mask=None, mask_flag: bool = True, ct2pi=256):
    """update_hologram + display_hologram's quantisation in one launch; returns
    (hologram float64, frame uint8)."""
    y, x = _trap_index(np.empty(shape, np.uint8), coords, which)
    phase, frame = _lib.trap_frames(shape, [y], [x], mask if (mask_flag and mask is not None) else None, ct2pi,
                                    _lib.QUANT_ASTYPE)
    return phase[0], frame[0]
