"""ctypes binding of libslm_hip.so (C-ABI declared in include/slm_hip.h).

The shared library is the only compute path of this package: there is no CPU
fallback. Loading fails loudly when the library has not been built, and every
compute call raises :class:`SlmError` when no gfx950 device is usable.

No torch: the library links the system ROCm runtime (libamdhip64, librccl).
A process that also imports PyTorch-ROCm (which bundles its own HIP runtime)
should import torch first so that one runtime is mapped.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

# $SLM_LIB_PATH selects an experimental build (A/B variants); default is the in-tree library
LIB_PATH = os.environ.get("SLM_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                          "libslm_hip.so")

ALGO_GS = 0
ALGO_GD = 1
ALGO_GSW = 2  # weighted GS: no reference counterpart (include/slm_hip.h)
ALGO_MRAF = 3  # mixed-region amplitude freedom: no reference counterpart (include/slm_hip.h)
TGT_U8 = 0
TGT_F32 = 1
PRECISION_F32 = 0
PRECISION_F64 = 1

KERNEL_COL_MAIN = 0
KERNEL_ROW_MAIN = 1
KERNEL_GD_STATS = 2
KERNEL_OTHER = 3
NUM_KERNEL_CLASSES = 4
KERNEL_CLASS_NAMES = ("col_main", "row_main", "gd_stats", "other")

# sides with a radix plan (the fused FFT kernels); any other side runs the
# float64 any-size engine (generic.hip: mixed radix, or chirp-z line transforms)
SUPPORTED_LENGTHS = (64, 128, 256, 512, 768, 1024, 2048, 4096)


class SlmError(RuntimeError):
    """A libslm_hip call failed (message from slm_last_error)."""

    code = 0  # the library's return code (ERR_*), set by check()


ERR_ARG = -1
ERR_HIP = -2
ERR_UNSUPPORTED = -3
ERR_STATE = -4


_c_int = ctypes.c_int
_c_double = ctypes.c_double
_c_float = ctypes.c_float
_vp = ctypes.c_void_p
_P = ctypes.POINTER

# (name, restype, argtypes) for every symbol of include/slm_hip.h
_SIGNATURES = [
    ("slm_init", _c_int, [_c_int]),
    ("slm_device_count", _c_int, []),
    ("slm_last_error", ctypes.c_char_p, []),
    ("slm_version", ctypes.c_char_p, []),
    ("slm_supported_length", _c_int, [_c_int]),
    ("slm_device_pci_bus_id", _c_int, [_c_int, ctypes.c_char_p, _c_int]),
    ("slm_copy_bandwidth", _c_int, [ctypes.c_longlong, _c_int, _P(_c_double)]),
    ("slm_plan_create", _c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _P(_vp)]),
    ("slm_plan_destroy", _c_int, [_vp]),
    ("slm_plan_set_target", _c_int, [_vp, _vp]),
    ("slm_plan_set_precision", _c_int, [_vp, _c_int]),
    ("slm_plan_get_precision", _c_int, [_vp]),
    ("slm_plan_set_ain", _c_int, [_vp, _vp]),
    ("slm_plan_set_phase", _c_int, [_vp, _vp]),
    ("slm_plan_set_field", _c_int, [_vp, _vp]),
    ("slm_plan_set_lr", _c_int, [_vp, _vp]),
    ("slm_plan_set_feedback", _c_int, [_vp, _c_float]),
    ("slm_plan_set_weights", _c_int, [_vp, _vp]),
    ("slm_plan_read_weights", _c_int, [_vp, _vp]),
    ("slm_plan_set_region", _c_int, [_vp, _vp]),
    ("slm_plan_set_mixing", _c_int, [_vp, _c_float]),
    ("slm_plan_read_efficiency", _c_int, [_vp, _vp]),
    ("slm_plan_run", _c_int, [_vp, _c_int, _c_double, _c_int, _c_float]),
    ("slm_plan_run_timed", _c_int, [_vp, _c_int, _c_double, _c_int, _c_float, _vp, _vp]),
    ("slm_plan_sync", _c_int, [_vp]),
    ("slm_plan_mark", _c_int, [_vp, _c_int]),
    ("slm_plan_marked_ms", _c_int, [_vp, _P(_c_double)]),
    ("slm_plan_gd_recoveries", _c_int, [_vp]),
    ("slm_plan_read", _c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("slm_plan_read_target_stats", _c_int, [_vp, _vp, _vp]),
    ("slm_plan_set_target_stats", _c_int, [_vp, _vp, _vp]),
    ("slm_plan_read_field", _c_int, [_vp, _vp]),
    ("slm_plan_sequence", _c_int, [_vp, _c_int, _vp, _vp, _c_int, _c_int, _c_double, _c_int, _vp, _c_double, _c_int,
                                   _c_int, _c_int, _c_int]),
    ("slm_plan_sequence_read", _c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("slm_plan_kernel_bytes", ctypes.c_longlong, [_vp, _c_int]),
    ("slm_plan_info", _c_int, [_vp, _vp]),
    ("slm_plan_generic_info", _c_int, [_vp, _vp]),
    ("slm_plan_layout", _c_int, [_vp, _vp, _vp]),
    ("slm_plan_engine", _c_int, [_vp, _vp, _vp]),
    ("slm_plan_device", _c_int, [_vp]),
    ("slm_plan_read_trace", _c_int, [_vp, _c_int, _vp]),
    ("slm_gs", _c_int, [_vp, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_double, _vp, _vp, _vp, _vp, _vp]),
    ("slm_gsw", _c_int, [_vp, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_double, _vp, _vp, _vp, _vp, _vp,
                         _c_float, _vp, _vp]),
    ("slm_gd", _c_int,
     [_vp, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_double, _vp, _vp, _c_float, _vp, _vp, _vp, _vp]),
    ("slm_fft2", _c_int, [_vp, _vp, _c_int, _c_int, _c_int, _c_int]),
    ("slm_gs_multi", _c_int, [_c_int, _vp, _vp, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_double, _vp, _vp,
                              _vp, _vp, _vp]),
    ("slm_gsw_multi", _c_int, [_c_int, _vp, _vp, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_double, _vp, _vp,
                               _vp, _vp, _vp, _c_float]),
    ("slm_gs_multi_timing", _c_int, [_c_int, _vp, _vp]),
    ("slm_comm_unique_id", _c_int, [_vp]),
    ("slm_comm_init", _c_int, [_c_int, _c_int, _vp]),
    ("slm_comm_destroy", _c_int, []),
    ("slm_plan_gather_phase", _c_int, [_vp, _vp, _c_int, _vp]),
    ("slm_plan_gather_stats", _c_int, [_vp, _vp, _c_int, _vp, _vp]),
    ("slm_plan_time_gather", _c_int, [_vp, _vp, _c_int, _c_int, _P(_c_double), _P(ctypes.c_longlong)]),
    ("slm_gather_layout", _c_int, [_c_int, _vp, ctypes.c_longlong, _vp]),
    ("slm_trap_frames", _c_int,
     [_c_int, _c_int, _c_int, _vp, _vp, _vp, _c_double, _c_int, _vp, _vp]),
    ("slm_quantize", _c_int, [_vp, _c_int, _vp, _c_int, _c_int, _c_int, _c_double, _c_int, _vp]),
    ("slm_transform_hologram", _c_int, [_vp, _c_int, _c_int, _c_int, _vp, _vp]),
    ("slm_fft2_intensity", _c_int, [_vp, _c_int, _c_int, _c_int, _vp]),
    ("slm_fft2_c128", _c_int, [_vp, _vp, _c_int, _c_int, _c_int, _c_int]),
    ("slm_release_caches", _c_int, []),
    ("slm_spots_create", _c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _P(_vp)]),
    ("slm_spots_destroy", _c_int, [_vp]),
    ("slm_spots_set_traps", _c_int, [_vp, _c_int, _vp, _vp, _vp, _vp]),
    ("slm_spots_set_ain", _c_int, [_vp, _vp]),
    ("slm_spots_set_phase", _c_int, [_vp, _vp]),
    ("slm_spots_set_weights", _c_int, [_vp, _vp]),
    ("slm_spots_set_feedback", _c_int, [_vp, _c_float]),
    ("slm_spots_run", _c_int, [_vp, _c_int]),
    ("slm_spots_run_timed", _c_int, [_vp, _c_int, _vp]),
    ("slm_spots_read", _c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("slm_spots_info", _c_int, [_vp, _vp]),
    ("slm_spots_sequence", _c_int, [_vp, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _c_int, _c_int, _c_double, _c_int,
                                    _vp, _c_double, _c_int, _c_int, _c_int]),
    ("slm_spots_sequence_read", _c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("slm_spots_fields", _c_int, [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("slm_spots_superpose", _c_int, [_c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp]),
    ("slm_farfield_zoom", _c_int, [_vp, _c_int, _c_int, _c_int, _c_int, _vp, _c_double, _c_double, _c_double,
                                   _c_double, _c_double, _c_int, _c_int, _c_double, _vp, _vp]),
    ("slm_farfield_zoom_timed", _c_int, [_vp, _c_int, _c_int, _c_int, _c_int, _vp, _c_double, _c_double, _c_double,
                                         _c_double, _c_double, _c_int, _c_int, _c_double, _vp, _vp, _vp]),
    ("slm_zoom_create", _c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _P(_vp)]),
    ("slm_zoom_destroy", _c_int, [_vp]),
    ("slm_zoom_set_ain", _c_int, [_vp, _vp]),
    ("slm_zoom_set_mask", _c_int, [_vp, _vp]),
    ("slm_zoom_set_window", _c_int, [_vp, _c_int, _vp, _vp, _vp, _c_double, _c_double, _c_int, _c_int]),
    ("slm_zoom_set_timed", _c_int, [_vp, _c_int]),
    ("slm_zoom_run", _c_int, [_vp, _vp, _c_int, _c_int, _c_double, _c_int]),
    ("slm_zoom_run_spots", _c_int, [_vp, _vp, _c_int, _c_int, _c_double, _c_int]),
    ("slm_zoom_run_plan", _c_int, [_vp, _vp, _c_int, _c_int, _c_double, _c_int]),
    ("slm_zoom_read", _c_int, [_vp, _vp, _vp, _vp]),
    ("slm_zoom_info", _c_int, [_vp, _vp]),
]

ZOOM_PHASE_F32 = 0
ZOOM_LEVELS_U8 = 1
ZOOM_KERNEL_TABLES = 0
ZOOM_KERNEL_FIELD = 1
ZOOM_KERNEL_ROWS = 2
ZOOM_KERNEL_COLS = 3
ZOOM_NUM_KERNEL_CLASSES = 4
ZOOM_KERNEL_CLASS_NAMES = ("tables", "field", "rows", "cols")
ZOOM_MIN_SIDE, ZOOM_MAX_SIDE = 2, 4096  # hologram sides
ZOOM_MAX_SAMPLES = 4096  # per window side
ZOOM_MAX_BATCH = 1024  # holograms per run of a Zoom handle

SPOTS_KERNEL_FIELDS = 0
SPOTS_KERNEL_UPDATE = 1
SPOTS_KERNEL_SUPERPOSE = 2
SPOTS_NUM_KERNEL_CLASSES = 3
SPOTS_KERNEL_CLASS_NAMES = ("fields", "update", "superpose")
SPOTS_MAX_TRAPS = 1024

TRANSFORM_DEFLECT = 1
TRANSFORM_LENS = 2

QUANT_ASTYPE = 0
QUANT_PIL = 1
SRC_F64 = 0
SRC_I16 = 1

_lib = None


def load() -> ctypes.CDLL:
    """Load libslm_hip.so once; raise ImportError if it was never built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C spatial_light_modulator_module_amd/csrc`). There is no CPU fallback."
        )
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, res, args in _SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    msg = load().slm_last_error()
    return msg.decode() if msg else ""


def check(rc: int, what: str) -> None:
    if rc != 0:
        err = SlmError(f"{what} failed ({rc}): {last_error()}")
        err.code = rc
        raise err


def ptr(a: np.ndarray | None) -> int | None:
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "arrays passed to libslm_hip must be C-contiguous"
    return a.ctypes.data


_initialised_device: int | None = None


def init(device: int | None = None) -> None:
    """Bind this process to one GPU (default: $SLM_DEVICE, $LOCAL_RANK or 0)."""
    global _initialised_device
    if device is None:
        device = int(os.environ.get("SLM_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    if _initialised_device == device:
        return
    check(load().slm_init(device), f"slm_init({device})")
    _initialised_device = device


def device_count() -> int:
    return int(load().slm_device_count())


def pci_bus_id(device: int) -> str:
    """PCI bus id of a HIP device (slm_device_pci_bus_id)."""
    buf = ctypes.create_string_buffer(64)
    check(load().slm_device_pci_bus_id(int(device), buf, 64), "slm_device_pci_bus_id")
    return buf.value.decode()


def gs_multi_timing(max_shards: int = 64):
    """(wall_ms, run_ms) per shard of this process's last gs_multi call."""
    wall = np.zeros(max_shards, np.float64)
    run = np.zeros(max_shards, np.float64)
    n = int(load().slm_gs_multi_timing(int(max_shards), ptr(wall), ptr(run)))
    return wall[:min(n, max_shards)].tolist(), run[:min(n, max_shards)].tolist()


def copy_bandwidth(nbytes: int, reps: int = 20) -> float:
    """Measured streaming-copy rate of two nbytes device buffers, GB/s
    (read + write; slm_copy_bandwidth)."""
    init()
    g = ctypes.c_double()
    check(load().slm_copy_bandwidth(int(nbytes), int(reps), ctypes.byref(g)), "slm_copy_bandwidth")
    return float(g.value)


class Plan:
    """A device-resident batch of holograms (slm_plan_* in include/slm_hip.h)."""

    def __init__(self, algo: int, batch: int, height: int, width: int, tgt_type: int, has_ain: bool,
                 max_loops: int):
        init()
        self._lib = load()
        h = ctypes.c_void_p()
        check(self._lib.slm_plan_create(algo, batch, height, width, tgt_type, int(bool(has_ain)), max_loops,
                                        ctypes.byref(h)), "slm_plan_create")
        self.handle = h
        self.algo, self.batch, self.height, self.width = algo, batch, height, width
        self.tgt_type, self.has_ain, self.max_loops = tgt_type, bool(has_ain), max_loops

    def close(self) -> None:
        if getattr(self, "handle", None):
            self._lib.slm_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def shape(self):
        return (self.batch, self.height, self.width)

    def set_target(self, tgt: np.ndarray) -> None:
        dt = np.uint8 if self.tgt_type == TGT_U8 else np.float32
        a = np.ascontiguousarray(tgt, dtype=dt).reshape(self.shape)
        check(self._lib.slm_plan_set_target(self.handle, ptr(a)), "slm_plan_set_target")

    @property
    def precision(self) -> int:
        return int(self._lib.slm_plan_get_precision(self.handle))

    def set_precision(self, precision: int) -> None:
        check(self._lib.slm_plan_set_precision(self.handle, int(precision)), "slm_plan_set_precision")

    def set_ain(self, ain: np.ndarray) -> None:
        a = np.ascontiguousarray(ain, dtype=np.float32).reshape(self.height, self.width)
        check(self._lib.slm_plan_set_ain(self.handle, ptr(a)), "slm_plan_set_ain")

    def set_phase(self, phase: np.ndarray | None) -> None:
        a = None if phase is None else np.ascontiguousarray(phase, dtype=np.float32).reshape(self.shape)
        check(self._lib.slm_plan_set_phase(self.handle, ptr(a)), "slm_plan_set_phase")

    def set_field(self, field: np.ndarray | None) -> None:
        a = None
        if field is not None:
            a = np.ascontiguousarray(np.asarray(field).astype(np.complex64)).reshape(self.shape)
            a = a.view(np.float32)
        check(self._lib.slm_plan_set_field(self.handle, ptr(a)), "slm_plan_set_field")

    def set_lr(self, lr: np.ndarray) -> None:
        a = np.ascontiguousarray(lr, dtype=np.float32)
        if a.size != self.max_loops:
            raise ValueError(f"need {self.max_loops} learning rates, got {a.size}")
        check(self._lib.slm_plan_set_lr(self.handle, ptr(a)), "slm_plan_set_lr")

    def set_feedback(self, feedback: float) -> None:
        """Weighted GS: the exponent p of g *= (a_T / |C|)^p (slm_plan_set_feedback)."""
        check(self._lib.slm_plan_set_feedback(self.handle, float(feedback)), "slm_plan_set_feedback")

    def set_weights(self, weights: np.ndarray | None) -> None:
        """Weighted GS: initial weights [batch][h][w], None = ones (slm_plan_set_weights)."""
        a = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32).reshape(self.shape)
        check(self._lib.slm_plan_set_weights(self.handle, ptr(a)), "slm_plan_set_weights")

    def read_weights(self) -> np.ndarray:
        """Weighted GS: the weights after the last run, mean 1 over the support
        (T > 0) and exactly 1 off it (slm_plan_read_weights)."""
        out = np.empty(self.shape, np.float32)
        check(self._lib.slm_plan_read_weights(self.handle, ptr(out)), "slm_plan_read_weights")
        return out

    def set_region(self, region: np.ndarray) -> None:
        """MRAF: the signal region [batch][h][w], nonzero = signal (slm_plan_set_region)."""
        a = np.ascontiguousarray(np.asarray(region) != 0, dtype=np.uint8).reshape(self.shape)
        check(self._lib.slm_plan_set_region(self.handle, ptr(a)), "slm_plan_set_region")

    def set_mixing(self, mixing: float) -> None:
        """MRAF: the mixing parameter m in (0, 1] (slm_plan_set_mixing)."""
        check(self._lib.slm_plan_set_mixing(self.handle, float(mixing)), "slm_plan_set_mixing")

    def read_efficiency(self) -> np.ndarray:
        """MRAF: sum_sr E / P per iteration of the last run, [batch][max_loops]
        (slm_plan_read_efficiency)."""
        out = np.empty((self.batch, self.max_loops), np.float64)
        check(self._lib.slm_plan_read_efficiency(self.handle, ptr(out)), "slm_plan_read_efficiency")
        return out

    def run(self, loops: int, tol: float = 0.0, checked: bool = False, white_attention: float = 0.0) -> None:
        check(self._lib.slm_plan_run(self.handle, loops, float(tol), int(bool(checked)), float(white_attention)),
              "slm_plan_run")

    def run_timed(self, loops: int, tol: float = 0.0, checked: bool = False, white_attention: float = 0.0):
        us = np.zeros(NUM_KERNEL_CLASSES, dtype=np.float64)
        cnt = np.zeros(NUM_KERNEL_CLASSES, dtype=np.int32)
        check(self._lib.slm_plan_run_timed(self.handle, loops, float(tol), int(bool(checked)),
                                           float(white_attention), ptr(us), ptr(cnt)), "slm_plan_run_timed")
        return us, cnt

    def sync(self) -> None:
        check(self._lib.slm_plan_sync(self.handle), "slm_plan_sync")

    def mark(self, which: int) -> None:
        """Record stopwatch event 0 or 1 on the plan stream (slm_plan_mark)."""
        check(self._lib.slm_plan_mark(self.handle, int(which)), "slm_plan_mark")

    def marked_ms(self) -> float:
        """Device time between marks 0 and 1 (slm_plan_marked_ms)."""
        ms = ctypes.c_double()
        check(self._lib.slm_plan_marked_ms(self.handle, ctypes.byref(ms)), "slm_plan_marked_ms")
        return float(ms.value)

    @property
    def gd_recoveries(self) -> int:
        """GD runs redone on the two-launch column side after the one-launch
        grid wait gave up (slm_plan_gd_recoveries)."""
        return int(self._lib.slm_plan_gd_recoveries(self.handle))

    def read(self, phase=True, expected=True, stats=True, iters=True):
        out_phase = np.empty(self.shape, np.float32) if phase else None
        out_exp = np.empty(self.shape, np.float32) if expected else None
        out_stats = np.empty((self.batch, self.max_loops, 4), np.float64) if stats else None
        out_iters = np.empty(self.batch, np.int32) if iters else None
        check(self._lib.slm_plan_read(self.handle, ptr(out_phase), ptr(out_exp), ptr(out_stats), ptr(out_iters)),
              "slm_plan_read")
        return out_phase, out_exp, out_stats, out_iters

    def sequence(self, targets, regions=None, loops_first: int = 5, loops: int = 5, tol: float = 0.0,
                 resume: bool = False, mask=None, ct2pi=256.0, rule: int = QUANT_PIL, frames: bool = True,
                 phases: bool = False, expected: bool = False) -> None:
        """slm_plan_sequence: targets [F][batch][h][w] (and, for MRAF plans,
        regions of the same shape, or None for the region in force) as one
        enqueued chain, bit for bit the loop of set_target / set_phase(previous
        phase) / run(loops_first for frame 0, else loops; tol; checked = tol > 0)
        / quantize per frame. Returns once the chain is enqueued; sequence_read
        waits."""
        dt = np.uint8 if self.tgt_type == TGT_U8 else np.float32
        t = np.ascontiguousarray(targets, dtype=dt)
        per = self.batch * self.height * self.width
        if t.ndim < 3 or t.size == 0 or t.size % per or t.shape[-2:] != (self.height, self.width):
            raise ValueError(f"targets of shape {t.shape} are not [frames][batch {self.batch}]"
                             f"[{self.height}][{self.width}]")
        f = t.size // per
        r = None
        if regions is not None:
            r = np.ascontiguousarray(np.asarray(regions) != 0, dtype=np.uint8)
            if r.size != t.size or r.shape[-2:] != (self.height, self.width):
                raise ValueError(f"regions of shape {r.shape} do not match targets of shape {t.shape}")
        mk = None
        if mask is not None:
            mk = np.ascontiguousarray(mask, dtype=np.float64)
            if mk.shape != (self.height, self.width):
                raise ValueError(f"the mask has shape {mk.shape}, the holograms {(self.height, self.width)}")
        check(self._lib.slm_plan_sequence(self.handle, f, ptr(t), ptr(r), int(loops_first), int(loops), float(tol),
                                          int(bool(resume)), ptr(mk), float(ct2pi), int(rule), int(bool(frames)),
                                          int(bool(phases)), int(bool(expected))), "slm_plan_sequence")
        self._seq = (f, max(int(loops_first), int(loops)))

    def sequence_read(self, frames=True, phases=False, expected=False, stats=True, efficiency=False, iters=True):
        """(frames uint8 [F][B][H][W], phases and expected float32 [F][B][H][W],
        stats [F][B][max(loops_first, loops)][4], efficiency
        [F][B][max(loops_first, loops)] (MRAF), iters int32 [F][B] as read()
        has them) of the last sequence; None where not asked for."""
        f, rows = getattr(self, "_seq", None) or (1, 1)
        fb = (f, self.batch)
        out_f = np.empty(fb + (self.height, self.width), np.uint8) if frames else None
        out_p = np.empty(fb + (self.height, self.width), np.float32) if phases else None
        out_e = np.empty(fb + (self.height, self.width), np.float32) if expected else None
        out_s = np.empty(fb + (rows, 4), np.float64) if stats else None
        out_eff = np.empty(fb + (rows,), np.float64) if efficiency else None
        out_i = np.empty(fb, np.int32) if iters else None
        check(self._lib.slm_plan_sequence_read(self.handle, ptr(out_f), ptr(out_p), ptr(out_e), ptr(out_s),
                                               ptr(out_eff), ptr(out_i)), "slm_plan_sequence_read")
        return out_f, out_p, out_e, out_s, out_eff, out_i

    def target_stats(self):
        norm = np.empty(self.batch, np.float64)
        st2 = np.empty(self.batch, np.float64)
        check(self._lib.slm_plan_read_target_stats(self.handle, ptr(norm), ptr(st2)), "slm_plan_read_target_stats")
        return norm, st2

    def set_target_stats(self, norm, sum_t2) -> None:
        n = np.ascontiguousarray(norm, dtype=np.float64).reshape(self.batch)
        s = np.ascontiguousarray(sum_t2, dtype=np.float64).reshape(self.batch)
        check(self._lib.slm_plan_set_target_stats(self.handle, ptr(n), ptr(s)), "slm_plan_set_target_stats")

    def read_field(self) -> np.ndarray:
        """GD state x [batch][h][w] complex64 after the last run."""
        out = np.empty(self.shape, np.complex64)
        check(self._lib.slm_plan_read_field(self.handle, ptr(out.view(np.float32))), "slm_plan_read_field")
        return out

    def kernel_bytes(self, cls: int) -> int:
        return int(self._lib.slm_plan_kernel_bytes(self.handle, cls))

    def info(self) -> dict:
        a = np.zeros(8, np.int32)
        check(self._lib.slm_plan_info(self.handle, ptr(a)), "slm_plan_info")
        return {"col_cw": int(a[0]), "col_workgroups": int(a[1]), "col_threads": int(a[2]),
                "row_threads": int(a[3]), "rows_per_workgroup": int(a[4]), "row_plan": int(a[5]),
                "col_plan": int(a[6]), "precision": "f64" if a[7] == PRECISION_F64 else "f32",
                "layout": self.layout(), "engine": self.engine()}

    def generic_info(self) -> dict:
        """The geometry an any-size plan runs (slm_plan_generic_info): engine
        name, precision, radix plan keys of rows / columns (-1 off the
        radix-plan engines), rows per row tile, columns per column tile, state
        layout ("rm" row-major, "b2" two-column panels) and column workgroups
        per hologram. Raises SlmError for a plan of the fused float32 engine
        (info() describes those)."""
        a = np.zeros(8, np.int32)
        check(self._lib.slm_plan_generic_info(self.handle, ptr(a)), "slm_plan_generic_info")
        names = ("stockham", "shuffle", "bluestein", "mixed-radix", "radix-c128", "radix-c64")
        return {"engine": names[int(a[0])], "precision": "f64" if a[1] == PRECISION_F64 else "f32",
                "row_plan": int(a[2]), "col_plan": int(a[3]), "rows_per_tile": int(a[4]),
                "cols_per_tile": int(a[5]), "layout": "b2" if a[6] else "rm", "col_workgroups": int(a[7])}

    @property
    def device(self) -> int:
        """HIP device of the plan (slm_plan_device)."""
        return int(self._lib.slm_plan_device(self.handle))

    def time_gather(self, counts, root: int = 0, reps: int = 5):
        """(ms per device-side phase gather, bytes this rank sends per gather):
        slm_plan_time_gather, collective."""
        c = np.ascontiguousarray(counts, dtype=np.int32)
        ms = ctypes.c_double()
        nb = ctypes.c_longlong()
        check(self._lib.slm_plan_time_gather(self.handle, ptr(c), int(root), int(reps), ctypes.byref(ms),
                                             ctypes.byref(nb)), "slm_plan_time_gather")
        return float(ms.value), int(nb.value)

    def engine(self) -> tuple[str, str]:
        """(column, row) transform engine of the GS iteration kernels:
        "stockham", "shuffle" (wave-shuffle pair, fft_shuffle.hpp) or, for
        sides without a float32 radix plan, "mixed-radix" (float64 radix
        2..13 kernels, mixed_radix.hpp) or "bluestein" (float64 1-D line
        transforms along rows and transposed columns, Bluestein's chirp-z
        for a side with a larger prime factor, generic.hip), and under
        $SLM_ENGINE=float64 on 2^k / 768 sides, and for uint8 GS / GD /
        float64 runs on 13-smooth SLM panel sides, "radix-c128" (float64
        Stockham kernels with complex128 state, radix_c128.hpp); float32 GS on
        panel sides (e.g. 1080 x 1920) "radix-c64" (the same kernels with
        complex64 state and float32 butterflies)."""
        c, r = ctypes.c_int(), ctypes.c_int()
        check(self._lib.slm_plan_engine(self.handle, ctypes.byref(c), ctypes.byref(r)), "slm_plan_engine")
        names = ("stockham", "shuffle", "bluestein", "mixed-radix", "radix-c128", "radix-c64")
        return names[c.value], names[r.value]

    def layout(self) -> tuple[int, int]:
        """(X, Y) panel widths of the plan's blocked device layouts."""
        x, y = ctypes.c_int(), ctypes.c_int()
        check(self._lib.slm_plan_layout(self.handle, ctypes.byref(x), ctypes.byref(y)), "slm_plan_layout")
        return 1 << x.value, 1 << y.value

    def read_trace(self, cls: int) -> np.ndarray:
        """[batch * workgroups, 8] phase timestamps of the last launch of a
        kernel class (SLM_TRACE builds with SLM_TRACE_BUF=1; diagnostics):
        tile start, loads done, transforms done, stores done, kernel entry,
        HW_ID, XCC_ID (kernels.hpp, trace_point)."""
        b, h, w = self.shape
        info = self.info()
        n = info["col_workgroups"] if cls == KERNEL_COL_MAIN else h // info["rows_per_workgroup"]
        out = np.zeros((b * n, 8), np.uint64)
        check(self._lib.slm_plan_read_trace(self.handle, cls, ptr(out)), "slm_plan_read_trace")
        return out

    def gather_phase(self, counts, root: int = 0, host_out: np.ndarray | None = None) -> None:
        c = np.ascontiguousarray(counts, dtype=np.int32)
        check(self._lib.slm_plan_gather_phase(self.handle, ptr(c), root, ptr(host_out)), "slm_plan_gather_phase")

    def gather_stats(self, counts, root: int = 0, want: bool = True):
        """Every rank's per-iteration statistics [sum(counts)][max_loops][4] and
        iterations executed [sum(counts)] on `root` (None elsewhere, or when
        want=False: the collective still runs, nothing is copied to the host)."""
        c = np.ascontiguousarray(counts, dtype=np.int32)
        total = int(c.sum())
        st = np.empty((total, self.max_loops, 4), np.float64) if want else None
        it = np.empty(total, np.int32) if want else None
        check(self._lib.slm_plan_gather_stats(self.handle, ptr(c), root, ptr(st), ptr(it)), "slm_plan_gather_stats")
        return st, it


def _trap_arrays(batch, n_traps, ys, xs, zs, intensity):
    """Trap coordinates as the C-contiguous [batch][n_traps] arrays slm_spots_* take."""
    y = np.ascontiguousarray(ys, dtype=np.float64).reshape(batch, n_traps)
    x = np.ascontiguousarray(xs, dtype=np.float64).reshape(batch, n_traps)
    z = None if zs is None else np.ascontiguousarray(zs, dtype=np.float64).reshape(batch, n_traps)
    i = None if intensity is None else np.ascontiguousarray(intensity, dtype=np.float32).reshape(batch, n_traps)
    return y, x, z, i


class Spots:
    """Device-resident weighted GS on trap lists (slm_spots_* in
    include/slm_hip.h): `batch` holograms of height x width with up to
    max_traps traps each, any panel shape."""

    def __init__(self, batch: int, height: int, width: int, max_traps: int, has_ain: bool = False,
                 max_loops: int = 30):
        init()
        self._lib = load()
        h = ctypes.c_void_p()
        check(self._lib.slm_spots_create(int(batch), int(height), int(width), int(max_traps), int(bool(has_ain)),
                                         int(max_loops), ctypes.byref(h)), "slm_spots_create")
        self.handle = h
        self.batch, self.height, self.width = int(batch), int(height), int(width)
        self.max_traps, self.has_ain, self.max_loops = int(max_traps), bool(has_ain), int(max_loops)
        self.n_traps = 0
        self.loops = 0
        self._seq = None  # (frames, traps, statistics rows per frame) of the last sequence

    def close(self) -> None:
        if getattr(self, "handle", None):
            self._lib.slm_spots_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def shape(self):
        return (self.batch, self.height, self.width)

    def set_traps(self, ys, xs, zs=None, intensity=None) -> None:
        """Trap lists [batch][n_traps]: positions in far-field pixels, defocus in
        radians per pixel^2 (None = 0), target intensities (None = 1). Returns
        the weights to ones."""
        n = np.asarray(ys).size // self.batch
        if n * self.batch != np.asarray(ys).size:
            raise ValueError(f"{np.asarray(ys).size} trap rows do not divide into a batch of {self.batch}")
        y, x, z, i = _trap_arrays(self.batch, n, ys, xs, zs, intensity) if n else (np.zeros(0),) * 2 + (None,) * 2
        check(self._lib.slm_spots_set_traps(self.handle, n, ptr(y), ptr(x), ptr(z), ptr(i)), "slm_spots_set_traps")
        self.n_traps = n

    def set_ain(self, ain: np.ndarray) -> None:
        a = np.ascontiguousarray(ain, dtype=np.float32).reshape(self.height, self.width)
        check(self._lib.slm_spots_set_ain(self.handle, ptr(a)), "slm_spots_set_ain")

    def set_phase(self, phase: np.ndarray | None) -> None:
        a = None if phase is None else np.ascontiguousarray(phase, dtype=np.float32).reshape(self.shape)
        check(self._lib.slm_spots_set_phase(self.handle, ptr(a)), "slm_spots_set_phase")

    def set_weights(self, weights: np.ndarray | None) -> None:
        a = None
        if weights is not None:
            a = np.ascontiguousarray(weights, dtype=np.float32).reshape(self.batch, max(self.n_traps, 1))
        check(self._lib.slm_spots_set_weights(self.handle, ptr(a)), "slm_spots_set_weights")

    def set_feedback(self, feedback: float) -> None:
        check(self._lib.slm_spots_set_feedback(self.handle, float(feedback)), "slm_spots_set_feedback")

    def run(self, loops: int) -> None:
        check(self._lib.slm_spots_run(self.handle, int(loops)), "slm_spots_run")
        self.loops = int(loops)

    def run_timed(self, loops: int) -> np.ndarray:
        """As run; returns microseconds per kernel class (SPOTS_KERNEL_*), HIP events."""
        us = np.zeros(SPOTS_NUM_KERNEL_CLASSES, np.float64)
        check(self._lib.slm_spots_run_timed(self.handle, int(loops), ptr(us)), "slm_spots_run_timed")
        self.loops = int(loops)
        return us

    def read(self, phase=True, fields=True, stats=True, weights=True):
        """(phase float32 [B][H][W], V complex128 [B][M] of the last iteration,
        stats [B][loops][4] = (efficiency, uniformity, min r, max r), weights
        float32 [B][M]); None where not asked for."""
        n = max(self.n_traps, 1)
        out_phase = np.empty(self.shape, np.float32) if phase else None
        out_v = np.empty((self.batch, n), np.complex128) if fields else None
        out_stats = np.empty((self.batch, max(self.loops, 1), 4), np.float64) if stats else None
        out_w = np.empty((self.batch, n), np.float32) if weights else None
        check(self._lib.slm_spots_read(self.handle, ptr(out_phase), None if out_v is None else out_v.ctypes.data,
                                       ptr(out_stats), ptr(out_w)), "slm_spots_read")
        return out_phase, out_v, out_stats, out_w

    def sequence(self, ys, xs, zs=None, intensity=None, weights0=None, loops_first: int = 30, loops: int = 4,
                 tol: float = 0.0, resume: bool = False, mask=None, ct2pi=256, rule: int = QUANT_ASTYPE,
                 frames: bool = True, phases: bool = False) -> None:
        """slm_spots_sequence: a trajectory ys, xs, zs, intensity [F][batch][n_traps]
        as one enqueued chain (frame f starts from frame f-1's unit field and
        weights; tol > 0 stops a frame on the device once its uniformity is
        <= tol). Returns once the chain is enqueued; sequence_read waits."""
        y = np.ascontiguousarray(ys, dtype=np.float64)
        if y.ndim < 2 or y.size == 0 or y.size % (y.shape[0] * self.batch):
            raise ValueError(f"ys of shape {y.shape} is not [frames][batch {self.batch}][traps]")
        f, n = y.shape[0], y.size // (y.shape[0] * self.batch)

        def same(v, dtype, name):
            if v is None:
                return None
            v = np.ascontiguousarray(v, dtype=dtype)
            if v.size != y.size:
                raise ValueError(f"{name} has {v.size} entries, ys {y.size}")
            return v

        x, z, i = same(xs, np.float64, "xs"), same(zs, np.float64, "zs"), same(intensity, np.float32, "intensity")
        w0 = None
        if weights0 is not None:
            w0 = np.ascontiguousarray(weights0, dtype=np.float32)
            if w0.size != self.batch * n:
                raise ValueError(f"weights0 has {w0.size} entries for {self.batch} lists of {n} traps")
        mk = None
        if mask is not None:
            mk = np.ascontiguousarray(mask, dtype=np.float64)
            if mk.shape != (self.height, self.width):
                raise ValueError(f"the mask has shape {mk.shape}, the holograms {(self.height, self.width)}")
        check(self._lib.slm_spots_sequence(self.handle, f, n, ptr(y), ptr(x), ptr(z), ptr(i), ptr(w0),
                                           int(loops_first), int(loops), float(tol), int(bool(resume)), ptr(mk),
                                           float(ct2pi), int(rule), int(bool(frames)), int(bool(phases))),
              "slm_spots_sequence")
        self.n_traps = n
        self._seq = (f, n, max(int(loops_first), int(loops)))

    def sequence_read(self, frames=True, phases=False, fields=True, stats=True, weights=True, iters=True):
        """(frames uint8 [F][B][H][W], phases float32 [F][B][H][W], V complex128
        [F][B][M], stats [F][B][max(loops_first, loops)][4] (rows past a frame's
        iteration count are 0), weights float32 [F][B][M], iters int32 [F][B]) of
        the last sequence; None where not asked for."""
        f, n, rows = self._seq or (1, 1, 1)
        fb = (f, self.batch)
        out_f = np.empty(fb + (self.height, self.width), np.uint8) if frames else None
        out_p = np.empty(fb + (self.height, self.width), np.float32) if phases else None
        out_v = np.empty(fb + (n,), np.complex128) if fields else None
        out_s = np.empty(fb + (rows, 4), np.float64) if stats else None
        out_w = np.empty(fb + (n,), np.float32) if weights else None
        out_i = np.empty(fb, np.int32) if iters else None
        check(self._lib.slm_spots_sequence_read(self.handle, ptr(out_f), ptr(out_p),
                                                None if out_v is None else out_v.ctypes.data, ptr(out_s), ptr(out_w),
                                                ptr(out_i)), "slm_spots_sequence_read")
        return out_f, out_p, out_v, out_s, out_w, out_i

    def info(self) -> dict:
        a = np.zeros(4, np.int32)
        check(self._lib.slm_spots_info(self.handle, ptr(a)), "slm_spots_info")
        return {"padded_traps": int(a[0]), "partials": int(a[1]), "cols_per_partial": int(a[2]),
                "waves_per_workgroup": int(a[3])}


def spots_fields(phase, ys, xs, zs=None, ain=None) -> np.ndarray:
    """slm_spots_fields (test entry): V [B][M] complex128 of exp(i phase)
    [B][H][W] (times ain [H][W]) at the traps ys, xs, zs [B][M]."""
    ph = np.ascontiguousarray(phase, dtype=np.float32)
    ph = ph[None] if ph.ndim == 2 else ph
    b, h, w = ph.shape
    n = np.asarray(ys).size // b
    y, x, z, _ = _trap_arrays(b, n, ys, xs, zs, None)
    a = None if ain is None else np.ascontiguousarray(ain, dtype=np.float32).reshape(h, w)
    out = np.empty((b, n), np.complex128)
    init()
    check(load().slm_spots_fields(b, h, w, n, ptr(y), ptr(x), ptr(z), ptr(a), ptr(ph), out.ctypes.data),
          "slm_spots_fields")
    return out


def spots_superpose(shape, c, ys, xs, zs=None) -> np.ndarray:
    """slm_spots_superpose (test entry): angle(sum_m c_m exp(i D_m)), float32
    [B][H][W], for complex c [B][M] and traps ys, xs, zs [B][M]."""
    h, w = shape
    cc = np.ascontiguousarray(c, dtype=np.complex128)
    cc = cc[None] if cc.ndim == 1 else cc
    b, n = cc.shape
    y, x, z, _ = _trap_arrays(b, n, ys, xs, zs, None)
    out = np.empty((b, h, w), np.float32)
    init()
    check(load().slm_spots_superpose(b, h, w, n, ptr(y), ptr(x), ptr(z), cc.ctypes.data, ptr(out)),
          "slm_spots_superpose")
    return out


def _pair(v, name, kind=float):
    """(a, b) from a pair, or from one number for both axes."""
    p = tuple(np.ravel(v).tolist())
    if len(p) == 1:
        p = p * 2
    if len(p) != 2:
        raise ValueError(f"{name} is one number or a (y, x) pair, got {v!r}")
    if kind is int:
        if any(int(c) != c for c in p):
            raise ValueError(f"{name} must be whole numbers, got {v!r}")
        return int(p[0]), int(p[1])
    return float(p[0]), float(p[1])


def _zoom_holograms(hologram, ct2pi):
    """(holograms [B][H][W] contiguous, float32 phases or uint8 levels, the kind,
    whether one [H][W] was given); ValueError on anything else."""
    holo = np.asarray(hologram)
    if holo.ndim not in (2, 3):
        raise ValueError(f"a hologram is [H][W] or [B][H][W], got shape {holo.shape}")
    if holo.dtype == np.uint8:
        kind = ZOOM_LEVELS_U8
        _zoom_check_ct2pi(ct2pi)
    elif np.issubdtype(holo.dtype, np.floating):
        kind = ZOOM_PHASE_F32
        holo = holo.astype(np.float32, copy=False)
    else:
        raise ValueError(f"a hologram is a floating phase or a uint8 frame, got dtype {holo.dtype}")
    single = holo.ndim == 2
    holo = np.ascontiguousarray(holo[None] if single else holo)
    if holo.shape[0] < 1:
        raise ValueError("the batch holds no hologram")
    return holo, kind, single


def _zoom_check_ct2pi(ct2pi):
    if ct2pi is None or not np.isfinite(ct2pi) or not ct2pi > 0:
        raise ValueError(f"a uint8 frame needs ct2pi finite and positive, got {ct2pi!r}")


def _zoom_check_sides(h, w):
    if not (ZOOM_MIN_SIDE <= h <= ZOOM_MAX_SIDE and ZOOM_MIN_SIDE <= w <= ZOOM_MAX_SIDE):
        raise ValueError(f"the zoom runs on sides {ZOOM_MIN_SIDE} .. {ZOOM_MAX_SIDE}, got {h} x {w}")


def _zoom_check_window(positions, dy, dx, ny, nx):
    """positions: every origin coordinate and defocus of the window(s)."""
    if not (1 <= ny <= ZOOM_MAX_SAMPLES and 1 <= nx <= ZOOM_MAX_SAMPLES):
        raise ValueError(f"a window has 1 .. {ZOOM_MAX_SAMPLES} samples per side, got {ny} x {nx}")
    if not (np.all(np.isfinite(positions)) and np.isfinite(dy) and np.isfinite(dx)):
        raise ValueError("the window's origin, pitch and defocus must be finite")
    if not (dy > 0 and dx > 0):
        raise ValueError(f"the pitch must be positive, got {dy} x {dx}")


def _zoom_ain(ain, h, w):
    if ain is None:
        return None
    a = np.ascontiguousarray(ain, dtype=np.float32)
    if a.shape != (h, w):
        raise ValueError(f"ain has shape {a.shape}, the hologram {(h, w)}")
    if not np.all(np.isfinite(a)):
        raise ValueError("ain has a non-finite entry")
    if not np.any(a):
        raise ValueError("ain is zero everywhere")
    return a


def farfield_zoom(hologram, origin, pitch, size, z=0.0, ain=None, ct2pi=None, return_field=False, timed=False):
    """slm_farfield_zoom: the far field of a hologram on the ny x nx samples
    y_j = origin[0] + j pitch[0], x_i = origin[1] + i pitch[1] (far-field
    pixels, fractional; `pitch` may be one number for both axes) with one
    defocus z (radians per pixel^2), in the trap-list conventions: a sample is
    what spots_fields gives for a trap there. `hologram` is [H][W] or
    [B][H][W]: a floating dtype is a phase in radians (taken as float32), uint8
    an SLM frame whose levels mean exp(i 2 pi level / ct2pi) (ct2pi required;
    no correction mask is applied). ain [H][W] is shared by the batch. Returns
    the float32 intensity |V|^2 in the hologram's leading shape + (ny, nx);
    with return_field also V complex128; with timed also the microseconds per
    kernel class (ZOOM_KERNEL_*) HIP events measured. Every argument is checked here
    (ValueError) before the device is touched."""
    holo, kind, single = _zoom_holograms(hologram, ct2pi)
    b, h, w = holo.shape
    _zoom_check_sides(h, w)
    (y0, x0), (dy, dx), (ny, nx) = _pair(origin, "origin"), _pair(pitch, "pitch"), _pair(size, "size", int)
    _zoom_check_window((y0, x0, float(z)), dy, dx, ny, nx)
    a = _zoom_ain(ain, h, w)
    out = np.empty((b, ny, nx), np.float32)
    field = np.empty((b, ny, nx), np.complex128) if return_field else None
    us = np.zeros(ZOOM_NUM_KERNEL_CLASSES, np.float64) if timed else None
    init()
    check(load().slm_farfield_zoom_timed(ptr(holo), kind, b, h, w, ptr(a), float(ct2pi or 0.0), y0, x0, dy, dx, ny, nx,
                                         float(z), ptr(out), None if field is None else field.ctypes.data, ptr(us)),
          "slm_farfield_zoom")
    res = [out[0] if single else out]
    if return_field:
        res.append(field[0] if single else field)
    if timed:
        res.append(us)
    return res[0] if len(res) == 1 else tuple(res)


class Zoom:
    """The resident zoomed far field (slm_zoom_* in include/slm_hip.h): up to
    `batch` holograms of height x width per run in the same launches, on windows
    of up to max_size = (ny, nx) samples (one number for both). Stream, buffers
    and tables stay with the handle; without a mask a sample is farfield_zoom's,
    bit for bit. Every argument of every method is checked here (ValueError)
    before the device is touched; the device handle itself is created by the
    first call that needs it."""

    def __init__(self, batch: int, height: int, width: int, max_size, timed: bool = False):
        if int(batch) != batch or not 1 <= batch <= ZOOM_MAX_BATCH:
            raise ValueError(f"a zoom handle takes 1 .. {ZOOM_MAX_BATCH} holograms per run, got {batch!r}")
        if int(height) != height or int(width) != width:
            raise ValueError(f"the sides must be whole numbers, got {height!r} x {width!r}")
        _zoom_check_sides(height, width)
        max_ny, max_nx = _pair(max_size, "max_size", int)
        if not (1 <= max_ny <= ZOOM_MAX_SAMPLES and 1 <= max_nx <= ZOOM_MAX_SAMPLES):
            raise ValueError(f"a window has 1 .. {ZOOM_MAX_SAMPLES} samples per side, got {max_ny} x {max_nx}")
        self.batch, self.height, self.width = int(batch), int(height), int(width)
        self.max_size = (max_ny, max_nx)
        self.timed = bool(timed)
        self.size = None  # (ny, nx) of the window in force
        self.per_hologram = False
        self.handle = None
        self._lib = None
        self._ran = None  # (count, (ny, nx), with the field) of the last run
        self._held = None  # the host array of the last run: the upload may still read it

    def _h(self):
        """The device handle, created at the first need."""
        if self.handle is None:
            init()
            self._lib = load()
            h = ctypes.c_void_p()
            check(self._lib.slm_zoom_create(self.batch, self.height, self.width, self.max_size[0], self.max_size[1],
                                            ctypes.byref(h)), "slm_zoom_create")
            self.handle = h
            check(self._lib.slm_zoom_set_timed(h, int(self.timed)), "slm_zoom_set_timed")
        return self.handle

    def close(self) -> None:
        if getattr(self, "handle", None):
            self._lib.slm_zoom_destroy(self.handle)
            self.handle = None
        self._held = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_ain(self, ain) -> None:
        """ain [H][W] shared by every hologram; None = ones."""
        a = _zoom_ain(ain, self.height, self.width)
        h = self._h()
        check(self._lib.slm_zoom_set_ain(h, ptr(a)), "slm_zoom_set_ain")

    def set_mask(self, mask) -> None:
        """The correction mask [H][W] (float64 radians) the holograms carry: it is
        taken off, the field is exp(i (phase - mask)). None = no mask."""
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, dtype=np.float64)
            if m.shape != (self.height, self.width):
                raise ValueError(f"the mask has shape {m.shape}, the holograms {(self.height, self.width)}")
            if not np.all(np.isfinite(m)):
                raise ValueError("the mask has a non-finite entry")
        h = self._h()
        check(self._lib.slm_zoom_set_mask(h, ptr(m)), "slm_zoom_set_mask")

    def set_window(self, origin, pitch, size, z=0.0) -> None:
        """One window (origin = (y0, x0), z a number) for every hologram, or one per
        hologram: origin [batch][2] and / or z [batch]; hologram i of a run then
        gets origin[i] and z[i]. Pitch and size are shared. Builds the tables."""
        o = np.asarray(origin, dtype=np.float64)
        zz = np.asarray(z, dtype=np.float64)
        if o.shape not in ((2,), (self.batch, 2)):
            raise ValueError(f"origin is (y0, x0) or an array [batch {self.batch}][2], got shape {o.shape}")
        if zz.shape not in ((), (self.batch,)):
            raise ValueError(f"z is one number or an array [batch {self.batch}], got shape {zz.shape}")
        (dy, dx), (ny, nx) = _pair(pitch, "pitch"), _pair(size, "size", int)
        _zoom_check_window(np.concatenate([o.ravel(), zz.ravel()]), dy, dx, ny, nx)
        if ny > self.max_size[0] or nx > self.max_size[1]:
            raise ValueError(f"a window of {ny} x {nx} samples exceeds the handle's {self.max_size[0]} x "
                             f"{self.max_size[1]}")
        per = o.ndim == 2 or zz.ndim == 1
        n = self.batch if per else 1
        o2 = np.broadcast_to(o, (n, 2))
        y0, x0 = np.ascontiguousarray(o2[:, 0]), np.ascontiguousarray(o2[:, 1])
        z1 = np.ascontiguousarray(np.broadcast_to(zz, (n,)))
        h = self._h()
        check(self._lib.slm_zoom_set_window(h, int(per), ptr(y0), ptr(x0), ptr(z1), dy, dx, ny, nx),
              "slm_zoom_set_window")
        self.size, self.per_hologram = (ny, nx), per

    def _check_run(self, count, ct2pi, levels):
        if self.size is None:
            raise ValueError("run before set_window")
        if not 1 <= count <= self.batch:
            raise ValueError(f"a run takes 1 .. {self.batch} holograms (the handle's batch), got {count}")
        if levels:
            _zoom_check_ct2pi(ct2pi)

    def run(self, holograms, ct2pi=None, return_field: bool = False) -> None:
        """`holograms` [count][H][W] (or one [H][W]) as farfield_zoom takes them,
        count <= batch: one upload, everything enqueued; read() waits."""
        holo, kind, _ = _zoom_holograms(holograms, ct2pi)
        if holo.shape[1:] != (self.height, self.width):
            raise ValueError(f"the holograms are {holo.shape[1:]}, the handle's {(self.height, self.width)}")
        self._check_run(holo.shape[0], ct2pi, kind == ZOOM_LEVELS_U8)
        h = self._h()
        self._held = holo
        check(self._lib.slm_zoom_run(h, ptr(holo), kind, holo.shape[0], float(ct2pi or 0.0), int(bool(return_field))),
              "slm_zoom_run")
        self._ran = (holo.shape[0], self.size, bool(return_field))

    def _run_frames(self, source, fn_name, first, count, ct2pi, return_field):
        if int(first) != first or int(count) != count:
            raise ValueError(f"first and count must be whole numbers, got {first!r} and {count!r}")
        if (source.height, source.width) != (self.height, self.width):
            raise ValueError(f"the frames are {(source.height, source.width)}, the handle's holograms "
                             f"{(self.height, self.width)}")
        seq = getattr(source, "_seq", None)
        if not seq or not getattr(source, "handle", None):
            raise ValueError("the source holds no sequence")
        self._check_run(count, ct2pi, True)
        total = seq[0] * source.batch
        if first < 0 or first + count > total:
            raise ValueError(f"frames {first} .. {first + count - 1} lie outside the sequence's {total}")
        h = self._h()
        check(getattr(self._lib, fn_name)(h, source.handle, int(first), int(count), float(ct2pi),
                                          int(bool(return_field))), fn_name)
        self._ran = (int(count), self.size, bool(return_field))

    def run_spots(self, spots: "Spots", first: int, count: int, ct2pi, return_field: bool = False) -> None:
        """The uint8 frames f B + b in [first, first + count) of the last
        Spots.sequence, read where they are on the device, ordered after the
        chain that writes them (and a later sequence after this run)."""
        self._run_frames(spots, "slm_zoom_run_spots", first, count, ct2pi, return_field)

    def run_plan(self, plan: "Plan", first: int, count: int, ct2pi, return_field: bool = False) -> None:
        """As run_spots, for the frames of the last Plan.sequence."""
        self._run_frames(plan, "slm_zoom_run_plan", first, count, ct2pi, return_field)

    def read(self):
        """Waits for the last run: the float32 intensity [count][ny][nx]; after a
        run with return_field also V complex128; on a timed handle also the
        microseconds per kernel class (ZOOM_KERNEL_*; the tables are no part of
        a run)."""
        if self._ran is None:
            raise ValueError("read before a run")
        count, (ny, nx), with_field = self._ran
        out = np.empty((count, ny, nx), np.float32)
        field = np.empty((count, ny, nx), np.complex128) if with_field else None
        us = np.zeros(ZOOM_NUM_KERNEL_CLASSES, np.float64) if self.timed else None
        check(self._lib.slm_zoom_read(self.handle, ptr(out), None if field is None else field.ctypes.data, ptr(us)),
              "slm_zoom_read")
        self._held = None
        res = [out] + ([field] if with_field else []) + ([us] if self.timed else [])
        return res[0] if len(res) == 1 else tuple(res)

    def info(self) -> dict:
        """How the last run was cut (slm_zoom_info)."""
        a = np.zeros(3, np.int32)
        check(self._lib.slm_zoom_info(self._h(), ptr(a)), "slm_zoom_info")
        return {"groups": int(a[0]), "bands": int(a[1]), "split_launches": int(a[2])}


def fft2(x: np.ndarray, inverse: bool = False) -> np.ndarray:
    """Unscaled 2-D C2C transform of [..., H, W] on the GPU (test entry)."""
    init()
    a = np.ascontiguousarray(x, dtype=np.complex64)
    shape = a.shape
    h, w = shape[-2:]
    b = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
    out = np.empty_like(a)
    check(load().slm_fft2(ptr(a.view(np.float32)), ptr(out.view(np.float32)), b, h, w, int(bool(inverse))),
          "slm_fft2")
    return out


def fft2_c128(x: np.ndarray, inverse: bool = False) -> np.ndarray:
    """Unscaled 2-D C2C transform of [..., H, W] complex128 in float64 on the
    GPU (slm_fft2_c128: the any-size engine's transforms; sides up to 4096, or
    up to 8192 without a prime factor above 13)."""
    init()
    a = np.ascontiguousarray(x, dtype=np.complex128)
    shape = a.shape
    h, w = shape[-2:]
    b = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
    out = np.empty_like(a)
    check(load().slm_fft2_c128(ptr(a.view(np.float64)), ptr(out.view(np.float64)), b, h, w, int(bool(inverse))),
          "slm_fft2_c128")
    return out


def release_caches() -> None:
    """Free the float64 engines slm_fft2_c128 keeps per shape (no-op without a library)."""
    if _lib is not None:
        check(_lib.slm_release_caches(), "slm_release_caches")


def transform_hologram(hologram, height, width, deflect_params=None, lens_params=None):
    """deflect / lens post-processing of src/generate_hologram.py:82-87 on the
    GPU (slm_transform_hologram). hologram float64 [h][w] or None (zeros);
    deflect_params = (sin(y u), sin(x u), 2 pi px / wl); lens_params =
    (2 pi f / wl, f, px)."""
    flags = 0
    params = np.zeros(6, np.float64)
    if deflect_params is not None:
        flags |= TRANSFORM_DEFLECT
        params[0:3] = deflect_params
    if lens_params is not None:
        flags |= TRANSFORM_LENS
        params[3:6] = lens_params
    src = None if hologram is None else np.ascontiguousarray(hologram, dtype=np.float64).reshape(height, width)
    out = np.empty((height, width), np.float64)
    init()
    check(load().slm_transform_hologram(ptr(src), height, width, flags, ptr(params), ptr(out)),
          "slm_transform_hologram")
    return out


def fft2_intensity(phase) -> np.ndarray:
    """|fft2(exp(1j phase))|^2 on the GPU (float32), phase [..., H, W]."""
    a = np.ascontiguousarray(phase, dtype=np.float32)
    h, w = a.shape[-2:]
    b = int(np.prod(a.shape[:-2])) if a.ndim > 2 else 1
    out = np.empty(a.shape, np.float32)
    init()
    check(load().slm_fft2_intensity(ptr(a), b, h, w, ptr(out)), "slm_fft2_intensity")
    return out


def gs_multi(targets, loops, devices, tol=0.0, ain=None, initial_phase=None, feedback=None):
    """slm_gs_multi: GS on a batch [B][H][W] sharded over `devices` (device ids,
    may repeat) from one process. Returns (phase, expected, stats, iters).
    With a feedback exponent: weighted GS (slm_gsw_multi)."""
    t = np.asarray(targets)
    tt = TGT_U8 if t.dtype == np.uint8 else TGT_F32
    t = np.ascontiguousarray(t, dtype=np.uint8 if tt == TGT_U8 else np.float32)
    b, h, w = t.shape
    dev = np.ascontiguousarray(devices, dtype=np.int32)
    a = None if ain is None else np.ascontiguousarray(ain, dtype=np.float32).reshape(h, w)
    ph0 = None if initial_phase is None else np.ascontiguousarray(initial_phase, dtype=np.float32).reshape(b, h, w)
    phase = np.empty((b, h, w), np.float32)
    expected = np.empty((b, h, w), np.float32)
    stats = np.empty((b, loops, 4), np.float64)
    iters = np.empty(b, np.int32)
    init()
    if feedback is None:
        check(load().slm_gs_multi(int(dev.size), ptr(dev), ptr(t), tt, ptr(a), b, h, w, int(loops), float(tol),
                                  ptr(ph0), ptr(phase), ptr(expected), ptr(stats), ptr(iters)), "slm_gs_multi")
    else:
        check(load().slm_gsw_multi(int(dev.size), ptr(dev), ptr(t), tt, ptr(a), b, h, w, int(loops), float(tol),
                                   ptr(ph0), ptr(phase), ptr(expected), ptr(stats), ptr(iters), float(feedback)),
              "slm_gsw_multi")
    return phase, expected, stats, iters


def gsw(targets, loops, feedback=1.0, tol=0.0, ain=None, initial_phase=None, initial_weights=None):
    """slm_gsw: one-shot weighted GS on a batch [B][H][W]. Returns (phase,
    expected, stats, iters, weights)."""
    t = np.asarray(targets)
    tt = TGT_U8 if t.dtype == np.uint8 else TGT_F32
    t = np.ascontiguousarray(t, dtype=np.uint8 if tt == TGT_U8 else np.float32)
    b, h, w = t.shape
    a = None if ain is None else np.ascontiguousarray(ain, dtype=np.float32).reshape(h, w)
    ph0 = None if initial_phase is None else np.ascontiguousarray(initial_phase, dtype=np.float32).reshape(b, h, w)
    w0 = None if initial_weights is None else np.ascontiguousarray(initial_weights, dtype=np.float32).reshape(b, h, w)
    phase = np.empty((b, h, w), np.float32)
    expected = np.empty((b, h, w), np.float32)
    stats = np.empty((b, loops, 4), np.float64)
    iters = np.empty(b, np.int32)
    weights = np.empty((b, h, w), np.float32)
    init()
    check(load().slm_gsw(ptr(t), tt, ptr(a), b, h, w, int(loops), float(tol), ptr(ph0), ptr(phase), ptr(expected),
                         ptr(stats), ptr(iters), float(feedback), ptr(w0), ptr(weights)), "slm_gsw")
    return phase, expected, stats, iters, weights


def gather_layout(counts, per_item: int) -> np.ndarray:
    """Rank-order element offsets of a gather (slm_gather_layout; host only):
    offsets[r] = per_item * sum(counts[:r]), offsets[-1] = the total."""
    c = np.ascontiguousarray(counts, dtype=np.int32)
    out = np.empty(c.size + 1, np.int64)
    check(load().slm_gather_layout(int(c.size), ptr(c), int(per_item), ptr(out)), "slm_gather_layout")
    return out


def comm_unique_id() -> bytes:
    buf = (ctypes.c_ubyte * 128)()
    check(load().slm_comm_unique_id(buf), "slm_comm_unique_id")
    return bytes(buf)


def comm_init(nranks: int, rank: int, uid: bytes) -> None:
    init()
    buf = (ctypes.c_ubyte * 128).from_buffer_copy(uid)
    check(load().slm_comm_init(nranks, rank, buf), "slm_comm_init")


def comm_destroy() -> None:
    load().slm_comm_destroy()


def trap_frames(shape, ys, xs, mask=None, ct2pi=256.0, rule=QUANT_ASTYPE, phase=True, frame=True):
    """Single-trap holograms (angle of ifft2 of one 255 pixel per trap) and/or
    their quantised SLM frames, one launch (slm_trap_frames)."""
    h, w = shape
    ys = np.ascontiguousarray(ys, dtype=np.int32).reshape(-1)
    xs = np.ascontiguousarray(xs, dtype=np.int32).reshape(-1)
    b = ys.size
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.float64).reshape(h, w)
    ph = np.empty((b, h, w), np.float64) if phase else None
    fr = np.empty((b, h, w), np.uint8) if frame else None
    init()
    check(load().slm_trap_frames(b, h, w, ptr(ys), ptr(xs), ptr(m), float(ct2pi), int(rule), ptr(ph), ptr(fr)),
          "slm_trap_frames")
    return ph, fr


def quantize(src, mask=None, ct2pi=256.0, rule=QUANT_PIL):
    """8-bit SLM levels of a float64 phase hologram (rule QUANT_ASTYPE / QUANT_PIL)
    or of an int16 hologram image, plus an optional float64 mask (slm_quantize)."""
    src = np.asarray(src)
    src_type = SRC_I16 if src.dtype == np.int16 else SRC_F64
    a = np.ascontiguousarray(src, dtype=np.int16 if src_type == SRC_I16 else np.float64)
    h, w = a.shape[-2:]
    b = int(np.prod(a.shape[:-2])) if a.ndim > 2 else 1
    m = None if mask is None else np.ascontiguousarray(np.broadcast_to(mask, (h, w)), dtype=np.float64)
    out = np.empty(a.shape, np.uint8)
    init()
    check(load().slm_quantize(ptr(a), src_type, ptr(m), b, h, w, float(ct2pi), int(rule), ptr(out)), "slm_quantize")
    return out
