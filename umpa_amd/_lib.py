"""
ctypes binding of the C ABI declared in ``include/umpa_hip.h``.

``Native`` wraps one shared library exporting that ABI under a symbol prefix.  The
product uses exactly one instance: ``libumpa_hip.so`` (prefix ``umpa_hip_``), the HIP
library built from ``umpa_amd/csrc``.  There is no CPU fallback: if the library is
missing, or no HIP device is present, loading / model creation raises.
(The CPU checkers under ``oracle/`` export the same call shapes under other prefixes;
only the test-suite binds those, through ``oracle/cpu_model.py``.)
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIB_PATH = os.path.join(_HERE, "libumpa_hip.so")

ST_OK, ST_BOUND, ST_DIM, ST_POSITIVE = 1, 2, 4, 8
F_DEVICE_FRAMES = 1
F_DEVICE_IO, F_FORCE_DIRECT, F_FORCE_TILED, F_PLANAR, F_REUSE_REF_MAPS, F_USE_STAGED, F_ASYNC, F_FORCE_PLAIN_DIRECT = 1, 2, 4, 8, 16, 32, 64, 128

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_dpp = C.POINTER(_dp)
_int, _vp, _dbl = C.c_int, C.c_void_p, C.c_double


class NativeError(RuntimeError):
    pass


def _ptr(a, typ):
    return a.ctypes.data_as(typ) if a is not None else None


class Library:
    """One loaded shared library: every function of ``table`` (``{name: (restype, argtypes)}``, exported as
    ``prefix + name``) is an attribute.  A table is the whole C ABI of its header: its keys are that library's ``*_SYMBOLS``."""

    def __init__(self, path, prefix, table):
        if not os.path.exists(path):
            raise NativeError(
                "native library %s not found - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)" % path)
        self.path, self.prefix = path, prefix
        self.lib = C.CDLL(path)
        for name, (restype, argtypes) in table.items():
            fn = getattr(self.lib, prefix + name)
            fn.restype, fn.argtypes = restype, argtypes
            setattr(self, name, fn)

    def error(self):
        last = getattr(self, "last_error", None)                     # (the CPU checkers keep no error text)
        return (last() or b"").decode() if last else ""

    def check(self, rc, what):
        if rc is not None and rc < 0:
            raise NativeError("%s failed (%d): %s" % (what, rc, self.error()))
        return rc


def _model_abi(is_hip):
    """``include/umpa_hip.h`` (``is_hip``), or the call shapes the CPU checkers share with it."""
    create = [_int, _int, _ip, _dpp, _dpp, _dpp, _ip, _int, _dp, _int, _int] + ([_int, _int] if is_hip else [])
    region = [_vp] + [_int] * 6 + [_vp, _int, _vp, _vp, _vp, _dbl, _vp, _vp, _vp] + ([_int, _vp] if is_hip else [_int])
    status = _int if is_hip else None
    abi = {
        "create": (_vp, create),
        "destroy": (None, [_vp]),
        "set_window": (status, [_vp, _dp, _int]),
        "set_subpx": (status, [_vp, _int]),
        "set_reference_shift": (status, [_vp, _int]),
        "coverage": (_int, [_vp, _dp, _int, _int]),
        "cost": (_int, [_vp, _int, _int, _int, _int, _dp]),
        "min": (_int, [_vp, _int, _int, _dp, _dp, _dp, _dp, _ip]),
        "match_region": (status, region),
    }
    if not is_hip:
        abi.update({"spmin": (_dbl, [_dp, _dp]), "spmin_quad": (_dbl, [_dp, _dp]), "max_threads": (_int, [])})
        return abi
    abi.update({
        "device_count": (_int, []),
        "last_error": (C.c_char_p, []),
        "version": (C.c_char_p, []),
        "coverage_region": (_int, [_vp] + [_int] * 6 + [_dp]),
        "spmin": (_int, [_int, _dp, _dp, _dp]),
        "spmin_quad": (_int, [_int, _dp, _dp, _dp]),
        "timing_enable": (_int, [_vp, _int]),
        "timing_collect": (_int, [_vp]),
        "timing_read": (_int, [_vp, _int, C.POINTER(C.c_char_p), _dp, _ip]),
        "timing_fma": (_int, [_vp, _int, _dp]),
        "host_alloc": (_vp, [C.c_size_t]),
        "host_free": (None, [_vp]),
        "host_trim": (None, []),
        "stage_sample": (_int, [_vp, _vp, _int, _vp, _vp]),
        "wait": (_int, [_vp]),
        "set_rows_callback": (_int, [_vp, _vp, _vp, _int]),
        "host_register": (_int, [_vp, C.c_size_t]),
        "host_unregister": (_int, [_vp]),
        "last_path": (_int, [_vp]),
        "last_stats": (_int, [_vp, _dp]),
        "update_frames": (_int, [_vp, _dpp, _dpp]),
        "correct_bad_pixels": (_int, [_vp, _vp, C.c_long, _int, _int, _int, _dbl, _dbl, _int, _int, _int, _vp]),
    })
    return abi


# every symbol include/umpa_hip.h declares (checked by tests/test_cabi_symbols.py)
HIP_SYMBOLS = list(_model_abi(True))


class Native(Library):
    """One loaded library + prefix with the model ABI: ``libumpa_hip.so``, or a CPU checker of ``oracle/``."""

    def __init__(self, path, prefix, is_hip):
        Library.__init__(self, path, prefix, _model_abi(is_hip))
        self.is_hip = is_hip


_loaded = {}


def _pin_hip_runtime():
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64; if both that copy
    and /opt/rocm's get loaded, the second one sees no device and streams / device pointers cannot be
    shared.  When torch is installed, load ITS runtime first (by path, so the order of `import torch`
    and of this call does not matter): libumpa_hip.so's DT_NEEDED libamdhip64.so.7 then resolves to
    the already-loaded object.  A host without torch (C, C++, cgo ...) simply gets /opt/rocm's."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


def hip():
    """The product library.  Raises if it is not built; never substitutes anything else."""
    if "hip" not in _loaded:
        _pin_hip_runtime()
        _loaded["hip"] = Native(HIP_LIB_PATH, "umpa_hip_", True)
    return _loaded["hip"]


def _satellite(name, table):
    """``libumpa_<name>.so``, loaded at first use from ``<NAME>_LIB_PATH``, after the product library it links or works on.
    Raises if it is not built."""
    if name not in _loaded:
        hip()
        _loaded[name] = Library(globals()[name.upper() + "_LIB_PATH"], "umpa_%s_" % name, table)
    return _loaded[name]


# One table per satellite library: every symbol its header declares, with its signature.

# include/umpa_grid.h: the exhaustive grid search and the cost volume, on models of libumpa_hip.so
GRID_LIB_PATH = os.path.join(_HERE, "libumpa_grid.so")
GRID_MIN_K, GRID_MAX_K = 1, 8                                    # UMPA_GRID_MAX_BASINS
GRID_TRACK_NEAREST, GRID_TRACK_PENALTY = 0, 1                    # UMPA_GRID_TRACK_*
_GRID_ABI = {
    "match_region": (_int, _model_abi(True)["match_region"][1]),
    "cost_volume": (_int, [_vp] + [_int] * 6 + [_vp] * 3 + [_int, _vp]),
    "basins": (_int, [_vp] + [_int] * 7 + [_vp] * 10 + [_int, _vp]),
    "track": (_int, [_vp] + [_int] * 6 + [_vp] * 2 + [_int, _dbl, _dbl] + [_vp] * 12 + [_int, _vp]),
    "last_error": (C.c_char_p, []),
}
# umpa_grid_wide_<name>: the sibling's arguments with `int b` after N1 (the seventh argument)
GRID_MAX_WIDEN = 8                                               # UMPA_GRID_MAX_WIDEN
for _name in ("match_region", "cost_volume", "basins", "track"):
    _GRID_ABI["wide_" + _name] = (_int, _GRID_ABI[_name][1][:7] + [_int] + _GRID_ABI[_name][1][7:])
# umpa_grid_levels_track: the model and the region, the level list, track's mode, lam and radius, tol, the twelve per-level
# arrays, the twelve selected ones, level and halfwidth
GRID_MAX_LEVELS = 4                                              # UMPA_GRID_MAX_LEVELS
GRID_LEVEL_WIDTHS = (1, 2, 4, 8)
_GRID_ABI["levels_track"] = (_int, [_vp] + [_int] * 6 + [_int, _vp, _int, _dbl, _dbl, _vp] + [_vp] * 26 + [_int, _vp])
# umpa_grid_sequence: the model and the region, prev, lam, trunc, next, the nine maps of track, total, cost0 and moved
GRID_SEQUENCE_MIN_MS, GRID_SEQUENCE_MAX_MS = 2, 8                # the search ranges umpa_grid_sequence admits
_GRID_ABI["sequence"] = (_int, [_vp] + [_int] * 6 + [_vp, _dbl, _dbl, _vp] + [_vp] * 12 + [_int, _vp])
# umpa_grid_set_masked: the model, on / off (the per-model switch that admits a masked model to the calls above)
_GRID_ABI["set_masked"] = (_int, [_vp, _int])
# umpa_grid_set_general: the model, 0 / 1 / 3 (the per-model switch of the general table: what no tiled path takes whole)
_GRID_ABI["set_general"] = (_int, [_vp, _int])
# umpa_grid_uncertainty: the model and the region, shift, moments (or NULL), unit, s2, dof, valid
GRID_SIGMA_PLANES = (17, 50)                                     # UMPA_GRID_SIGMA_PLANES_PLAIN, _DF: a model with masks
_GRID_ABI["uncertainty"] = (_int, [_vp] + [_int] * 6 + [_vp] * 6 + [_int, _vp])
GRID_SYMBOLS = list(_GRID_ABI)

# include/umpa_unwarp.h: detector distortion correction, stand-alone and fused into stage_sample of models of libumpa_hip.so
UNWARP_LIB_PATH = os.path.join(_HERE, "libumpa_unwarp.so")
_UNWARP_ABI = {
    "map_create": (_vp, [_int, _int, C.POINTER(C.c_float), C.POINTER(C.c_float), _int, _int]),
    "map_destroy": (None, [_vp]),
    "frames": (_int, [_vp, _vp, _int, _int, _vp, _vp, _vp, _int, _vp]),
    "attach": (_int, [_vp, _vp]),
    "last_error": (C.c_char_p, []),
}
UNWARP_SYMBOLS = list(_UNWARP_ABI)

# include/umpa_register.h: the sums of the registration distance over a box of shifts
REGISTER_LIB_PATH = os.path.join(_HERE, "libumpa_register.so")
REGISTER_MAX_SHIFT = 32
REGISTER_F_SHARED_A, REGISTER_F_SHARED_W = 256, 512
_REGISTER_ABI = {
    "sums": (_int, [_vp, _vp, _vp] + [_int] * 7 + [_vp] * 3 + [_int, _int, _vp]),
    "last_error": (C.c_char_p, []),
}
REGISTER_SYMBOLS = list(_REGISTER_ABI)

# include/umpa_integrate.h: weighted least-squares phase integration
INTEGRATE_LIB_PATH = os.path.join(_HERE, "libumpa_integrate.so")
INTEGRATE_F_NO_TAIL, INTEGRATE_F_JACOBI, INTEGRATE_F_DEBUG = 256, 512, 1024
INTEGRATE_CONVERGED, INTEGRATE_MAXITER, INTEGRATE_BREAKDOWN = 0, 1, 2
INTEGRATE_CHECK_EVERY = 8
_INTEGRATE_ABI = {
    "solve": (_int, [_vp] * 3 + [_int] * 3 + [_dbl, _int, _dbl] + [_vp] * 4 + [_int, _int, _vp]),
    "vcycle": (_int, [_vp] * 3 + [_int] * 4 + [_vp]),
    "last_error": (C.c_char_p, []),
}
INTEGRATE_SYMBOLS = list(_INTEGRATE_ABI)

# include/umpa_ddf.h: the whole-image blur and the candidate fold of the directional dark-field search
DDF_LIB_PATH = os.path.join(_HERE, "libumpa_ddf.so")
DDF_TAPS, DDF_HALF, DDF_MAX_FRAMES = 17, 8, 32
_DDF_ABI = {
    "kernel": (_int, [_dbl] * 3 + [_vp]),
    "blur": (_int, [_vp, _vp] + [_int] * 3 + [_vp, _int, _int, _vp]),
    "fold": (_int, [_int, C.c_longlong] + [_vp] * 11 + [_int, _int, _vp]),
    "last_error": (C.c_char_p, []),
}
DDF_SYMBOLS = list(_DDF_ABI)

# include/umpa_smooth.h: path aggregation over a cost volume and the per-pixel selection
SMOOTH_LIB_PATH = os.path.join(_HERE, "libumpa_smooth.so")
SMOOTH_MIN_U, SMOOTH_MAX_U, SMOOTH_ALL_DIRS = 3, 15, 0xFF
_SMOOTH_ABI = {
    "aggregate": (_int, [_vp] + [_int] * 3 + [_dbl] * 2 + [_int] + [_vp] * 5 + [_int, _int, _vp]),
    "workspace_bytes": (C.c_longlong, [_int] * 4),
    "last_error": (C.c_char_p, []),
}
SMOOTH_SYMBOLS = list(_SMOOTH_ABI)

# include/umpa_sigma.h: the covariance of a matched shift and the noise estimate from the residual
SIGMA_LIB_PATH = os.path.join(_HERE, "libumpa_sigma.so")
SIGMA_MAX_NW, SIGMA_PLANES, SIGMA_SKIP = 8, (16, 34), -2 ** 31
_SIGMA_ABI = {
    "region": (_int, [_vp, _vp] + [_int] * 3 + [_vp] + [_int] * 9 + [_vp] * 6 + [_int, _int, _vp]),
    "solve": (_int, [_vp, _int, _int, C.c_longlong, _dbl] + [_vp] * 4 + [_int, _int, _vp]),
    "last_error": (C.c_char_p, []),
}
SIGMA_SYMBOLS = list(_SIGMA_ABI)


def grid():
    return _satellite("grid", _GRID_ABI)


def unwarp():
    return _satellite("unwarp", _UNWARP_ABI)


def register():
    return _satellite("register", _REGISTER_ABI)


def integrate():
    return _satellite("integrate", _INTEGRATE_ABI)


def ddf():
    return _satellite("ddf", _DDF_ABI)


def smooth():
    return _satellite("smooth", _SMOOTH_ABI)


def sigma():
    return _satellite("sigma", _SIGMA_ABI)


def host_device(device):
    """The device index of a call on host arrays: ``device``, or the package's default for ``None``."""
    if device is None:
        from . import model
        return model._default_device()
    return int(device)


class Side:
    """The side a binding call is on, decided once from its arrays (``None`` entries are skipped) and its ``device=``
    keyword: host arrays, which the library copies to ``device`` and back, or HIP tensors, which it works on where they
    lie, on the caller's current stream.  The first array decides; with ``mixed`` (a module's refusal text) a call that
    has arrays of both sides is refused with it.

    ``on_device`` is for the few lines that differ per side on purpose (host arrays are converted where a tensor of a
    wrong dtype is refused).  Allocation, pointers and the end of the native call are spelled here only."""

    def __init__(self, *arrays, device=None, mixed=None):
        self._arrays = [a for a in arrays if a is not None]
        sides = [hasattr(a, "data_ptr") for a in self._arrays]
        if mixed is not None and any(sides) and not all(sides):
            raise ValueError(mixed)
        self.on_device, self._device = sides[0], device

    def empty(self, shape, dtype):
        """An uninitialised output of a numpy ``dtype`` on the call's side (on the first tensor's device)."""
        import numpy as np
        if not self.on_device:
            return np.empty(shape, dtype=dtype)
        import torch
        return torch.empty(tuple(shape), dtype=getattr(torch, np.dtype(dtype).name), device=self._arrays[0].device)

    @staticmethod
    def ptr(a):
        """The address of an array or a tensor; ``None`` for ``None``.  (Per array, not per side: the small host arrays
        some calls take or fill beside tensors -- a window, iteration counts -- go through here too.)"""
        if a is None:
            return None
        return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data

    def tail(self, flags=0):
        """``(device, flags, stream)``, the last three arguments of every satellite call.  For tensors this is where they
        are checked: contiguous and on one HIP device, whose index and current stream the call gets with ``F_DEVICE_IO``."""
        if not self.on_device:
            return host_device(self._device), flags, None
        import torch
        d = self._arrays[0].device
        for t in self._arrays:
            if not t.is_contiguous() or not t.is_cuda or t.device != d:
                raise ValueError("device arrays must be contiguous HIP tensors on one device")
        return d.index if d.index is not None else torch.cuda.current_device(), F_DEVICE_IO | flags, torch.cuda.current_stream(d).cuda_stream


ROWS_FN = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_void_p)       # umpa_hip_rows_fn


def pinned_empty(shape, dtype, zero=False):
    """A numpy array in page-locked host memory from the library's pool (``umpa_hip_host_alloc``): the result maps of
    the host-array API are downloaded into such arrays at PCIe rate.  The block goes back to the pool when the last
    view of the array is gone.  Falls back to an ordinary array if pinning fails (the download is then staged)."""
    import weakref
    import numpy as np
    lib = hip()
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    ptr = lib.host_alloc(max(n, 1))
    if not ptr:
        return (np.zeros if zero else np.empty)(shape, dtype=dt)
    buf = (C.c_char * max(n, 1)).from_address(ptr)
    weakref.finalize(buf, lib.host_free, ptr)
    a = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)
    if zero:
        a[...] = 0
    return a


class FrameSet:
    """Pointer tables for a list of frames (host ndarrays or CUDA/HIP torch tensors)."""

    def __init__(self, frames):
        self.keep = frames
        n = len(frames)
        self.table = (_dp * n)()
        for k, a in enumerate(frames):
            if hasattr(a, "data_ptr"):
                self.table[k] = C.cast(C.c_void_p(a.data_ptr()), _dp)
            else:
                self.table[k] = a.ctypes.data_as(_dp)

