"""The diagnostic build (liblidar_amd_diag.so, `make diag`) for the tests: the product library plus its
testing aids (lidar_debug_fill_workspace / _poison_workspace / _workspace_info / _set_epoch / _voxel_inject),
which the product ABI does not export.

Two ways in:

* ``DiagVoxel`` loads it beside the product library and keeps a handle of its own for the batched voxel path.
* ``diag_library()`` is a context manager that makes the *package* run on it: every package call reaches the
  library through ``nat.load_library()`` / ``nat.call()`` / ``nat.handle()``, so swapping ``nat._lib`` and the
  calling thread's ``nat._tls.handles`` for the diagnostic library and a fresh handle table runs the Python
  wrappers unchanged on the diagnostic build, with ``poison()`` and ``info()`` acting on the very handle the
  wrappers use.  On exit (also on an exception) it synchronises, destroys the handles it created and puts the
  product library and the original handles back.

``diag_library()`` is for a single-threaded test: ``nat._lib`` is swapped for the whole process, so any other
thread that called the package while the context is live (density_stream's lane threads, for instance) would reach
the diagnostic library with handles the product library created, and the ``_active`` flag that refuses nesting is a
plain module global, not guarded by a lock.  The tests that use it start no thread inside it.
"""
import contextlib
import ctypes
import os

from lidar_ai_recommendation_software_amd import _native as nat

U64 = ctypes.c_uint64
# the testing aids: name -> argtypes (restype int)
AIDS = {
    "lidar_debug_fill_workspace": [nat.P, U64, U64, nat.P],
    "lidar_debug_poison_workspace": [nat.P, U64, U64, U64, nat.P],
    "lidar_debug_workspace_info": [nat.P, ctypes.POINTER(nat.P), ctypes.POINTER(U64), ctypes.POINTER(U64), U64, nat.P],
    "lidar_debug_set_epoch": [nat.P, ctypes.c_uint32],
    "lidar_debug_voxel_inject": [ctypes.c_int64],
}

_diag = None
_active = None  # the live DiagContext: diag_library() does not nest


def load():
    """liblidar_amd_diag.so, typed from nat.SIGNATURES plus the aids (loaded once)."""
    global _diag
    if _diag is None:
        path = os.path.join(os.path.dirname(nat.__file__), "liblidar_amd_diag.so")
        assert os.path.exists(path), "liblidar_amd_diag.so not built (__graft_entry__.build(): make diag)"
        lib = ctypes.CDLL(path)
        for name, at in nat.SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = at
            fn.restype = nat._RESTYPES.get(name, ctypes.c_int)
        for name, at in AIDS.items():
            fn = getattr(lib, name)
            fn.argtypes = at
            fn.restype = ctypes.c_int
        _diag = lib
    return _diag


def _synchronize():
    import torch
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _destroy(lib, handles):
    """lidar_destroy on every handle of the table, which is left empty (so its finaliser, which would
    reach for whatever library is current then, finds nothing)."""
    for h in list(handles.values()):
        lib.lidar_destroy(h)
    handles.clear()


class DiagContext:
    """What diag_library() yields: the swapped-in library and this thread's handle on it."""

    def __init__(self, lib, device, poison_bytes):
        self.lib, self.device, self.poison_bytes = lib, device, poison_bytes
        self.slot = 0  # the handle slot poison() and info() act on (package calls default to slot 0)

    @property
    def handle(self):
        """The handle the package's calls on (`device`, `slot`) use inside the context."""
        return nat.handle(self.device, self.slot)

    def poison(self, bound, seed):
        """Grow the handle's block to at least `poison_bytes` and fill all of it with 64-bit words in
        [1, bound] (a function of word index and seed)."""
        nat.call("lidar_debug_poison_workspace", self.handle, int(self.poison_bytes), int(bound), int(seed),
                 nat.stream_ptr())

    def info(self, bound=1):
        """(address, bytes, words of the block that match the poison predicate for `bound`); synchronises."""
        p, b, w = nat.P(), U64(0), U64(0)
        nat.call("lidar_debug_workspace_info", self.handle, ctypes.byref(p), ctypes.byref(b), ctypes.byref(w),
                 int(bound), nat.stream_ptr())
        return p.value or 0, b.value, w.value

    @contextlib.contextmanager
    def clean_handles(self):
        """Inside: the package runs on newly created handles of the same library (destroyed on exit)."""
        mine = nat._tls.handles
        nat._tls.handles = fresh = nat._ThreadHandles()
        try:
            yield
        finally:
            try:
                _synchronize()
                _destroy(self.lib, fresh)
            finally:
                nat._tls.handles = mine


@contextlib.contextmanager
def diag_library(device=0, lib=None, poison_bytes=0):
    """Run the package on the diagnostic library (or on `lib`, a stand-in) with fresh handles.
    poison_bytes: the size poison() grows the handle's block to (0: the block as it is)."""
    global _active
    if _active is not None:
        raise RuntimeError("diag_library() does not nest")
    lib = load() if lib is None else lib
    with nat._lib_lock:
        saved_lib = nat._lib
        nat._lib = lib
    had = hasattr(nat._tls, "handles")
    saved_handles = getattr(nat._tls, "handles", None)
    nat._tls.handles = fresh = nat._ThreadHandles()
    _active = ctx = DiagContext(lib, device, poison_bytes)
    try:
        yield ctx
    finally:
        try:
            _synchronize()
            _destroy(lib, fresh)
        finally:
            _active = None
            with nat._lib_lock:
                nat._lib = saved_lib
            if had:
                nat._tls.handles = saved_handles
            else:
                del nat._tls.handles


class DiagVoxel:
    """The diagnostic build loaded beside the product library, with a handle of its own, so the voxel calls
    below run the diag build's copy of the batched voxel path (csrc/voxel_batch.hip, voxel_keys.hip,
    voxel_bucket.hip: the same sources)."""

    def __init__(self, device=0):
        self.lib, self.nat = load(), nat
        hp = nat.P()
        self.call("lidar_create", int(device), ctypes.byref(hp))
        self.h = hp

    def call(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        assert rc == 0, (name, rc, self.lib.lidar_last_error())

    def voxel(self, xt, voxel):
        import torch
        B, N, _ = xt.shape
        cent = torch.empty((B, N, 3), dtype=torch.float32, device=xt.device)
        vid = torch.empty((B, N), dtype=torch.int32, device=xt.device)
        cnt = torch.empty((B, N), dtype=torch.int32, device=xt.device)
        nvox = torch.empty(B, dtype=torch.int32, device=xt.device)
        p = self.nat.ptr
        self.call("lidar_voxel_downsample_batch_f32", self.h, p(xt), B, N, float(voxel), p(vid), p(cent), p(cnt),
                  p(nvox), self.nat.stream_ptr())
        return cent, vid, cnt, nvox
