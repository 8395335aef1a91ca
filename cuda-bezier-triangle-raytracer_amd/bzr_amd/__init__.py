"""Python binding of libbzr.so (the MI355X-native Bezier-triangle ray tracer).

Thin ctypes layer over the C ABI in include/bzr.h.  The hot path
(BezierMesh::intersect, BezierTriangle::intersect, BezierLens::refract and the
refraction chain; reference/bezierMesh.cpp:206-227, bezierTriangle.cpp:123-195,
bezierLens.cpp:4-34, test.cpp:376-401) only exists as HIP kernels inside
libbzr.so: there is no Python or CPU fallback, and importing this package
raises if the library has not been built.

Arrays: rays are float32 SoA [6, n] (ox, oy, oz, dx, dy, dz); hits are
float32 [13, n] with rows t, px, py, pz, cos, b0, b1, b2, nx, ny, nz and the
uint32 bit patterns of `what` and `patch` in rows 11 and 12.  Host numpy
arrays or CUDA (HIP) torch tensors are accepted; tensors stay on the device
and the call returns before the kernels finish.  Stream: a context bound with
Context.set_stream / use_torch_stream launches there; an unbound context
launches tensor calls on torch's current stream (so the inputs torch produced
are ready and torch's caching allocator sees the outputs used in stream
order), then hands its own stream an event to wait on.
"""
from __future__ import annotations

import ctypes
import os
from contextlib import contextmanager
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent.parent
# BZR_LIBRARY: an alternative build of libbzr.so (A/B experiments); default: the in-tree build
LIB_PATH = Path(os.environ.get("BZR_LIBRARY", PKG_DIR / "lib" / "libbzr.so"))

OK = 0
HOST_PTRS, DEVICE_PTRS = 0, 1
MODE_PARITY, MODE_FAST = 0, 2
ACCEL_NONE = 4  # brute-force scan (A/B against the default BVH-culled path)
PIPELINE_STAGED = 8  # the culled path as separate kernels (traverse, bucket, Newton, resolve, finish)
PIPELINE_FUSED = 16  # the culled path as one k_trace kernel (default for dense batches; see include/bzr.h)
RAYS_AOS = 32  # rays / out_rays as [n, 6] records (the reference's Ray layout), transposed on the device
WHAT_FOLLOW0, WHAT_FOLLOW1, WHAT_FOLLOW2, WHAT_NONE, WHAT_INTERSECT = 0, 1, 2, 3, 4
LIMIT_THIS, LIMIT_NONE = 0, 1
RR_NONE, RR_INSIDE, RR_OUTSIDE = 0, 1, 2
RR_BACK = 4  # BZR_RR_BACK: trace_chain_bidir alone, the ray left the chain in front of its first lens
ENVELOPE_ELLIPSOID, ENVELOPE_TESTLENS = 0, 1
PATCH_WORDS = 66  # sizeof(bzr_patch) / 4
KERNELS = ("k_traverse", "bucket", "k_newton", "k_follow", "k_finish", "k_overflow", "k_intersect_scan",
           "k_refract_scan", "k_chain_scan", "k_patch", "k_newton_lane", "k_trace")  # BZR_KERNEL_* ids
COUNTERS = ("segments", "pairs", "follows", "overflow_rays", "lane_chunks", "node_visits", "leaf_fetches",
            "gate_tests", "newton_rounds", "rounds_odd", "runs_odd", "short_passes")  # BZR_COUNTER_* ids
HIT_FIELDS = 13

_P = ctypes.c_void_p
_U32 = ctypes.c_uint32
_I32 = ctypes.c_int32
_F = ctypes.c_float

# name -> argtypes (all return bzr_status = int32 unless listed in _RET)
_SIGS = {
    "bzr_abi_version": [],
    "bzr_last_error": [],
    "bzr_device_count": [ctypes.POINTER(_I32)],
    "bzr_ctx_create": [_I32, ctypes.POINTER(_P)],
    "bzr_ctx_destroy": [_P],
    "bzr_ctx_set_stream": [_P, _P],
    "bzr_ctx_use_own_stream": [_P],
    "bzr_ctx_get_stream": [_P, ctypes.POINTER(_P)],
    "bzr_sync": [_P],
    "bzr_ctx_timing": [_P, _I32],
    "bzr_ctx_timing_report": [_P, _P, _P],
    "bzr_ctx_counters": [_P, _I32],
    "bzr_ctx_counters_report": [_P, _P],
    "bzr_mesh_create": [_P, _P, _U32, _U32, ctypes.POINTER(_P)],
    "bzr_mesh_destroy": [_P],
    "bzr_mesh_size": [_P, ctypes.POINTER(_U32)],
    "bzr_intersect": [_P, _P, _P, _U32, _P, _U32],
    "bzr_intersect_records": [_P, _P, _P, _U32, _P, _P, _U32],
    "bzr_patch_intersect": [_P, _P, _P, _P, _P, _U32, _P, _U32],
    "bzr_refract": [_P, _P, _F, _P, _P, _U32, _U32, _P, _P, _U32],
    "bzr_trace_chain": [_P, _P, _P, _U32, _P, _U32, _P, _P, _P, _U32],
    "bzr_trace_chain_power": [_P, _P, _P, _U32, _P, _P, _U32, _P, _P, _P, _P, _U32],
    "bzr_trace_chain_spectral": [_P, _P, _P, _U32, _U32, _P, _P, _P, _U32, _P, _P, _P, _P, _U32],
    "bzr_trace_chain_tir": [_P, _P, _P, _U32, _U32, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, _U32],
    "bzr_trace_chain_opl": [_P, _P, _P, _U32, _U32, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, _P, _P, _U32],
    "bzr_trace_chain_media": [_P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, _P, _P, _U32],
    "bzr_trace_chain_absorb": [_P, _P, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _P, _P, _P,
                               _U32],
    "bzr_trace_chain_ghost": [_P, _P, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _U32, _U32, ctypes.c_uint64,
                              ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _P, _U32],
    "bzr_ghost_uniform": [ctypes.c_uint64, ctypes.c_uint64, _U32, _U32, _P],
    "bzr_trace_chain_bidir": [_P, _P, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _U32, _U32, ctypes.c_uint64,
                              ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, _U32],
    "bzr_bidir_uniform": [ctypes.c_uint64, ctypes.c_uint64, _U32, _P],
    "bzr_illuminate_bidir": [_P, _P, _P, _P, _P, _P, _U32, _U32, _P, ctypes.c_uint64, _P, _P, _U32, ctypes.c_uint64, _P, _P,
                             _P, _P, _P, _P, _P, _P, _P, _P, _P, _U32, _P, _P, _P, _P, _P, _P],
    "bzr_trace_chain_coated": [_P, _P, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _U32, _U32, ctypes.c_uint64,
                               ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _U32],
    "bzr_illuminate_coated": [_P, _P, _P, _P, _P, _P, _U32, _U32, _P, ctypes.c_uint64, _P, _P, _U32, ctypes.c_uint64, _P, _P,
                              _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _U32, _P, _P, _P, _P, _P, _P],
    "bzr_coat_transmittance": [_P, ctypes.c_float, _P],
    "bzr_coating_reflectance": [ctypes.c_double, ctypes.c_double, _P, _P, _U32, ctypes.c_double, _P],
    "bzr_absorption_from_transmittance": [_P, _U32, ctypes.c_double, _P],
    "bzr_dispersion_index": [_I32, _P, _U32, _P, _U32, _P],
    "bzr_trace_tiled": [_P, _U32, _P, _P, _U32, _P, _U32, _U32, _P, _P, _P, _U32],
    "bzr_tiled_create": [_P, _U32, _U32, _U32, _U32, _I32, ctypes.POINTER(_P)],
    "bzr_tiled_destroy": [_P],
    "bzr_tiled_info": [_P, _P, _P, _P],
    "bzr_tiled_set_rays": [_P, _P, _U32],
    "bzr_tiled_share_rays": [_P, _U32, ctypes.POINTER(_P)],
    "bzr_tiled_trace": [_P, _P, _P, _U32, _P, _P, _P, _U32],
    "bzr_tiled_stream": [_P, ctypes.POINTER(_P)],
    "bzr_tiled_sync": [_P],
    "bzr_tiled_set_layout": [_P, _I32, _U32],
    "bzr_tiled_calibrate": [_P, _P, _P, _U32, _U32, ctypes.POINTER(_U32)],
    "bzr_mesh_interpolate": [_P, _P, _I32, _P, _U32],
    "bzr_emit": [_P, _P, ctypes.c_uint64, _U32, _P, _P, _U32],
    "bzr_illuminate": [_P, _P, _P, _U32, _P, ctypes.c_uint64, _P, _P, _P, _U32],
    "bzr_illuminate_power": [_P, _P, _P, _U32, _P, ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _U32],
    "bzr_illuminate_spectral": [_P, _P, _P, _U32, _U32, _P, ctypes.c_uint64, _P, _P, _P, _P, _P, _P, _U32],
    "bzr_illuminate_tir": [_P, _P, _P, _U32, _U32, _P, ctypes.c_uint64, _P, _P, _U32, _P, _P, _P, _P, _P, _P, _P, _P,
                           _U32],
    "bzr_illuminate_media": [_P, _P, _P, _P, _P, _P, _U32, _U32, _P, ctypes.c_uint64, _P, _P, _U32, _P, _P, _P, _P, _P,
                             _P, _P, _P, _U32],
    "bzr_farfield_bin": [_P, _P, _P, _P, _P, _P, _U32, _U32, _P, _P, _P, _P, _U32],
    "bzr_illuminate_farfield": [_P, _P, _P, _P, _P, _P, _U32, _U32, _P, ctypes.c_uint64, _P, _P, _U32, _P, _P, _P, _P, _P,
                                _P, _P, _P, _U32, _P, _P, _P, _P, _P, _P],
    "bzr_illuminate_ghost": [_P, _P, _P, _P, _P, _P, _U32, _U32, _P, ctypes.c_uint64, _P, _P, _U32, ctypes.c_uint64, _P,
                             _P, _P, _P, _P, _P, _P, _P, _U32, _P, _P, _P, _P, _P, _P],
    "bzr_farfield_cell": [_P, _P, _P],
    "bzr_farfield_directions": [_P, _P, _P, _P],
    "bzr_farfield_intensity": [_P, _P, _U32, ctypes.c_double, _P],
    "bzr_debug_farfield_cells": [_P, _P, _U32, _P],
    "bzr_mesh_bounding_sphere": [_P, _P],
    "bzr_trimesh_create": [ctypes.POINTER(_P)],
    "bzr_trimesh_destroy": [_P],
    "bzr_trimesh_copy": [_P, ctypes.POINTER(_P)],
    "bzr_trimesh_size": [_P, ctypes.POINTER(_U32)],
    "bzr_trimesh_get": [_P, _P],
    "bzr_trimesh_set": [_P, _P, _U32],
    "bzr_trimesh_make_solid_of_revolution": [_P, _I32, _I32, _I32, _F, _F, _F],
    "bzr_trimesh_make_ellipsoid": [_P, _I32, _I32, _F, _F, _F],
    "bzr_trimesh_read_stl": [_P, ctypes.c_char_p],
    "bzr_trimesh_write_stl": [_P, ctypes.c_char_p],
    "bzr_trimesh_transform": [_P, _P, _P],
    "bzr_trimesh_split": [_P, _I32],
    "bzr_trimesh_split_maxside": [_P, _F],
    "bzr_trimesh_standardize_vertices": [_P],
    "bzr_trimesh_standardize_normals": [_P],
    "bzr_trimesh_neighbours": [_P, _P, _P],
    "bzr_bezier_build": [_P, _P],
    "bzr_bezier_split_thick": [_P, _P],
    "bzr_bezier_interpolate": [_P, _I32, _P],
    "bzr_pack_frame": [_P, _I32, _P, _P, _P, _U32, _U32, _U32, _P],
    "bzr_debug_unit": [_P, _P, _U32, _P],
    "bzr_debug_div_heights": [_P, _P, _U32, _P],
    "bzr_debug_bundle_setup": [_P, _P, _P, _U32, _P],
    "bzr_debug_pass_order": [_P, _P, _P, _U32, _P],
    "bzr_debug_fast_unit": [_P, _P, _U32, _P],
    "bzr_debug_wave_clock": [_P, _P, _U32],
    "bzr_debug_wave_clock_rate": [_P, _P, _U32],
    "bzr_debug_chunk_plan": [ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(_U32), ctypes.POINTER(_U32)],
    "bzr_debug_chunk_cap": [_P, _U32, ctypes.POINTER(_U32)],
    "bzr_debug_fresnel": [_P, _P, _U32, _P],
    "bzr_debug_attenuation": [_P, _P, _U32, _P],
    "bzr_debug_coat_transmittance": [_P, _P, _U32, _P],
    "bzr_debug_farfield_rounds": [_P, _I32],
}
# entry points added without an ABI bump: an explicitly chosen earlier build (BZR_LIBRARY) may lack them
_ADDED = ("bzr_trace_chain_power", "bzr_illuminate_power", "bzr_trace_chain_spectral", "bzr_illuminate_spectral",
          "bzr_dispersion_index", "bzr_trace_chain_tir", "bzr_illuminate_tir", "bzr_trace_chain_opl",
          "bzr_trace_chain_media", "bzr_trace_chain_absorb", "bzr_absorption_from_transmittance",
          "bzr_illuminate_media", "bzr_debug_attenuation", "bzr_farfield_bin", "bzr_illuminate_farfield",
          "bzr_farfield_cell", "bzr_farfield_directions", "bzr_farfield_intensity", "bzr_debug_farfield_cells",
          "bzr_trace_chain_ghost", "bzr_ghost_uniform", "bzr_illuminate_ghost", "bzr_trace_chain_bidir",
          "bzr_bidir_uniform", "bzr_illuminate_bidir", "bzr_trace_chain_coated", "bzr_illuminate_coated",
          "bzr_coat_transmittance", "bzr_coating_reflectance")
_RET = {"bzr_last_error": ctypes.c_char_p, "bzr_abi_version": _I32}

_lib = None


class BzrError(RuntimeError):
    pass


def lib():
    """Load libbzr.so (raises BzrError if it has not been built).

    PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64.  If libbzr were loaded first it
    would bind /opt/rocm's copies and torch would then load a second HIP runtime into the process
    (torch reports "No HIP GPUs are available").  Importing torch first (when installed) makes
    libbzr bind the runtime torch already loaded: one HIP runtime per process."""
    global _lib
    if _lib is None:
        if os.environ.get("BZR_NO_TORCH_PRELOAD") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        if not LIB_PATH.exists():
            raise BzrError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        handle = ctypes.CDLL(str(LIB_PATH))
        for name, args in _SIGS.items():
            if (os.environ.get("BZR_LIBRARY") and (name.startswith("bzr_debug_") or name in _ADDED)
                    and not hasattr(handle, name)):
                continue  # an explicitly chosen other build (A/B against an earlier round): its debug hooks may differ
            fn = getattr(handle, name)
            fn.argtypes = args
            fn.restype = _RET.get(name, _I32)
        _lib = handle
    return _lib


def exported_symbols():
    return list(_SIGS)


def _check(status: int):
    if status != OK:
        msg = lib().bzr_last_error().decode(errors="replace")
        raise BzrError(f"libbzr status {status}: {msg}")


def device_count() -> int:
    c = _I32(0)
    _check(lib().bzr_device_count(ctypes.byref(c)))
    return c.value


# --------------------------------------------------------------- buffers
def _is_tensor(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


class _Buf:
    """Pointer + residency of a numpy array or a torch tensor."""

    def __init__(self, x, dtype, writable=False):
        if x is None:
            self.ptr, self.device, self.keep = None, None, None
            return
        if _is_tensor(x):
            if not x.is_contiguous():
                raise BzrError("tensor arguments must be contiguous")
            want = {np.float32: "torch.float32", np.uint32: "torch.uint32", np.int32: "torch.int32",
                    np.uint64: "torch.uint64", np.uint8: "torch.uint8"}
            same_bits = {np.uint32: "torch.int32", np.uint64: "torch.int64"}
            if str(x.dtype) not in (want[dtype], same_bits.get(dtype, want[dtype])):
                raise BzrError(f"tensor dtype {x.dtype} where {want[dtype]} is expected")
            self.ptr, self.device, self.keep = x.data_ptr(), bool(x.is_cuda), x
        else:
            a = np.asarray(x)
            if a.dtype != dtype or not a.flags["C_CONTIGUOUS"]:
                if writable:
                    raise BzrError(f"output array must be C-contiguous {np.dtype(dtype).name}")
                a = np.ascontiguousarray(a, dtype=dtype)
            self.ptr, self.device, self.keep = a.ctypes.data, False, a


def _residency(*bufs) -> int:
    flags = {b.device for b in bufs if b.device is not None}
    if len(flags) != 1:
        raise BzrError("mix of host and device buffers in one call")
    return DEVICE_PTRS if flags.pop() else HOST_PTRS


@contextmanager
def _stream_for(ctx: "Context", residency: int):
    """Device-buffer calls on an unbound context run on torch's current stream: the torch-made inputs are
    ready there and the outputs are used in that stream's order (torch's caching allocator relies on
    it).  The context's own stream is then ordered after them (event hand-off, no host wait)."""
    if residency == DEVICE_PTRS and not ctx.bound:
        import torch

        _check(lib().bzr_ctx_set_stream(ctx.handle, torch.cuda.current_stream(ctx.device).cuda_stream or None))
        try:
            yield
        finally:
            _check(lib().bzr_ctx_use_own_stream(ctx.handle))
    else:
        yield


# --------------------------------------------------------------- context
class Context:
    """A HIP device + stream (bzr_ctx)."""

    def __init__(self, device: int = 0):
        h = _P()
        _check(lib().bzr_ctx_create(device, ctypes.byref(h)))
        self.handle = h
        self.device = device
        self.bound = False  # launching on a caller stream (set_stream / use_torch_stream)

    def set_stream(self, stream_ptr: int | None):
        """Launch on this hipStream_t (0 / None = the HIP null stream); None-safe.  The stream must stay
        alive while bound (include/bzr.h bzr_ctx_set_stream)."""
        _check(lib().bzr_ctx_set_stream(self.handle, stream_ptr or None))
        self.bound = True

    def use_own_stream(self):
        _check(lib().bzr_ctx_use_own_stream(self.handle))
        self.bound = False

    def use_torch_stream(self, stream=None):
        """Launch on a torch stream (default: torch's current stream, which may be the null stream),
        so torch ops and torch.cuda.Event timing order with the kernels."""
        import torch

        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.set_stream(s.cuda_stream)

    def sync(self):
        _check(lib().bzr_sync(self.handle))

    def timing(self, enable: bool = True):
        """Bracket every launch with hipEvents on this context's stream (bzr_ctx_timing)."""
        _check(lib().bzr_ctx_timing(self.handle, int(bool(enable))))

    def timing_report(self) -> dict:
        """{kernel name: (total ms, launches)} since the last report (synchronises)."""
        ms = np.zeros(len(KERNELS), np.float32)
        calls = np.zeros(len(KERNELS), np.uint32)
        _check(lib().bzr_ctx_timing_report(self.handle, ms.ctypes.data, calls.ctypes.data))
        return {k: (float(ms[i]), int(calls[i])) for i, k in enumerate(KERNELS) if calls[i]}

    def counters(self, enable: bool = True):
        """Enable/disable the culled path's device work counters (see counters_report)."""
        _check(lib().bzr_ctx_counters(self.handle, 1 if enable else 0))

    def counters_report(self) -> dict:
        """{segments, pairs, follows, overflow_rays} accumulated since the last report (synchronises)."""
        out = np.zeros(len(COUNTERS), np.uint64)
        _check(lib().bzr_ctx_counters_report(self.handle, out.ctypes.data))
        return {k: int(out[i]) for i, k in enumerate(COUNTERS)}

    def close(self):
        if getattr(self, "handle", None):
            lib().bzr_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceMesh:
    """Immutable device copy of a patch array (bzr_mesh): float32 [n, 66] records."""

    def __init__(self, ctx: Context, patches: np.ndarray):
        p = np.ascontiguousarray(patches, dtype=np.float32).reshape(-1, PATCH_WORDS)
        h = _P()
        _check(lib().bzr_mesh_create(ctx.handle, p.ctypes.data if len(p) else None, len(p), PATCH_WORDS * 4,
                                     ctypes.byref(h)))
        self.handle, self.ctx, self.n = h, ctx, len(p)

    def close(self):
        if getattr(self, "handle", None):
            lib().bzr_mesh_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _n_of(rays, mode=0) -> int:
    """Rays in a batch: [6, n] rows, or [n, 6] records when mode has RAYS_AOS."""
    shape = tuple(rays.shape)
    if mode & RAYS_AOS:
        if len(shape) != 2 or shape[1] != 6:
            raise BzrError(f"RAYS_AOS rays must be [n, 6], got {shape}")
        return int(shape[0])
    if len(shape) != 2 or shape[0] != 6:
        raise BzrError(f"rays must be [6, n], got {shape}")
    return int(shape[1])


def _empty_like(rays, rows, dtype, mode=0):
    n = _n_of(rays, mode)
    shape = ((n, 6) if mode & RAYS_AOS else (6, n)) if rows == 6 else ((rows, n) if rows else (n,))
    if _is_tensor(rays):
        import torch

        tdt = {np.float32: torch.float32, np.uint32: torch.int32}[dtype]
        return torch.empty(shape, dtype=tdt, device=rays.device)
    return np.empty(shape, dtype=dtype)


def intersect(ctx: Context, mesh: DeviceMesh, rays, out=None, mode=MODE_PARITY):
    """BezierMesh::intersect over a batch -> hits [13, n].  mode |= ACCEL_NONE for the brute-force scan; mode |=
    RAYS_AOS for [n, 6] ray records."""
    n = _n_of(rays, mode)
    out = _empty_like(rays, HIT_FIELDS, np.float32, mode) if out is None else out
    r, o = _Buf(rays, np.float32), _Buf(out, np.float32, True)
    res = _residency(r, o)
    with _stream_for(ctx, res):
        _check(lib().bzr_intersect(ctx.handle, mesh.handle, r.ptr, n, o.ptr, res | mode))
    return out


HIT_RECORD_WORDS = 13  # bzr_hit_record: valid, point xyz, cos, distance, bary xyz, normal xyz, what


def intersect_records(ctx: Context, mesh: DeviceMesh, rays, records=None, patch=None, mode=MODE_PARITY):
    """bzr_intersect_records: the hits as the reference's BezierIntersection records -> (records uint32 [n, 13]
    (view float words with .view(float32)), patch [n]).  Same values as intersect()'s rows."""
    n = _n_of(rays, mode)
    if records is None and _is_tensor(rays):
        import torch

        records = torch.empty((n, HIT_RECORD_WORDS), dtype=torch.int32, device=rays.device)
    elif records is None:
        records = np.empty((n, HIT_RECORD_WORDS), np.uint32)
    patch = _empty_like(rays, 0, np.uint32, mode) if patch is None else patch
    r, o, p_ = _Buf(rays, np.float32), _Buf(records, np.uint32, True), _Buf(patch, np.uint32, True)
    res = _residency(r, o, p_)
    with _stream_for(ctx, res):
        _check(lib().bzr_intersect_records(ctx.handle, mesh.handle, r.ptr, n, o.ptr, p_.ptr, res | mode))
    return records, patch


def patch_intersect(ctx: Context, mesh: DeviceMesh, patch_index, limit, rays, out=None, mode=MODE_PARITY):
    """BezierTriangle::intersect for (patch, ray, limit) triples -> hits [13, n]; mode MODE_FAST: the Newton stage in
    fast arithmetic after the exact gate."""
    n = _n_of(rays)
    out = _empty_like(rays, HIT_FIELDS, np.float32) if out is None else out
    i, l_ = _Buf(patch_index, np.uint32), _Buf(limit, np.uint32)
    r, o = _Buf(rays, np.float32), _Buf(out, np.float32, True)
    res = _residency(i, l_, r, o)
    with _stream_for(ctx, res):
        _check(lib().bzr_patch_intersect(ctx.handle, mesh.handle, i.ptr, l_.ptr, r.ptr, n, o.ptr, res | mode))
    return out


def refract(ctx: Context, mesh: DeviceMesh, ri: float, rays, expected=None, expected_all=RR_INSIDE,
            out_rays=None, out_status=None, mode=MODE_PARITY):
    """BezierLens::refract over a batch -> (rays [6, n], status [n]); RAYS_AOS in mode: rays [n, 6] both ways."""
    n = _n_of(rays, mode)
    out_rays = _empty_like(rays, 6, np.float32, mode) if out_rays is None else out_rays
    out_status = _empty_like(rays, 0, np.uint32, mode) if out_status is None else out_status
    r, e = _Buf(rays, np.float32), _Buf(expected, np.uint32)
    o, s = _Buf(out_rays, np.float32, True), _Buf(out_status, np.uint32, True)
    res = _residency(r, o, s, *([e] if expected is not None else []))
    with _stream_for(ctx, res):
        _check(lib().bzr_refract(ctx.handle, mesh.handle, float(ri), r.ptr, e.ptr, int(expected_all), n, o.ptr, s.ptr,
                                 res | mode))
    return out_rays, out_status


def trace_chain(ctx: Context, lenses, ri, rays, out_rays=None, out_status=None, out_segments=None, mode=MODE_PARITY):
    """Refraction chain through `lenses` (list of DeviceMesh) -> (rays [6, n], status [n], segments [n]);
    RAYS_AOS in mode: rays [n, 6] both ways."""
    n = _n_of(rays, mode)
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    ris = (_F * nl)(*[float(x) for x in ri])
    out_rays = _empty_like(rays, 6, np.float32, mode) if out_rays is None else out_rays
    out_status = _empty_like(rays, 0, np.uint32, mode) if out_status is None else out_status
    out_segments = _empty_like(rays, 0, np.uint32, mode) if out_segments is None else out_segments
    r = _Buf(rays, np.float32)
    o, s, g = _Buf(out_rays, np.float32, True), _Buf(out_status, np.uint32, True), _Buf(out_segments, np.uint32, True)
    res = _residency(r, o, s, g)
    with _stream_for(ctx, res):
        _check(lib().bzr_trace_chain(ctx.handle, ctypes.cast(handles, _P), ctypes.cast(ris, _P), nl, r.ptr, n, o.ptr,
                                     s.ptr, g.ptr, res | mode))
    return out_rays, out_status, out_segments


def trace_chain_power(ctx: Context, lenses, ri, rays, weight=None, out_rays=None, out_weight=None, out_status=None,
                      out_segments=None, mode=MODE_PARITY):
    """trace_chain with the rays' power -> (rays, weight [n], status [n], segments [n]).  weight [n] float32 is the
    power the rays start with (None: 1.0 each); out_weight[i] = weight[i] x the Fresnel transmittance of each successful
    refraction of ray i (bzr.h bzr_trace_chain_power).  out_weight may be `weight` itself."""
    n = _n_of(rays, mode)
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    ris = (_F * nl)(*[float(x) for x in ri])
    out_rays = _empty_like(rays, 6, np.float32, mode) if out_rays is None else out_rays
    out_weight = _empty_like(rays, 0, np.float32, mode) if out_weight is None else out_weight
    out_status = _empty_like(rays, 0, np.uint32, mode) if out_status is None else out_status
    out_segments = _empty_like(rays, 0, np.uint32, mode) if out_segments is None else out_segments
    r, wi = _Buf(rays, np.float32), _Buf(weight, np.float32)
    o, w = _Buf(out_rays, np.float32, True), _Buf(out_weight, np.float32, True)
    s, g = _Buf(out_status, np.uint32, True), _Buf(out_segments, np.uint32, True)
    res = _residency(r, o, w, s, g, *([wi] if weight is not None else []))
    with _stream_for(ctx, res):
        _check(lib().bzr_trace_chain_power(ctx.handle, ctypes.cast(handles, _P), ctypes.cast(ris, _P), nl, r.ptr, wi.ptr,
                                           n, o.ptr, w.ptr, s.ptr, g.ptr, res | mode))
    return out_rays, out_weight, out_status, out_segments


MAX_CHANNELS = 64  # BZR_MAX_CHANNELS
DISPERSION_CAUCHY, DISPERSION_SELLMEIER = 0, 1  # BZR_DISPERSION_*


def _ri_table(ri_table, nl):
    """The index table as C-contiguous float32 [nlens, nchan] -> (array, nchan)."""
    t = np.ascontiguousarray(ri_table, dtype=np.float32)
    if t.ndim != 2 or t.shape[0] != nl:
        raise BzrError(f"ri_table must be [nlens = {nl}, nchan], got {t.shape}")
    return t, int(t.shape[1])


def trace_chain_spectral(ctx: Context, lenses, ri_table, rays, channel, weight=None, out_rays=None, out_weight=None,
                         out_status=None, out_segments=None, mode=MODE_PARITY):
    """trace_chain_power with one index per ray and lens -> (rays, weight [n], status [n], segments [n]).  ri_table
    [nlens, nchan] float32 (host) is lens l's index for channel c, channel [n] uint8 the rays' channels (host or
    device as the rays); ray i refracts at lens l with ri_table[l, channel[i]].  A ray whose channel is nchan or more
    comes back with status NONE, one segment, its ray and weight unchanged (bzr.h bzr_trace_chain_spectral)."""
    n = _n_of(rays, mode)
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    table, nchan = _ri_table(ri_table, nl)
    out_rays = _empty_like(rays, 6, np.float32, mode) if out_rays is None else out_rays
    out_weight = _empty_like(rays, 0, np.float32, mode) if out_weight is None else out_weight
    out_status = _empty_like(rays, 0, np.uint32, mode) if out_status is None else out_status
    out_segments = _empty_like(rays, 0, np.uint32, mode) if out_segments is None else out_segments
    r, c, wi = _Buf(rays, np.float32), _Buf(channel, np.uint8), _Buf(weight, np.float32)
    o, w = _Buf(out_rays, np.float32, True), _Buf(out_weight, np.float32, True)
    s, g = _Buf(out_status, np.uint32, True), _Buf(out_segments, np.uint32, True)
    res = _residency(r, c, o, w, s, g, wi)
    with _stream_for(ctx, res):
        _check(lib().bzr_trace_chain_spectral(ctx.handle, ctypes.cast(handles, _P), table.ctypes.data if table.size else None,
                                              nl, nchan, r.ptr, c.ptr, wi.ptr, n, o.ptr, w.ptr, s.ptr, g.ptr, res | mode))
    return out_rays, out_weight, out_status, out_segments


MAX_BOUNCES = 8  # BZR_MAX_BOUNCES


def trace_chain_tir(ctx: Context, lenses, ri_table, rays, channel=None, weight=None, max_bounces=4, out_rays=None,
                    out_weight=None, out_status=None, out_segments=None, out_bounces=None, mode=MODE_PARITY):
    """trace_chain_spectral with total internal reflection -> (rays, weight [n], status [n], segments [n], bounces [n]).
    A ray that cannot leave a lens (s2 >= 1 at its back surface) is mirrored inside it and traced against the same lens
    again, up to max_bounces (<= MAX_BOUNCES) times per lens; its weight is not touched.  channel None: every ray is
    channel 0.  segments counts the bounce segments too, bounces is the ray's reflections over all lenses.  With
    max_bounces = 0 the result is trace_chain_spectral's (bzr.h bzr_trace_chain_tir)."""
    n = _n_of(rays, mode)
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    table, nchan = _ri_table(ri_table, nl)
    out_rays = _empty_like(rays, 6, np.float32, mode) if out_rays is None else out_rays
    out_weight = _empty_like(rays, 0, np.float32, mode) if out_weight is None else out_weight
    out_status = _empty_like(rays, 0, np.uint32, mode) if out_status is None else out_status
    out_segments = _empty_like(rays, 0, np.uint32, mode) if out_segments is None else out_segments
    out_bounces = _empty_like(rays, 0, np.uint32, mode) if out_bounces is None else out_bounces
    r, c, wi = _Buf(rays, np.float32), _Buf(channel, np.uint8), _Buf(weight, np.float32)
    o, w = _Buf(out_rays, np.float32, True), _Buf(out_weight, np.float32, True)
    s, g, b = _Buf(out_status, np.uint32, True), _Buf(out_segments, np.uint32, True), _Buf(out_bounces, np.uint32, True)
    res = _residency(r, c, o, w, s, g, b, wi)
    with _stream_for(ctx, res):
        _check(lib().bzr_trace_chain_tir(ctx.handle, ctypes.cast(handles, _P), table.ctypes.data if table.size else None,
                                         nl, nchan, r.ptr, c.ptr, wi.ptr, n, int(max_bounces), o.ptr, w.ptr, s.ptr, g.ptr,
                                         b.ptr, res | mode))
    return out_rays, out_weight, out_status, out_segments, out_bounces


def trace_chain_opl(ctx: Context, lenses, ri_table, rays, channel=None, weight=None, opl=None, max_bounces=4,
                    out_rays=None, out_weight=None, out_status=None, out_segments=None, out_bounces=None, out_opl=None,
                    out_glass=None, mode=MODE_PARITY):
    """trace_chain_tir with the rays' optical path -> (rays, weight [n], status [n], segments [n], bounces [n], opl [n],
    glass [n]).  opl [n] float32 is the path the rays arrive with (None: 0 each; out_opl may be `opl` itself).  Every
    segment that ends in a refraction or a reflection adds its leg, the distance from the segment's origin to the hit
    point: to opl as it is in air, times the lens's index for the ray's channel in glass, where glass takes the bare
    length.  The first five outputs are trace_chain_tir's bit for bit.  out_glass=False: no glass row is computed and
    the last element is None (bzr.h bzr_trace_chain_opl)."""
    n = _n_of(rays, mode)
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    table, nchan = _ri_table(ri_table, nl)
    out_rays = _empty_like(rays, 6, np.float32, mode) if out_rays is None else out_rays
    out_weight = _empty_like(rays, 0, np.float32, mode) if out_weight is None else out_weight
    out_status = _empty_like(rays, 0, np.uint32, mode) if out_status is None else out_status
    out_segments = _empty_like(rays, 0, np.uint32, mode) if out_segments is None else out_segments
    out_bounces = _empty_like(rays, 0, np.uint32, mode) if out_bounces is None else out_bounces
    out_opl = _empty_like(rays, 0, np.float32, mode) if out_opl is None else out_opl
    if out_glass is False:
        out_glass = None
    elif out_glass is None:
        out_glass = _empty_like(rays, 0, np.float32, mode)
    r, c, wi, pi = _Buf(rays, np.float32), _Buf(channel, np.uint8), _Buf(weight, np.float32), _Buf(opl, np.float32)
    o, w = _Buf(out_rays, np.float32, True), _Buf(out_weight, np.float32, True)
    s, g, b = _Buf(out_status, np.uint32, True), _Buf(out_segments, np.uint32, True), _Buf(out_bounces, np.uint32, True)
    p, q = _Buf(out_opl, np.float32, True), _Buf(out_glass, np.float32, True)
    res = _residency(r, c, o, w, s, g, b, wi, pi, p, q)
    with _stream_for(ctx, res):
        _check(lib().bzr_trace_chain_opl(ctx.handle, ctypes.cast(handles, _P), table.ctypes.data if table.size else None,
                                         nl, nchan, r.ptr, c.ptr, wi.ptr, pi.ptr, n, int(max_bounces), o.ptr, w.ptr,
                                         s.ptr, g.ptr, b.ptr, p.ptr, q.ptr, res | mode))
    return out_rays, out_weight, out_status, out_segments, out_bounces, out_opl, out_glass


def trace_chain_media(ctx: Context, lenses, ri_table, gap_table, rays, channel=None, weight=None, opl=None, max_bounces=4,
                      out_rays=None, out_weight=None, out_status=None, out_segments=None, out_bounces=None, out_opl=None,
                      out_glass=None, mode=MODE_PARITY):
    """trace_chain_opl with a medium in front of, between and behind the lenses -> the same seven-tuple.  gap_table
    [nlens + 1, nchan] float32 (host): row l is the index in front of lens l, the last row the index behind the last
    lens; None is vacuum, and with every entry 1 the result is trace_chain_opl's bit for bit.  Going into lens l a ray
    of channel c refracts with eta = gap[l, c] / ri[l, c], coming out (and in the reflection test) with ri[l, c] /
    gap[l + 1, c]; a leg in front of a lens adds gap[l, c] x its length to opl, glass counts lens glass only.  Every
    entry must be finite and above 0 (bzr.h bzr_trace_chain_media)."""
    n = _n_of(rays, mode)
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    table, nchan = _ri_table(ri_table, nl)
    gap = None
    if gap_table is not None:
        gap = np.ascontiguousarray(gap_table, dtype=np.float32)
        if gap.shape != (nl + 1, nchan):
            raise BzrError(f"gap_table must be [nlens + 1 = {nl + 1}, nchan = {nchan}], got {gap.shape}")
    out_rays = _empty_like(rays, 6, np.float32, mode) if out_rays is None else out_rays
    out_weight = _empty_like(rays, 0, np.float32, mode) if out_weight is None else out_weight
    out_status = _empty_like(rays, 0, np.uint32, mode) if out_status is None else out_status
    out_segments = _empty_like(rays, 0, np.uint32, mode) if out_segments is None else out_segments
    out_bounces = _empty_like(rays, 0, np.uint32, mode) if out_bounces is None else out_bounces
    out_opl = _empty_like(rays, 0, np.float32, mode) if out_opl is None else out_opl
    if out_glass is False:
        out_glass = None
    elif out_glass is None:
        out_glass = _empty_like(rays, 0, np.float32, mode)
    r, c, wi, pi = _Buf(rays, np.float32), _Buf(channel, np.uint8), _Buf(weight, np.float32), _Buf(opl, np.float32)
    o, w = _Buf(out_rays, np.float32, True), _Buf(out_weight, np.float32, True)
    s, g, b = _Buf(out_status, np.uint32, True), _Buf(out_segments, np.uint32, True), _Buf(out_bounces, np.uint32, True)
    p, q = _Buf(out_opl, np.float32, True), _Buf(out_glass, np.float32, True)
    res = _residency(r, c, o, w, s, g, b, wi, pi, p, q)
    with _stream_for(ctx, res):
        _check(lib().bzr_trace_chain_media(ctx.handle, ctypes.cast(handles, _P), table.ctypes.data if table.size else None,
                                           gap.ctypes.data if gap is not None and gap.size else None, nl, nchan, r.ptr,
                                           c.ptr, wi.ptr, pi.ptr, n, int(max_bounces), o.ptr, w.ptr, s.ptr, g.ptr, b.ptr,
                                           p.ptr, q.ptr, res | mode))
    return out_rays, out_weight, out_status, out_segments, out_bounces, out_opl, out_glass


def _absorb_table(table, name, nl, nchan):
    """An absorption table [nlens, nchan] as contiguous float32, or None."""
    if table is None:
        return None
    a = np.ascontiguousarray(table, dtype=np.float32)
    if a.shape != (nl, nchan):
        raise BzrError(f"{name} must be [nlens = {nl}, nchan = {nchan}], got {a.shape}")
    return a


def _gap_table(gap_table, nl, nchan):
    if gap_table is None:
        return None
    gap = np.ascontiguousarray(gap_table, dtype=np.float32)
    if gap.shape != (nl + 1, nchan):
        raise BzrError(f"gap_table must be [nlens + 1 = {nl + 1}, nchan = {nchan}], got {gap.shape}")
    return gap


def _table_ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def trace_chain_absorb(ctx: Context, lenses, ri_table, gap_table, glass_absorb, gap_absorb, rays, channel=None, weight=None,
                       opl=None, max_bounces=4, out_rays=None, out_weight=None, out_status=None, out_segments=None,
                       out_bounces=None, out_opl=None, out_glass=None, mode=MODE_PARITY):
    """trace_chain_media with Beer-Lambert absorption along the legs -> the same seven-tuple.  glass_absorb and
    gap_absorb [nlens, nchan] float32 (host): the Napierian absorption coefficient per unit length of lens l's glass and
    of the medium in front of lens l (gap_table's row l); None is all zero, and with both zero the result is
    trace_chain_media's bit for bit.  Every leg that ends in a refraction or a reflection multiplies the weight by
    att(a x its length) ahead of the Fresnel term; only the weight depends on the two tables.  Every entry must be
    finite and not below 0 (bzr.h bzr_trace_chain_absorb)."""
    n = _n_of(rays, mode)
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    table, nchan = _ri_table(ri_table, nl)
    gap = _gap_table(gap_table, nl, nchan)
    ga, pa = _absorb_table(glass_absorb, "glass_absorb", nl, nchan), _absorb_table(gap_absorb, "gap_absorb", nl, nchan)
    out_rays = _empty_like(rays, 6, np.float32, mode) if out_rays is None else out_rays
    out_weight = _empty_like(rays, 0, np.float32, mode) if out_weight is None else out_weight
    out_status = _empty_like(rays, 0, np.uint32, mode) if out_status is None else out_status
    out_segments = _empty_like(rays, 0, np.uint32, mode) if out_segments is None else out_segments
    out_bounces = _empty_like(rays, 0, np.uint32, mode) if out_bounces is None else out_bounces
    out_opl = _empty_like(rays, 0, np.float32, mode) if out_opl is None else out_opl
    if out_glass is False:
        out_glass = None
    elif out_glass is None:
        out_glass = _empty_like(rays, 0, np.float32, mode)
    r, c, wi, pi = _Buf(rays, np.float32), _Buf(channel, np.uint8), _Buf(weight, np.float32), _Buf(opl, np.float32)
    o, w = _Buf(out_rays, np.float32, True), _Buf(out_weight, np.float32, True)
    s, g, b = _Buf(out_status, np.uint32, True), _Buf(out_segments, np.uint32, True), _Buf(out_bounces, np.uint32, True)
    p, q = _Buf(out_opl, np.float32, True), _Buf(out_glass, np.float32, True)
    res = _residency(r, c, o, w, s, g, b, wi, pi, p, q)
    with _stream_for(ctx, res):
        _check(lib().bzr_trace_chain_absorb(ctx.handle, ctypes.cast(handles, _P), table.ctypes.data if table.size else None,
                                            _table_ptr(gap), _table_ptr(ga), _table_ptr(pa), nl, nchan, r.ptr, c.ptr,
                                            wi.ptr, pi.ptr, n, int(max_bounces), o.ptr, w.ptr, s.ptr, g.ptr, b.ptr, p.ptr,
                                            q.ptr, res | mode))
    return out_rays, out_weight, out_status, out_segments, out_bounces, out_opl, out_glass


def trace_chain_ghost(ctx: Context, lenses, ri_table, gap_table, glass_absorb, gap_absorb, rays, channel=None, weight=None,
                      opl=None, max_bounces=4, ghost_seed=0, first_ray=0, out_rays=None, out_weight=None, out_status=None,
                      out_segments=None, out_bounces=None, out_opl=None, out_glass=None, mode=MODE_PARITY):
    """trace_chain_absorb with the Fresnel roulette at glass exits -> the same seven-tuple.  A ray that would refract
    out of a lens with bounce budget left draws u = ghost_uniform(ghost_seed, first_ray + i, lens, reflections so far):
    u >= T reflects it like a total reflection, u < T lets it out without the factor T.  The draws depend on the ray's
    64-bit number alone, so a call split in two (first_ray moved along) gives the same bits; max_bounces = 0 is
    trace_chain_absorb bit for bit (bzr.h bzr_trace_chain_ghost)."""
    n = _n_of(rays, mode)
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    table, nchan = _ri_table(ri_table, nl)
    gap = _gap_table(gap_table, nl, nchan)
    ga, pa = _absorb_table(glass_absorb, "glass_absorb", nl, nchan), _absorb_table(gap_absorb, "gap_absorb", nl, nchan)
    out_rays = _empty_like(rays, 6, np.float32, mode) if out_rays is None else out_rays
    out_weight = _empty_like(rays, 0, np.float32, mode) if out_weight is None else out_weight
    out_status = _empty_like(rays, 0, np.uint32, mode) if out_status is None else out_status
    out_segments = _empty_like(rays, 0, np.uint32, mode) if out_segments is None else out_segments
    out_bounces = _empty_like(rays, 0, np.uint32, mode) if out_bounces is None else out_bounces
    out_opl = _empty_like(rays, 0, np.float32, mode) if out_opl is None else out_opl
    if out_glass is False:
        out_glass = None
    elif out_glass is None:
        out_glass = _empty_like(rays, 0, np.float32, mode)
    r, c, wi, pi = _Buf(rays, np.float32), _Buf(channel, np.uint8), _Buf(weight, np.float32), _Buf(opl, np.float32)
    o, w = _Buf(out_rays, np.float32, True), _Buf(out_weight, np.float32, True)
    s, g, b = _Buf(out_status, np.uint32, True), _Buf(out_segments, np.uint32, True), _Buf(out_bounces, np.uint32, True)
    p, q = _Buf(out_opl, np.float32, True), _Buf(out_glass, np.float32, True)
    res = _residency(r, c, o, w, s, g, b, wi, pi, p, q)
    mask = (1 << 64) - 1
    with _stream_for(ctx, res):
        _check(lib().bzr_trace_chain_ghost(ctx.handle, ctypes.cast(handles, _P), table.ctypes.data if table.size else None,
                                           _table_ptr(gap), _table_ptr(ga), _table_ptr(pa), nl, nchan, r.ptr, c.ptr,
                                           wi.ptr, pi.ptr, n, int(max_bounces), int(ghost_seed) & mask,
                                           int(first_ray) & mask, o.ptr, w.ptr, s.ptr, g.ptr, b.ptr, p.ptr, q.ptr,
                                           res | mode))
    return out_rays, out_weight, out_status, out_segments, out_bounces, out_opl, out_glass


def trace_chain_bidir(ctx: Context, lenses, ri_table, gap_table, glass_absorb, gap_absorb, rays, channel=None, weight=None,
                      opl=None, max_bounces=4, ghost_seed=0, first_ray=0, axis=(1.0, 0.0, 0.0), out_rays=None,
                      out_weight=None, out_status=None, out_segments=None, out_bounces=None, out_opl=None, out_glass=None,
                      mode=MODE_PARITY):
    """The bidirectional chain -> trace_chain_ghost's seven-tuple.  The roulette runs at every surface, front surfaces
    included; a ray goes on to the neighbour lens that the surface it left faces along `axis` (the chain's forward
    direction), and ends RR_OUTSIDE behind the last lens, RR_BACK in front of the first, or RR_NONE.  max_bounces is the
    ray's budget for its whole path.  Fused, or ACCEL_NONE for the scan; PIPELINE_STAGED is refused (bzr.h
    bzr_trace_chain_bidir)."""
    n = _n_of(rays, mode)
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    table, nchan = _ri_table(ri_table, nl)
    gap = _gap_table(gap_table, nl, nchan)
    ga, pa = _absorb_table(glass_absorb, "glass_absorb", nl, nchan), _absorb_table(gap_absorb, "gap_absorb", nl, nchan)
    ax = np.ascontiguousarray(axis, np.float32)
    if ax.shape != (3,):
        raise BzrError("axis must have three components")
    out_rays = _empty_like(rays, 6, np.float32, mode) if out_rays is None else out_rays
    out_weight = _empty_like(rays, 0, np.float32, mode) if out_weight is None else out_weight
    out_status = _empty_like(rays, 0, np.uint32, mode) if out_status is None else out_status
    out_segments = _empty_like(rays, 0, np.uint32, mode) if out_segments is None else out_segments
    out_bounces = _empty_like(rays, 0, np.uint32, mode) if out_bounces is None else out_bounces
    out_opl = _empty_like(rays, 0, np.float32, mode) if out_opl is None else out_opl
    if out_glass is False:
        out_glass = None
    elif out_glass is None:
        out_glass = _empty_like(rays, 0, np.float32, mode)
    r, c, wi, pi = _Buf(rays, np.float32), _Buf(channel, np.uint8), _Buf(weight, np.float32), _Buf(opl, np.float32)
    o, w = _Buf(out_rays, np.float32, True), _Buf(out_weight, np.float32, True)
    s, g, b = _Buf(out_status, np.uint32, True), _Buf(out_segments, np.uint32, True), _Buf(out_bounces, np.uint32, True)
    p, q = _Buf(out_opl, np.float32, True), _Buf(out_glass, np.float32, True)
    res = _residency(r, c, o, w, s, g, b, wi, pi, p, q)
    mask = (1 << 64) - 1
    with _stream_for(ctx, res):
        _check(lib().bzr_trace_chain_bidir(ctx.handle, ctypes.cast(handles, _P), table.ctypes.data if table.size else None,
                                           _table_ptr(gap), _table_ptr(ga), _table_ptr(pa), nl, nchan, r.ptr, c.ptr,
                                           wi.ptr, pi.ptr, n, int(max_bounces), int(ghost_seed) & mask,
                                           int(first_ray) & mask, ax.ctypes.data, o.ptr, w.ptr, s.ptr, g.ptr, b.ptr, p.ptr,
                                           q.ptr, res | mode))
    return out_rays, out_weight, out_status, out_segments, out_bounces, out_opl, out_glass


COAT_SAMPLES = 129  # BZR_COAT_SAMPLES: a row's reflectances at the gap-side cosines i / 128


class _CoatingC(ctypes.Structure):
    """bzr_coating"""
    _fields_ = [("table", _P), ("mask", _U32)]


class Coating:
    """bzr_coating: tabulated reflectances of coated surfaces.  Coating(table, mask) takes the table
    [2 nlens, nchan, COAT_SAMPLES] float32 (surface 2 l + side: side 0 the front of lens l, 1 its back) and the mask,
    bit 2 l + side per coated surface; Coating({(lens, side): rows [nchan, COAT_SAMPLES], ...}, nlens=) builds both
    from the coated surfaces alone (bzr.h bzr_coating)."""

    def __init__(self, table, mask=None, nlens=None):
        if isinstance(table, dict):
            if nlens is None:
                raise BzrError("Coating from a dict needs nlens")
            rows = {k: np.ascontiguousarray(v, np.float32) for k, v in table.items()}
            shapes = {r.shape for r in rows.values()}
            if len(shapes) > 1 or any(len(sh) != 2 or sh[1] != COAT_SAMPLES for sh in shapes):
                raise BzrError(f"every surface's rows must be [nchan, {COAT_SAMPLES}] of one nchan")
            nchan = shapes.pop()[0] if shapes else 1
            self.table = np.zeros((2 * int(nlens), nchan, COAT_SAMPLES), np.float32)
            self.mask = 0
            for (lens, side), r in rows.items():
                if not (0 <= int(lens) < int(nlens)) or int(side) not in (0, 1):
                    raise BzrError(f"no surface ({lens}, {side}) in a chain of {nlens} lenses")
                self.table[2 * int(lens) + int(side)] = r
                self.mask |= 1 << (2 * int(lens) + int(side))
        else:
            self.table = None if table is None else np.ascontiguousarray(table, np.float32)
            self.mask = int(mask or 0)

    def _c(self, nl, nchan):
        if self.table is not None and self.table.shape != (2 * nl, nchan, COAT_SAMPLES):
            raise BzrError(f"coating table must be [2 nlens = {2 * nl}, nchan = {nchan}, {COAT_SAMPLES}], "
                           f"got {self.table.shape}")
        return _CoatingC(self.table.ctypes.data if self.table is not None else None, self.mask & 0xFFFFFFFF)


def _coating(coat, nl, nchan):
    """A Coating (or None) as a pointer argument; the structure must outlive the call, so it is returned too."""
    if coat is None:
        return None, None
    c = coat._c(nl, nchan)
    return ctypes.byref(c), c


def trace_chain_coated(ctx: Context, lenses, ri_table, gap_table, glass_absorb, gap_absorb, rays, channel=None, weight=None,
                       opl=None, max_bounces=4, ghost_seed=0, first_ray=0, axis=(1.0, 0.0, 0.0), coat=None,
                       out_rays=None, out_weight=None, out_status=None, out_segments=None, out_bounces=None, out_opl=None,
                       out_glass=None, mode=MODE_PARITY):
    """trace_chain_bidir over coated surfaces -> the same seven-tuple.  coat: a Coating, or None (no surface coated:
    trace_chain_bidir bit for bit).  On a coated surface the roulette's threshold and the budget-spent factor T come
    from the surface's row at the gap-side cosine instead of the Fresnel formula (bzr.h bzr_coating)."""
    n = _n_of(rays, mode)
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    table, nchan = _ri_table(ri_table, nl)
    gap = _gap_table(gap_table, nl, nchan)
    ga, pa = _absorb_table(glass_absorb, "glass_absorb", nl, nchan), _absorb_table(gap_absorb, "gap_absorb", nl, nchan)
    ax = np.ascontiguousarray(axis, np.float32)
    if ax.shape != (3,):
        raise BzrError("axis must have three components")
    cref, ckeep = _coating(coat, nl, nchan)
    out_rays = _empty_like(rays, 6, np.float32, mode) if out_rays is None else out_rays
    out_weight = _empty_like(rays, 0, np.float32, mode) if out_weight is None else out_weight
    out_status = _empty_like(rays, 0, np.uint32, mode) if out_status is None else out_status
    out_segments = _empty_like(rays, 0, np.uint32, mode) if out_segments is None else out_segments
    out_bounces = _empty_like(rays, 0, np.uint32, mode) if out_bounces is None else out_bounces
    out_opl = _empty_like(rays, 0, np.float32, mode) if out_opl is None else out_opl
    if out_glass is False:
        out_glass = None
    elif out_glass is None:
        out_glass = _empty_like(rays, 0, np.float32, mode)
    r, c, wi, pi = _Buf(rays, np.float32), _Buf(channel, np.uint8), _Buf(weight, np.float32), _Buf(opl, np.float32)
    o, w = _Buf(out_rays, np.float32, True), _Buf(out_weight, np.float32, True)
    s, g, b = _Buf(out_status, np.uint32, True), _Buf(out_segments, np.uint32, True), _Buf(out_bounces, np.uint32, True)
    p, q = _Buf(out_opl, np.float32, True), _Buf(out_glass, np.float32, True)
    res = _residency(r, c, o, w, s, g, b, wi, pi, p, q)
    mask = (1 << 64) - 1
    with _stream_for(ctx, res):
        _check(lib().bzr_trace_chain_coated(ctx.handle, ctypes.cast(handles, _P), table.ctypes.data if table.size else None,
                                            _table_ptr(gap), _table_ptr(ga), _table_ptr(pa), nl, nchan, r.ptr, c.ptr,
                                            wi.ptr, pi.ptr, n, int(max_bounces), int(ghost_seed) & mask,
                                            int(first_ray) & mask, ax.ctypes.data, cref, o.ptr, w.ptr, s.ptr, g.ptr, b.ptr,
                                            p.ptr, q.ptr, res | mode))
    del ckeep
    return out_rays, out_weight, out_status, out_segments, out_bounces, out_opl, out_glass


def coat_transmittance(row, mu) -> np.ndarray:
    """The coated surface's lookup on the host, the device's twin bit for bit: T = coat_t(row, mu) for every mu (a
    scalar, or an array in one call), row [COAT_SAMPLES] float32 (bzr.h bzr_coat_transmittance, bzr_debug.h
    bzr_debug_coat_transmittance)."""
    r = np.ascontiguousarray(row, np.float32)
    if r.shape != (COAT_SAMPLES,):
        raise BzrError(f"row must hold {COAT_SAMPLES} reflectances")
    m = np.asarray(mu, np.float32)
    if m.ndim == 0:
        t = ctypes.c_float()
        _check(lib().bzr_coat_transmittance(r.ctypes.data, ctypes.c_float(float(m)), ctypes.byref(t)))
        return np.float32(t.value)
    flat = np.ascontiguousarray(m).reshape(-1)
    out = np.empty(flat.size, np.float32)
    _check(lib().bzr_debug_coat_transmittance(r.ctypes.data, flat.ctypes.data, flat.size, out.ctypes.data))
    return out.reshape(m.shape)


def coating_reflectance(n_gap: float, n_glass: float, layer_index=(), layer_thickness_um=(), wavelength_um=0.55):
    """One row of a Coating on the host: the unpolarised reflectance of a lossless dielectric stack between a gap of
    index n_gap and glass of index n_glass at the gap-side cosines i / 128, float32 [COAT_SAMPLES].  Layers from the
    gap side to the glass; none is the bare Fresnel surface (bzr.h bzr_coating_reflectance)."""
    li = np.ascontiguousarray(layer_index, np.float64).ravel()
    lt = np.ascontiguousarray(layer_thickness_um, np.float64).ravel()
    if li.size != lt.size:
        raise BzrError("one thickness per layer")
    out = np.empty(COAT_SAMPLES, np.float32)
    _check(lib().bzr_coating_reflectance(float(n_gap), float(n_glass), li.ctypes.data if li.size else None,
                                         lt.ctypes.data if lt.size else None, li.size, float(wavelength_um),
                                         out.ctypes.data))
    return out


def bidir_uniform(seed: int, ray: int, segment: int) -> np.float32:
    """trace_chain_bidir's draw on the host: the 24-bit uniform of (seed, the ray's 64-bit number, the segment's ordinal
    counted from 0) (bzr.h bzr_bidir_uniform)."""
    u = ctypes.c_float()
    mask = (1 << 64) - 1
    _check(lib().bzr_bidir_uniform(int(seed) & mask, int(ray) & mask, int(segment), ctypes.byref(u)))
    return np.float32(u.value)


def ghost_uniform(seed: int, ray: int, lens: int, reflections: int) -> np.float32:
    """The roulette's draw on the host, the device's twin: a 24-bit uniform in [0, 1) for (seed, the ray's 64-bit
    number, lens 0..7, reflections in that lens so far 0..8) (bzr.h bzr_ghost_uniform)."""
    u = ctypes.c_float()
    mask = (1 << 64) - 1
    _check(lib().bzr_ghost_uniform(int(seed) & mask, int(ray) & mask, int(lens), int(reflections), ctypes.byref(u)))
    return np.float32(u.value)


def absorption_from_transmittance(internal_transmittance, thickness: float) -> np.ndarray:
    """Absorption coefficients a = -ln(T) / thickness, float32, from a catalogue's internal transmittance T at a
    thickness, per unit of the length the thickness is given in.  Host only (bzr.h bzr_absorption_from_transmittance)."""
    t = np.ascontiguousarray(internal_transmittance, np.float64)
    out = np.empty(t.shape, np.float32)
    _check(lib().bzr_absorption_from_transmittance(t.ctypes.data, t.size, float(thickness), out.ctypes.data))
    return out


def dispersion_index(model: int, coeff, wavelength_um) -> np.ndarray:
    """Refractive index at each wavelength (micrometres) from a dispersion formula, float32: DISPERSION_CAUCHY
    (coeff A, B[, C]: n = A + B / l^2 + C / l^4) or DISPERSION_SELLMEIER (coeff B1, C1, B2, C2, ...:
    n^2 = 1 + sum B_k l^2 / (l^2 - C_k)).  Host only (bzr.h bzr_dispersion_index)."""
    c = np.ascontiguousarray(coeff, np.float64).ravel()
    lam = np.ascontiguousarray(wavelength_um, np.float64)
    out = np.empty(lam.shape, np.float32)
    _check(lib().bzr_dispersion_index(int(model), c.ctypes.data, c.size, lam.ctypes.data, lam.size, out.ctypes.data))
    return out


PACK_IMAGE, PACK_RAYS, PACK_COMPACT = 0, 1, 2  # BZR_PACK_*
PACK_LAYOUTS = {"image": PACK_IMAGE, "rays": PACK_RAYS, "compact": PACK_COMPACT}


def pack_frame(ctx: Context, layout: str, rays, status, segments, packed, npad: int, cap: int = 0):
    """bzr_pack_frame: one chain frame's device outputs (rays [6, n], status [n], segments [n]) into the
    gather buffer `packed` (a CUDA tensor laid out as bzr_amd.frame's `layout`: image, rays or compact)
    on the device, no host sync.  Same bits as frame.pack / frame.pack_compact in the columns they read."""
    if layout not in PACK_LAYOUTS:
        raise ValueError(f"layout {layout!r}")
    n = int(status.shape[0])
    if int(segments.shape[0]) != n:
        raise BzrError(f"pack_frame: segments [{int(segments.shape[0])}] for status [{n}]")
    if rays is not None and tuple(rays.shape) != (6, n):
        raise BzrError(f"pack_frame: rays must be [6, {n}], got {tuple(rays.shape)}")
    # the device writes this many floats into `packed` (include/bzr.h bzr_pack_frame)
    need = {"image": npad, "rays": 7 * npad, "compact": npad // 4 + 1 + 6 * (cap + 1)}[layout]
    if int(packed.numel()) < need:
        raise BzrError(f"pack_frame: {layout} layout needs {need} floats (npad {npad}, cap {cap}), packed has "
                       f"{int(packed.numel())}")
    bufs = [_Buf(status, np.uint32), _Buf(segments, np.uint32), _Buf(packed, np.float32, True)]
    r = _Buf(rays, np.float32) if rays is not None else _Buf(None, np.float32)
    if r.ptr is not None:
        bufs.append(r)
    if _residency(*bufs) != DEVICE_PTRS:
        raise BzrError("pack_frame takes device tensors")
    with _stream_for(ctx, DEVICE_PTRS):
        _check(lib().bzr_pack_frame(ctx.handle, PACK_LAYOUTS[layout], r.ptr, bufs[0].ptr, bufs[1].ptr, n, int(npad),
                                    int(cap), bufs[2].ptr))
    return packed


def trace_tiled(ctxs, lenses, ri, rays, tile_rays=4096, mode=MODE_PARITY, out=None):
    """bzr_trace_tiled: the chain over several contexts (one per device) from one process, gathered to
    ctxs[0]'s device on the device side.  `lenses[d]` is the list of DeviceMesh living on ctxs[d]; rays
    [6, n] ordered tile-major, a host array or a tensor on ctxs[0]'s device (then the outputs are tensors
    there).  -> (rays [6, n], status [n], segments [n]) in input order (RAYS_AOS in mode: rays [n, 6] both ways)."""
    nc, nl = len(ctxs), len(ri)
    if len(lenses) != nc or any(len(ls) != nl for ls in lenses):
        raise ValueError("lenses must hold one list of len(ri) meshes per context")
    r = _Buf(rays, np.float32)
    n = _n_of(rays, mode)
    if out is None:
        out = (_empty_like(rays, 6, np.float32, mode), _empty_like(rays, 0, np.uint32, mode),
               _empty_like(rays, 0, np.uint32, mode))
    o, s_, g = _Buf(out[0], np.float32, True), _Buf(out[1], np.uint32, True), _Buf(out[2], np.uint32, True)
    res = _residency(r, o, s_, g)
    cs = (_P * nc)(*[c.handle for c in ctxs])
    hs = (_P * (nc * nl))(*[m.handle for ls in lenses for m in ls])
    ris = (_F * nl)(*[float(x) for x in ri])
    if res == DEVICE_PTRS:
        import torch

        torch.cuda.current_stream(ctxs[0].device).synchronize()  # torch-made inputs are complete
    _check(lib().bzr_trace_tiled(ctypes.cast(cs, _P), nc, ctypes.cast(hs, _P), ctypes.cast(ris, _P), nl,
                                 r.ptr, n, tile_rays, o.ptr, s_.ptr, g.ptr, mode | res))
    return out


GATHER_AUTO, GATHER_RCCL, GATHER_PEER, GATHER_DIRECT = 0, 1, 2, 3  # BZR_GATHER_*


class TiledPlan:
    """bzr_tiled: multi-device frames from one process, gathered to device 0 on the device side (RCCL over
    xGMI between distinct devices, peer copies otherwise; one device: traced straight into the outputs).  ctxs: nslot lists of ndev contexts (slot s, device
    d); the frame is n tile-major rays."""

    def __init__(self, ctxs, n: int, tile_rays: int = 4096, transport: int = GATHER_AUTO):
        slots = [list(s) for s in ctxs]
        self.ndev, self.nslot = len(slots[0]), len(slots)
        if any(len(s) != self.ndev for s in slots):
            raise ValueError("every slot lists the same number of devices")
        self.ctxs = slots
        flat = (_P * (self.ndev * self.nslot))(*[c.handle for s in slots for c in s])
        h = _P()
        _check(lib().bzr_tiled_create(ctypes.cast(flat, _P), self.ndev, self.nslot, n, tile_rays, transport,
                                      ctypes.byref(h)))
        self.handle, self.n, self.tile_rays = h, n, tile_rays

    def info(self):
        """(transport, rays per device share, npad)"""
        t, npad = _I32(0), _U32(0)
        share = np.zeros(self.ndev, np.uint32)
        _check(lib().bzr_tiled_info(self.handle, ctypes.byref(t), share.ctypes.data, ctypes.byref(npad)))
        return int(t.value), share, int(npad.value)

    def set_rays(self, rays, mode=0):
        """The frame's rays [6, n] (or [n, 6] records with mode RAYS_AOS), host array or tensor on device 0."""
        if _n_of(rays, mode) != self.n:
            raise BzrError(f"set_rays: {_n_of(rays, mode)} rays for a plan of {self.n}")
        r = _Buf(rays, np.float32)
        if r.device:
            import torch

            torch.cuda.current_stream(self.ctxs[0][0].device).synchronize()
        _check(lib().bzr_tiled_set_rays(self.handle, r.ptr, (DEVICE_PTRS if r.device else HOST_PTRS) | (mode & RAYS_AOS)))
        # a device source is only queued for copying (bzr_tiled_set_rays): keep it -- and any contiguous / float32
        # copy _Buf made of it -- alive until the copy has run, i.e. until the next sync() or set_rays(), so torch's
        # caching allocator cannot hand its memory to a kernel that overwrites it first
        self._pending_src = (rays, r) if r.device else None

    def trace(self, lenses, ri, out_rays, out_status, out_segments=None, mode=MODE_PARITY):
        """One frame; lenses[d] = device d's DeviceMesh list.  Device tensors (on device 0): queued, ready on
        stream() / after sync(); host arrays: synchronous."""
        nl = len(ri)
        hs = (_P * (self.ndev * nl))(*[m.handle for ls in lenses for m in ls])
        ris = (_F * nl)(*[float(x) for x in ri])
        o, s_ = _Buf(out_rays, np.float32, True), _Buf(out_status, np.uint32, True)
        g = _Buf(out_segments, np.uint32, True)
        res = _residency(o, s_, *([g] if out_segments is not None else []))
        _check(lib().bzr_tiled_trace(self.handle, ctypes.cast(hs, _P), ctypes.cast(ris, _P), nl, o.ptr, s_.ptr, g.ptr,
                                     res | mode))

    def stream(self) -> int:
        p = _P()
        _check(lib().bzr_tiled_stream(self.handle, ctypes.byref(p)))
        return int(p.value or 0)

    def sync(self):
        _check(lib().bzr_tiled_sync(self.handle))
        self._pending_src = None  # the queued ray copy has run

    def set_layout(self, layout: str, cap: int = 0):
        """"rays" (28 B per ray) or "compact" (survivors only, up to `cap` per device share)."""
        _check(lib().bzr_tiled_set_layout(self.handle, PACK_LAYOUTS[layout], cap))

    def calibrate(self, lenses, ri, mode=MODE_PARITY) -> int:
        """One synchronous frame, then the compact layout sized from its survivors; returns the capacity."""
        nl = len(ri)
        hs = (_P * (self.ndev * nl))(*[m.handle for ls in lenses for m in ls])
        ris = (_F * nl)(*[float(x) for x in ri])
        cap = _U32(0)
        _check(lib().bzr_tiled_calibrate(self.handle, ctypes.cast(hs, _P), ctypes.cast(ris, _P), nl, mode,
                                          ctypes.byref(cap)))
        return int(cap.value)

    def close(self):
        if getattr(self, "handle", None):
            lib().bzr_tiled_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def interpolate(ctx: Context, mesh: DeviceMesh, divisor: int, out=None):
    """BezierMesh::interpolate(divisor) on the device -> triangles [divisor^2 * n_patches, 3, 3] float32
    (reference order: sub-triangle outer, patch inner).  `out` may be a CUDA tensor (stays on the device)."""
    count = int(divisor) * int(divisor) * mesh.n
    if out is None:
        out = np.empty((count, 3, 3), np.float32)
    o = _Buf(out, np.float32, True)
    res = _residency(o)
    with _stream_for(ctx, res):
        _check(lib().bzr_mesh_interpolate(ctx.handle, mesh.handle, int(divisor), o.ptr, res))
    return out


# ------------------------------------------------------------ illumination
class Emitter(ctypes.Structure):
    """bzr_emitter: rectangle origin + a*edge_u + b*edge_v, parts_u x parts_v parts, points_per_part
    points per part, rays_per_point rays per point, hemisphere around +x numbered by `belts`."""
    _fields_ = [("origin", _F * 3), ("edge_u", _F * 3), ("edge_v", _F * 3), ("parts_u", _U32), ("parts_v", _U32),
                ("points_per_part", _U32), ("rays_per_point", _U32), ("belts", _U32), ("seed", ctypes.c_uint64)]


class Target(ctypes.Structure):
    """bzr_target: origin + a*axis_u + b*axis_v, a < size_u, b < size_v, bins_u x bins_v cells."""
    _fields_ = [("origin", _F * 3), ("axis_u", _F * 3), ("axis_v", _F * 3), ("size_u", _F), ("size_v", _F),
                ("bins_u", _U32), ("bins_v", _U32)]


ILLUM_STATS = ("emitted", "culled", "exited", "landed")  # BZR_ILLUM_* ids


def emit(ctx: Context, em: Emitter, first: int, n: int, rays=None, patch=None):
    """Rays first .. first+n-1 of the emitter -> (rays [6, n], hemisphere patch index [n])."""
    rays = np.empty((6, n), np.float32) if rays is None else rays
    patch = np.empty(n, np.uint32) if patch is None else patch
    r, p = _Buf(rays, np.float32, True), _Buf(patch, np.uint32, True)
    res = _residency(r, p)
    with _stream_for(ctx, res):
        _check(lib().bzr_emit(ctx.handle, ctypes.byref(em), int(first), int(n), r.ptr, p.ptr, res))
    return rays, patch


def illuminate(ctx: Context, lenses, ri, em: Emitter, total_rays: int, target: Target, hist=None, mode=MODE_PARITY):
    """Emitter -> bounding-sphere cull -> refraction chain -> target counts.  Returns (hist [bins_v, bins_u]
    uint32, accumulated into `hist` if given, stats dict).  mode: PIPELINE_STAGED / PIPELINE_FUSED, MODE_FAST."""
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    ris = (_F * nl)(*[float(x) for x in ri])
    hist = np.zeros((target.bins_v, target.bins_u), np.uint32) if hist is None else hist
    h = _Buf(hist, np.uint32, True)
    stats = (ctypes.c_uint64 * 4)()
    res = _residency(h)
    with _stream_for(ctx, res):
        _check(lib().bzr_illuminate(ctx.handle, handles, ris, nl, ctypes.byref(em), int(total_rays),
                                    ctypes.byref(target), h.ptr, stats, res | mode))
    return hist, dict(zip(ILLUM_STATS, [int(x) for x in stats]))


EMISSION_UNIFORM, EMISSION_LAMBERT = 0, 1  # BZR_EMISSION_*: w0 = 1 | w0 = the direction's x component
SURFACE_LOSSLESS, SURFACE_FRESNEL = 0, 1  # BZR_SURFACE_*: T = 1 | the unpolarised Fresnel transmittance


class Radiometry(ctypes.Structure):
    """bzr_radiometry"""
    _fields_ = [("emission", _U32), ("surface", _U32)]


def illuminate_power(ctx: Context, lenses, ri, em: Emitter, total_rays: int, target: Target,
                     emission=EMISSION_LAMBERT, surface=SURFACE_FRESNEL, flux=None, hist=None, mode=MODE_PARITY):
    """illuminate with ray power.  Returns (flux uint64 [bins_v, bins_u] in 32.32 fixed point (flux_to_float),
    accumulated into `flux` if given; hist uint32 [bins_v, bins_u] as illuminate's, accumulated into `hist` if given;
    stats dict; power dict: the emitted / culled / exited / landed power in the same fixed point)."""
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    ris = (_F * nl)(*[float(x) for x in ri])
    if flux is None:
        flux = np.zeros((target.bins_v, target.bins_u), np.uint64)
    if hist is None:
        if _is_tensor(flux):
            import torch

            hist = torch.zeros((target.bins_v, target.bins_u), dtype=torch.int32, device=flux.device)
        else:
            hist = np.zeros((target.bins_v, target.bins_u), np.uint32)
    f, h = _Buf(flux, np.uint64, True), _Buf(hist, np.uint32, True)
    rad = Radiometry(int(emission), int(surface))
    stats, power = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)()
    res = _residency(f, h)
    with _stream_for(ctx, res):
        _check(lib().bzr_illuminate_power(ctx.handle, handles, ris, nl, ctypes.byref(em), int(total_rays),
                                          ctypes.byref(target), ctypes.byref(rad), f.ptr, h.ptr, stats, power, res | mode))
    return (flux, hist, dict(zip(ILLUM_STATS, [int(x) for x in stats])),
            dict(zip(ILLUM_STATS, [int(x) for x in power])))


def illuminate_spectral(ctx: Context, lenses, ri_table, em: Emitter, total_rays: int, target: Target,
                        emission=EMISSION_LAMBERT, surface=SURFACE_FRESNEL, flux=None, hist=None, mode=MODE_PARITY):
    """illuminate_power per spectral channel: emitter ray i is in channel i mod nchan and refracts at lens l with
    ri_table[l, i mod nchan] (ri_table [nlens, nchan] float32, host).  Returns (flux uint64 [nchan, bins_v, bins_u] in
    32.32 fixed point, accumulated into `flux` if given; hist uint32 of the same shape, accumulated into `hist` if given;
    stats: a list of nchan dicts; power: a list of nchan dicts, in the same fixed point).  No source spectrum is
    taken: scale channel c's map by the source's power in that channel."""
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    table, nchan = _ri_table(ri_table, nl)
    shape = (nchan, target.bins_v, target.bins_u)
    if flux is None:
        flux = np.zeros(shape, np.uint64)
    if hist is None:
        if _is_tensor(flux):
            import torch

            hist = torch.zeros(shape, dtype=torch.int32, device=flux.device)
        else:
            hist = np.zeros(shape, np.uint32)
    f, h = _Buf(flux, np.uint64, True), _Buf(hist, np.uint32, True)
    rad = Radiometry(int(emission), int(surface))
    rows = max(nchan, 1)
    stats, power = (ctypes.c_uint64 * (4 * rows))(), (ctypes.c_uint64 * (4 * rows))()
    res = _residency(f, h)
    with _stream_for(ctx, res):
        _check(lib().bzr_illuminate_spectral(ctx.handle, handles, table.ctypes.data if table.size else None, nl, nchan,
                                             ctypes.byref(em), int(total_rays), ctypes.byref(target), ctypes.byref(rad),
                                             f.ptr, h.ptr, stats, power, res | mode))
    return (flux, hist, [dict(zip(ILLUM_STATS, [int(x) for x in stats[4 * c:4 * c + 4]])) for c in range(nchan)],
            [dict(zip(ILLUM_STATS, [int(x) for x in power[4 * c:4 * c + 4]])) for c in range(nchan)])


LEDGER_LOST, LEDGER_EXITED, LEDGER_LANDED, LEDGER_FIELDS = 0, 1, 2, 3  # BZR_LEDGER_*
LEDGER_ROWS = MAX_BOUNCES + 1  # BZR_LEDGER_ROWS: row min(bounces, MAX_BOUNCES)


def illuminate_tir(ctx: Context, lenses, ri_table, em: Emitter, total_rays: int, target: Target, max_bounces=4,
                   emission=EMISSION_LAMBERT, surface=SURFACE_FRESNEL, flux=None, hist=None, reflected_flux=None,
                   reflected_hist=None, mode=MODE_PARITY):
    """illuminate_spectral with total internal reflection: every traced ray goes through trace_chain_tir's chain with up
    to max_bounces (<= MAX_BOUNCES) reflections per lens.  Returns (flux, hist, reflected_flux, reflected_hist, stats,
    power, ledger): the first two and stats / power as illuminate_spectral returns them, now including the rays that
    reflected; reflected_flux / reflected_hist [nchan, bins_v, bins_u] hold the landed rays with at least one reflection
    (the stray-light map), accumulated into the arrays given; ledger = {"count", "power"}: uint64
    [nchan, LEDGER_ROWS, LEDGER_FIELDS], every traced ray of channel c in row min(bounces, MAX_BOUNCES) under
    LEDGER_LOST (ended NONE) or LEDGER_EXITED (left the last lens), and under LEDGER_LANDED too if it met the target;
    "power" sums the rays' final weights in the maps' 32.32 fixed point (bzr.h bzr_illuminate_tir)."""
    return _illuminate_reflecting(ctx, lenses, ri_table, None, em, total_rays, target, max_bounces, emission, surface,
                                  flux, hist, reflected_flux, reflected_hist, mode)


def illuminate_media(ctx: Context, lenses, ri_table, gap_table, glass_absorb, gap_absorb, em: Emitter, total_rays: int,
                     target: Target, max_bounces=4, emission=EMISSION_LAMBERT, surface=SURFACE_FRESNEL, flux=None,
                     hist=None, reflected_flux=None, reflected_hist=None, mode=MODE_PARITY):
    """illuminate_tir over trace_chain_absorb's chain -> the same seven-tuple.  gap_table [nlens + 1, nchan] and
    glass_absorb / gap_absorb [nlens, nchan] are trace_chain_absorb's (None: vacuum, all zero).  The emitter sits in the
    medium gap_table[0]; the leg from the last lens to the target is neither refracted again nor attenuated.  With
    absorption the ledger's LOST + EXITED power falls short of EMITTED - CULLED under SURFACE_LOSSLESS by what the media
    absorbed; with vacuum and zero tables every output is illuminate_tir's bit for bit (bzr.h bzr_illuminate_media)."""
    nl = len(lenses)
    _, nchan = _ri_table(ri_table, nl)
    media = (_gap_table(gap_table, nl, nchan), _absorb_table(glass_absorb, "glass_absorb", nl, nchan),
             _absorb_table(gap_absorb, "gap_absorb", nl, nchan))
    return _illuminate_reflecting(ctx, lenses, ri_table, media, em, total_rays, target, max_bounces, emission, surface,
                                  flux, hist, reflected_flux, reflected_hist, mode)


def _illuminate_reflecting(ctx, lenses, ri_table, media, em, total_rays, target, max_bounces, emission, surface, flux, hist,
                           reflected_flux, reflected_hist, mode, far=None, ghost_seed=None, axis=None, coat=None):
    """illuminate_tir (media None), illuminate_media (media = the gap table and the two absorption tables) or
    illuminate_farfield (far = the frame and its three maps, each map or None; target may then be None);
    illuminate_ghost: ghost_seed given, media given, far or None; illuminate_bidir: and axis given -- the ledger dict
    then holds the BACK rays' rows too, "back_count" and "back_power" [nchan][LEDGER_ROWS]; illuminate_coated: and coat
    given (a Coating)."""
    nl = len(lenses)
    handles = (_P * nl)(*[m.handle for m in lenses])
    table, nchan = _ri_table(ri_table, nl)
    rows = max(nchan, 1)
    first = flux  # the buffer whose residency the maps made here follow
    if far is not None:
        first = next((a for a in (flux, hist, reflected_flux, reflected_hist) + tuple(far[1:]) if a is not None), None)

    def like(a, shape, np_dtype, torch_dtype):
        if a is not None:
            return a
        if _is_tensor(first):
            import torch

            return torch.zeros(shape, dtype=getattr(torch, torch_dtype), device=first.device)
        return np.zeros(shape, np_dtype)

    if target is not None:
        shape = (nchan, target.bins_v, target.bins_u)
        flux = like(flux, shape, np.uint64, "int64")
        first = flux if first is None else first
        hist = like(hist, shape, np.uint32, "int32")
        reflected_flux = like(reflected_flux, shape, np.uint64, "int64")
        reflected_hist = like(reflected_hist, shape, np.uint32, "int32")
    f, h = _Buf(flux, np.uint64, True), _Buf(hist, np.uint32, True)
    rf, rh = _Buf(reflected_flux, np.uint64, True), _Buf(reflected_hist, np.uint32, True)
    bufs = [f, h, rf, rh]
    far_out = None
    if far is not None:
        frame = far[0]
        fshape = (nchan, frame.bins_v, frame.bins_u)
        far_out = {"flux": like(far[1], fshape, np.uint64, "int64"), "hist": like(far[2], fshape, np.uint32, "int32"),
                   "reflected_flux": like(far[3], fshape, np.uint64, "int64")}
        ff, fh = _Buf(far_out["flux"], np.uint64, True), _Buf(far_out["hist"], np.uint32, True)
        frf = _Buf(far_out["reflected_flux"], np.uint64, True)
        bufs += [ff, fh, frf]
        fstats, fpower = (ctypes.c_uint64 * (2 * rows))(), (ctypes.c_uint64 * (2 * rows))()
    rad = Radiometry(int(emission), int(surface))
    stats, power = (ctypes.c_uint64 * (4 * rows))(), (ctypes.c_uint64 * (4 * rows))()
    ledger = {k: np.zeros((rows, LEDGER_ROWS, LEDGER_FIELDS), np.uint64) for k in ("count", "power")}
    res = _residency(*bufs)
    tail = (nl, nchan, ctypes.byref(em), int(total_rays), ctypes.byref(target) if target is not None else None,
            ctypes.byref(rad), int(max_bounces), f.ptr,
            h.ptr, rf.ptr, rh.ptr, stats, power, ledger["count"].ctypes.data, ledger["power"].ctypes.data, res | mode)
    back = {k: np.zeros((rows, LEDGER_ROWS), np.uint64) for k in ("back_count", "back_power")}
    with _stream_for(ctx, res):
        if axis is not None:
            ax = np.ascontiguousarray(axis, np.float32)
            if ax.shape != (3,):
                raise BzrError("axis must have three components")
            far_args = (ctypes.byref(frame), ff.ptr, fh.ptr, frf.ptr, fstats, fpower) if far is not None else (None,) * 6
            if coat is not None:
                cref, ckeep = _coating(coat, nl, nchan)
                _check(lib().bzr_illuminate_coated(ctx.handle, handles, table.ctypes.data if table.size else None,
                                                   *[_table_ptr(a) for a in media], *tail[:7],
                                                   int(ghost_seed) & ((1 << 64) - 1), ax.ctypes.data, cref, *tail[7:-1],
                                                   back["back_count"].ctypes.data, back["back_power"].ctypes.data,
                                                   tail[-1], *far_args))
                del ckeep
            else:
                _check(lib().bzr_illuminate_bidir(ctx.handle, handles, table.ctypes.data if table.size else None,
                                                  *[_table_ptr(a) for a in media], *tail[:7],
                                                  int(ghost_seed) & ((1 << 64) - 1), ax.ctypes.data, *tail[7:-1],
                                                  back["back_count"].ctypes.data, back["back_power"].ctypes.data,
                                                  tail[-1], *far_args))
            ledger.update(back)
        elif ghost_seed is not None:
            far_args = (ctypes.byref(frame), ff.ptr, fh.ptr, frf.ptr, fstats, fpower) if far is not None else (None,) * 6
            _check(lib().bzr_illuminate_ghost(ctx.handle, handles, table.ctypes.data if table.size else None,
                                              *[_table_ptr(a) for a in media], *tail[:7],
                                              int(ghost_seed) & ((1 << 64) - 1), *tail[7:], *far_args))
        elif far is not None:
            _check(lib().bzr_illuminate_farfield(ctx.handle, handles, table.ctypes.data if table.size else None,
                                                 *[_table_ptr(a) for a in media], *tail, ctypes.byref(frame), ff.ptr,
                                                 fh.ptr, frf.ptr, fstats, fpower))
        elif media is None:
            _check(lib().bzr_illuminate_tir(ctx.handle, handles, table.ctypes.data if table.size else None, *tail))
        else:
            _check(lib().bzr_illuminate_media(ctx.handle, handles, table.ctypes.data if table.size else None,
                                              *[_table_ptr(a) for a in media], *tail))
    seven = (flux, hist, reflected_flux, reflected_hist,
             [dict(zip(ILLUM_STATS, [int(x) for x in stats[4 * c:4 * c + 4]])) for c in range(nchan)],
             [dict(zip(ILLUM_STATS, [int(x) for x in power[4 * c:4 * c + 4]])) for c in range(nchan)],
             {k: v[:nchan] for k, v in ledger.items()})
    if far is None:
        return seven
    far_out["stats"] = [dict(zip(FAR_STATS, [int(x) for x in fstats[2 * c:2 * c + 2]])) for c in range(nchan)]
    far_out["power"] = [dict(zip(FAR_STATS, [int(x) for x in fpower[2 * c:2 * c + 2]])) for c in range(nchan)]
    return seven + (far_out,)


# ------------------------------------------------------------ far field
class FarField(ctypes.Structure):
    """bzr_farfield: unit, orthogonal axis_u / axis_v (the pole is axis_u x axis_v), the map [-extent, extent)^2 of the
    Lambert azimuthal equal-area projection about the pole (0 < extent <= sqrt(2)), bins_u x bins_v cells of equal
    solid angle."""
    _fields_ = [("axis_u", _F * 3), ("axis_v", _F * 3), ("extent", _F), ("bins_u", _U32), ("bins_v", _U32)]


FAR_STATS = ("seen", "binned")  # BZR_FAR_* ids
SQRT2 = float(np.float32(np.sqrt(2.0)))  # the largest extent: the float at or below sqrt(2), 0x3FB504F3


def farfield_bin(ctx: Context, far: FarField, rays, weight=None, status=None, channel=None, nchan=1, flux=None,
                 hist=None, mode=MODE_PARITY):
    """bzr_farfield_bin: bins a traced batch (rays [6, n] as trace_chain_* returns them; weight, status, channel [n] or
    None) by direction.  Returns (flux uint64 [nchan, bins_v, bins_u] in 32.32 fixed point, hist uint32 of the same
    shape -- accumulated into the arrays given --, stats: a list of nchan dicts {"seen", "binned"}, power: the same
    with the sums of q(w)).  numpy arrays or device tensors, all on one side."""
    n = _n_of(rays)
    shape = (int(nchan), far.bins_v, far.bins_u)
    if flux is None:
        if _is_tensor(rays):
            import torch

            flux = torch.zeros(shape, dtype=torch.int64, device=rays.device)
        else:
            flux = np.zeros(shape, np.uint64)
    if hist is None:
        if _is_tensor(flux):
            import torch

            hist = torch.zeros(shape, dtype=torch.int32, device=flux.device)
        else:
            hist = np.zeros(shape, np.uint32)
    r, w, s = _Buf(rays, np.float32), _Buf(weight, np.float32), _Buf(status, np.uint32)
    c, f, h = _Buf(channel, np.uint8), _Buf(flux, np.uint64, True), _Buf(hist, np.uint32, True)
    for name, a in (("weight", weight), ("status", status), ("channel", channel)):
        if a is not None and tuple(a.shape if _is_tensor(a) else np.shape(a)) != (n,):
            raise BzrError(f"{name} must be [{n}]")
    rows = max(int(nchan), 1)
    stats, power = (ctypes.c_uint64 * (2 * rows))(), (ctypes.c_uint64 * (2 * rows))()
    res = _residency(r, w, s, c, f, h)
    with _stream_for(ctx, res):
        _check(lib().bzr_farfield_bin(ctx.handle, ctypes.byref(far), r.ptr, w.ptr, s.ptr, c.ptr, n, int(nchan), f.ptr,
                                      h.ptr, stats, power, res | mode))
    return (flux, hist, [dict(zip(FAR_STATS, [int(x) for x in stats[2 * k:2 * k + 2]])) for k in range(int(nchan))],
            [dict(zip(FAR_STATS, [int(x) for x in power[2 * k:2 * k + 2]])) for k in range(int(nchan))])


def illuminate_farfield(ctx: Context, lenses, ri_table, gap_table, glass_absorb, gap_absorb, em: Emitter, total_rays: int,
                        target, far: FarField, max_bounces=4, emission=EMISSION_LAMBERT, surface=SURFACE_FRESNEL,
                        flux=None, hist=None, reflected_flux=None, reflected_hist=None, far_flux=None, far_hist=None,
                        far_reflected_flux=None, mode=MODE_PARITY):
    """illuminate_media with a far-field frame -> illuminate_media's seven-tuple plus a dict of the far outputs: "flux",
    "hist" and "reflected_flux" [nchan, far.bins_v, far.bins_u] (every traced ray that left the last lens, binned by
    direction with its final weight; the reflected map holds those with at least one reflection), "stats" and "power":
    lists of nchan dicts {"seen", "binned"}, "seen" being the channel's exited count / power.  target None: no near
    maps (the first four entries are None, the near maps must not be given) and the landed entries are 0."""
    nl = len(lenses)
    _, nchan = _ri_table(ri_table, nl)
    media = (_gap_table(gap_table, nl, nchan), _absorb_table(glass_absorb, "glass_absorb", nl, nchan),
             _absorb_table(gap_absorb, "gap_absorb", nl, nchan))
    if target is None and any(a is not None for a in (flux, hist, reflected_flux, reflected_hist)):
        raise BzrError("target maps given without a target")
    return _illuminate_reflecting(ctx, lenses, ri_table, media, em, total_rays, target, max_bounces, emission, surface,
                                  flux, hist, reflected_flux, reflected_hist, mode,
                                  far=(far, far_flux, far_hist, far_reflected_flux))


def illuminate_ghost(ctx: Context, lenses, ri_table, gap_table, glass_absorb, gap_absorb, em: Emitter, total_rays: int,
                     target, far=None, max_bounces=4, ghost_seed=0, emission=EMISSION_LAMBERT, surface=SURFACE_FRESNEL,
                     flux=None, hist=None, reflected_flux=None, reflected_hist=None, far_flux=None, far_hist=None,
                     far_reflected_flux=None, mode=MODE_PARITY):
    """illuminate_farfield over trace_chain_ghost's chain: emitter ray j draws with ray number j, whatever the batching.
    Returns illuminate_farfield's eight-tuple, or with far None illuminate_media's seven-tuple; one of target and far is
    given.  Ghost rays arrive in the reflected maps and in ledger rows >= 1.  With SURFACE_LOSSLESS or max_bounces 0
    every output is illuminate_farfield's bit for bit (bzr.h bzr_illuminate_ghost)."""
    nl = len(lenses)
    _, nchan = _ri_table(ri_table, nl)
    media = (_gap_table(gap_table, nl, nchan), _absorb_table(glass_absorb, "glass_absorb", nl, nchan),
             _absorb_table(gap_absorb, "gap_absorb", nl, nchan))
    if target is None and far is None:
        raise BzrError("neither a target nor a far-field frame")
    if target is None and any(a is not None for a in (flux, hist, reflected_flux, reflected_hist)):
        raise BzrError("target maps given without a target")
    if far is None and any(a is not None for a in (far_flux, far_hist, far_reflected_flux)):
        raise BzrError("far maps given without a far-field frame")
    return _illuminate_reflecting(ctx, lenses, ri_table, media, em, total_rays, target, max_bounces, emission, surface,
                                  flux, hist, reflected_flux, reflected_hist, mode,
                                  far=None if far is None else (far, far_flux, far_hist, far_reflected_flux),
                                  ghost_seed=ghost_seed)


def illuminate_bidir(ctx: Context, lenses, ri_table, gap_table, glass_absorb, gap_absorb, em: Emitter, total_rays: int,
                     target, far=None, max_bounces=4, ghost_seed=0, axis=(1.0, 0.0, 0.0), emission=EMISSION_LAMBERT,
                     surface=SURFACE_FRESNEL, flux=None, hist=None, reflected_flux=None, reflected_hist=None,
                     far_flux=None, far_hist=None, far_reflected_flux=None, mode=MODE_PARITY):
    """illuminate_ghost over trace_chain_bidir's chain, `axis` its forward direction.  Returns illuminate_ghost's tuple;
    its ledger dict also holds "back_count" and "back_power" [nchan][LEDGER_ROWS]: the rays that left in front of the
    first lens (RR_BACK), by min(bounces, MAX_BOUNCES), and their summed q(w).  Those rays are in no ledger field and
    in no map; per channel LOST + EXITED + BACK over the rows is EMITTED - CULLED (bzr.h bzr_illuminate_bidir)."""
    nl = len(lenses)
    _, nchan = _ri_table(ri_table, nl)
    media = (_gap_table(gap_table, nl, nchan), _absorb_table(glass_absorb, "glass_absorb", nl, nchan),
             _absorb_table(gap_absorb, "gap_absorb", nl, nchan))
    if target is None and far is None:
        raise BzrError("neither a target nor a far-field frame")
    if target is None and any(a is not None for a in (flux, hist, reflected_flux, reflected_hist)):
        raise BzrError("target maps given without a target")
    if far is None and any(a is not None for a in (far_flux, far_hist, far_reflected_flux)):
        raise BzrError("far maps given without a far-field frame")
    return _illuminate_reflecting(ctx, lenses, ri_table, media, em, total_rays, target, max_bounces, emission, surface,
                                  flux, hist, reflected_flux, reflected_hist, mode,
                                  far=None if far is None else (far, far_flux, far_hist, far_reflected_flux),
                                  ghost_seed=ghost_seed, axis=axis)


def illuminate_coated(ctx: Context, lenses, ri_table, gap_table, glass_absorb, gap_absorb, em: Emitter, total_rays: int,
                      target, far=None, max_bounces=4, ghost_seed=0, axis=(1.0, 0.0, 0.0), coat=None,
                      emission=EMISSION_LAMBERT, surface=SURFACE_FRESNEL, flux=None, hist=None, reflected_flux=None,
                      reflected_hist=None, far_flux=None, far_hist=None, far_reflected_flux=None, mode=MODE_PARITY):
    """illuminate_bidir over trace_chain_coated's chain, `coat` a Coating (None: no surface coated) -> illuminate_bidir's
    tuple.  With surface=SURFACE_LOSSLESS the coating is ignored; with no surface coated the call is illuminate_bidir
    bit for bit (bzr.h bzr_illuminate_coated)."""
    nl = len(lenses)
    _, nchan = _ri_table(ri_table, nl)
    media = (_gap_table(gap_table, nl, nchan), _absorb_table(glass_absorb, "glass_absorb", nl, nchan),
             _absorb_table(gap_absorb, "gap_absorb", nl, nchan))
    if target is None and far is None:
        raise BzrError("neither a target nor a far-field frame")
    if target is None and any(a is not None for a in (flux, hist, reflected_flux, reflected_hist)):
        raise BzrError("target maps given without a target")
    if far is None and any(a is not None for a in (far_flux, far_hist, far_reflected_flux)):
        raise BzrError("far maps given without a far-field frame")
    return _illuminate_reflecting(ctx, lenses, ri_table, media, em, total_rays, target, max_bounces, emission, surface,
                                  flux, hist, reflected_flux, reflected_hist, mode,
                                  far=None if far is None else (far, far_flux, far_hist, far_reflected_flux),
                                  ghost_seed=ghost_seed, axis=axis, coat=coat if coat is not None else Coating(None, 0))


def farfield_cell(far: FarField, directions) -> np.ndarray:
    """bzr_farfield_cell on the host (the device's twin, bit for bit): directions [n, 3] (or [3]) float32 -> int32 cell
    indices iv * bins_u + iu, -1 where a direction is not binned."""
    d = np.ascontiguousarray(directions, np.float32)
    one = d.ndim == 1
    d = d.reshape(-1, 3)
    out = np.empty(len(d), np.int32)
    _check(lib().bzr_debug_farfield_cells(ctypes.byref(far), d.ctypes.data, len(d), out.ctypes.data))
    return out[0] if one else out


def farfield_directions(far: FarField):
    """Each cell centre in float64: (unit directions [bins_v, bins_u, 3], polar angle from the pole [bins_v, bins_u],
    azimuth atan2(Y, X) [bins_v, bins_u]), radians."""
    d = np.empty((far.bins_v, far.bins_u, 3), np.float64)
    polar, azimuth = np.empty((far.bins_v, far.bins_u), np.float64), np.empty((far.bins_v, far.bins_u), np.float64)
    _check(lib().bzr_farfield_directions(ctypes.byref(far), d.ctypes.data, polar.ctypes.data, azimuth.ctypes.data))
    return d, polar, azimuth


def farfield_intensity(far: FarField, flux, scale: float = 1.0) -> np.ndarray:
    """Power per steradian: scale x flux / 2^32 / cell solid angle, float64 of flux's shape ([..., bins_v, bins_u]);
    scale = 1 / emitted power gives a normalised pattern."""
    a = np.ascontiguousarray(flux.cpu().numpy() if _is_tensor(flux) else flux).view(np.uint64)
    if a.shape[-2:] != (far.bins_v, far.bins_u):
        raise BzrError(f"flux must be [..., {far.bins_v}, {far.bins_u}], got {a.shape}")
    out = np.empty(a.shape, np.float64)
    nmaps = a.size // (far.bins_v * far.bins_u)
    _check(lib().bzr_farfield_intensity(ctypes.byref(far), a.ctypes.data, nmaps, float(scale), out.ctypes.data))
    return out


def debug_farfield_rounds(ctx: Context, rounds: int):
    """bzr_debug_farfield_rounds: k_land_far's combine rounds for the following calls (0: per-lane atomics, 64:
    unbounded, negative: the default)."""
    _check(lib().bzr_debug_farfield_rounds(ctx.handle, int(rounds)))


def flux_to_float(flux) -> np.ndarray:
    """32.32 fixed-point power (illuminate_power's flux and power sums) as float64."""
    a = flux.cpu().numpy() if _is_tensor(flux) else np.asarray(flux)
    return a.astype(np.uint64).astype(np.float64) / 2.0 ** 32


def debug_fresnel(eta, cs) -> np.ndarray:
    """bzr_debug_fresnel: the kernels' Fresnel transmittance evaluated on the host for (eta, cos) pairs; 0 where
    eta^2 (1 - cos^2) >= 0.99."""
    e, c = np.ascontiguousarray(eta, np.float32), np.ascontiguousarray(cs, np.float32)
    if e.shape != c.shape or e.ndim != 1:
        raise BzrError("eta and cs must be 1-D arrays of one length")
    out = np.empty(e.shape, np.float32)
    _check(lib().bzr_debug_fresnel(e.ctypes.data, c.ctypes.data, e.size, out.ctypes.data))
    return out


def debug_attenuation(x, ctx: Context = None) -> np.ndarray:
    """bzr_debug_attenuation: the chain's Beer-Lambert term att(x) for x >= 0 (or NaN), evaluated on the host (ctx None)
    or by one kernel on the context's device; the two agree bit for bit."""
    a = np.ascontiguousarray(x, np.float32)
    if a.ndim != 1:
        raise BzrError("x must be a 1-D array")
    out = np.empty(a.shape, np.float32)
    _check(lib().bzr_debug_attenuation(ctx.handle if ctx is not None else None, a.ctypes.data, a.size, out.ctypes.data))
    return out


def bounding_sphere(mesh: DeviceMesh) -> np.ndarray:
    """The lens's Ritter sphere over its gate-region boxes: [cx, cy, cz, r]."""
    out = (_F * 4)()
    _check(lib().bzr_mesh_bounding_sphere(mesh.handle, out))
    return np.array(list(out), np.float32)


# ------------------------------------------------------------ host preprocessing
class TriMesh:
    """The reference's Mesh (host C++ in libbzr): generators, welding, orientation, Bezier build."""

    def __init__(self, _handle=None):
        if _handle is None:
            h = _P()
            _check(lib().bzr_trimesh_create(ctypes.byref(h)))
            _handle = h
        self.handle = _handle

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                lib().bzr_trimesh_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def copy(self) -> "TriMesh":
        h = _P()
        _check(lib().bzr_trimesh_copy(self.handle, ctypes.byref(h)))
        return TriMesh(h)

    def __len__(self):
        n = _U32(0)
        _check(lib().bzr_trimesh_size(self.handle, ctypes.byref(n)))
        return n.value

    @property
    def triangles(self) -> np.ndarray:
        t = np.empty((len(self), 3, 3), dtype=np.float32)
        _check(lib().bzr_trimesh_get(self.handle, t.ctypes.data))
        return t

    @triangles.setter
    def triangles(self, tris):
        t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 3, 3)
        _check(lib().bzr_trimesh_set(self.handle, t.ctypes.data, len(t)))

    def make_ellipsoid(self, sectors, belts, size=(1.0, 1.0, 1.0)):
        _check(lib().bzr_trimesh_make_ellipsoid(self.handle, sectors, belts, *map(float, size)))
        return self

    def make_unit_sphere(self, sectors, belts):
        return self.make_ellipsoid(sectors, belts, (1.0, 1.0, 1.0))

    def make_solid_of_revolution(self, sectors, belts, envelope, size):
        _check(lib().bzr_trimesh_make_solid_of_revolution(self.handle, sectors, belts, envelope, *map(float, size)))
        return self

    def read_stl(self, path):
        _check(lib().bzr_trimesh_read_stl(self.handle, str(path).encode()))
        return self

    def write_stl(self, path):
        _check(lib().bzr_trimesh_write_stl(self.handle, str(path).encode()))
        return self

    def transform(self, matrix=None, displacement=(0.0, 0.0, 0.0)):
        m = np.eye(3, dtype=np.float32) if matrix is None else np.asarray(matrix, dtype=np.float32)
        colmajor = np.ascontiguousarray(m.T.reshape(-1))
        d = np.ascontiguousarray(displacement, dtype=np.float32)
        _check(lib().bzr_trimesh_transform(self.handle, colmajor.ctypes.data, d.ctypes.data))
        return self

    def translate(self, d):
        return self.transform(None, d)

    def split(self, divisor: int):
        _check(lib().bzr_trimesh_split(self.handle, divisor))
        return self

    def split_maxside(self, max_side: float):
        _check(lib().bzr_trimesh_split_maxside(self.handle, float(max_side)))
        return self

    def standardize_vertices(self):
        _check(lib().bzr_trimesh_standardize_vertices(self.handle))
        return self

    def standardize_normals(self):
        _check(lib().bzr_trimesh_standardize_normals(self.handle))
        return self

    def standardize(self):
        return self.standardize_vertices().standardize_normals()

    def neighbours(self):
        n = len(self)
        fellow = np.empty((n, 3), dtype=np.uint32)
        start = np.empty((n, 3), dtype=np.uint8)
        _check(lib().bzr_trimesh_neighbours(self.handle, fellow.ctypes.data, start.ctypes.data))
        return fellow, start

    def bezier_patches(self) -> np.ndarray:
        """BezierMesh(Mesh) -> float32 [3n, 66] patch records (bzr_patch layout)."""
        out = np.empty((3 * len(self), PATCH_WORDS), dtype=np.float32)
        _check(lib().bzr_bezier_build(self.handle, out.ctypes.data))
        return out

    def bezier_split_thick(self) -> "TriMesh":
        out = TriMesh()
        _check(lib().bzr_bezier_split_thick(self.handle, out.handle))
        return out

    def bezier_interpolate(self, divisor: int) -> "TriMesh":
        out = TriMesh()
        _check(lib().bzr_bezier_interpolate(self.handle, divisor, out.handle))
        return out


__all__ = [
    "BzrError", "Context", "DeviceMesh", "TriMesh", "intersect", "patch_intersect", "refract", "trace_chain", "interpolate",
    "Emitter", "Target", "emit", "illuminate", "bounding_sphere",
    "FarField", "farfield_bin", "illuminate_farfield", "trace_chain_ghost", "ghost_uniform", "illuminate_ghost",
    "trace_chain_bidir", "bidir_uniform", "illuminate_bidir", "RR_BACK",
    "Coating", "COAT_SAMPLES", "trace_chain_coated", "illuminate_coated", "coat_transmittance", "coating_reflectance", "farfield_cell", "farfield_directions", "farfield_intensity",
    "device_count", "lib", "exported_symbols", "LIB_PATH",
]
