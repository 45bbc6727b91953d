"""Tensor-level wrappers over the C ABI (include/fjagg.h).

Every function here takes device-resident ``torch`` tensors (only the weights of
:func:`weighted_sum_dense` may be host arrays), launches on torch's current HIP
stream and returns without synchronising (like a JAX dispatch). They are the only
route from Python to the kernels; there is no CPU or PyTorch fallback: host client
deltas, an unsupported dtype or a missing library raise.
"""

from __future__ import annotations

import ctypes
import math
import os
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from fedjax_amd import _lib

_EUNSUPPORTED = -3  # FJAGG_EUNSUPPORTED: the launch was refused, nothing was issued
# how host weights reached the dense folds: in the kernel arguments, or uploaded because
# the launch was not built that way (tests and bench.py read these)
HOST_WEIGHT_PATHS = {"kernel_args": 0, "uploaded": 0}
_CODES = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.int32: _lib.I32}


def dtype_code(dt: torch.dtype) -> int:
    try:
        return _CODES[dt]
    except KeyError:
        raise TypeError(f"fedjax_amd kernels support float32, bfloat16 and int32, not {dt}") from None


class Event:
    """HIP timing event created without the system-scope fence (``fjagg_event_create``,
    include/fjcomm.h): recording one does not write back or invalidate the caches, so
    bracketing every launch leaves the launches themselves unperturbed (a default
    ``torch.cuda.Event`` record costs ~30 us of cache write-back on MI355X)."""

    def __init__(self):
        import ctypes
        h = ctypes.c_void_p()
        _lib.call("fjagg_event_create", ctypes.byref(h))
        self.handle = h.value

    def record(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        s = stream if stream is not None else torch.cuda.current_stream()
        _lib.call("fjagg_event_record", self.handle, s.cuda_stream)

    def elapsed_time(self, end: "Event") -> float:
        """Milliseconds from this event to ``end`` (waits for ``end``)."""
        import ctypes
        ms = ctypes.c_float()
        _lib.call("fjagg_event_elapsed_ms", ctypes.byref(ms), self.handle, end.handle)
        return float(ms.value)

    def __del__(self):
        if getattr(self, "handle", None):
            _lib.load().fjagg_event_destroy(self.handle)
            self.handle = None


def _stream_handle(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _require_device(*ts: torch.Tensor) -> torch.device:
    dev = None
    for t in ts:
        if not t.is_cuda:
            raise ValueError("fedjax_amd kernels need device tensors (got a host tensor); "
                             "move client deltas to the GPU first")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"tensors on different devices: {dev} and {t.device}")
    return dev


def stripe_variant(total_cols: int, cus: int) -> int:
    """The stripe width k_dense_stripe / k_ptrs_stripe use for ``total_cols`` columns
    (fjstripe.hip stripe_cols): 64 while every CU still gets a stripe, then 32, else 16,
    as FJAGG_VARIANT 20 / 21 / 22."""
    if (total_cols + 63) // 64 >= cus:
        return 20
    if (total_cols + 31) // 32 >= cus:
        return 21
    return 22


def weighted_sum_dense(x: torch.Tensor, w: torch.Tensor, *, scale: Optional[float] = None,
                       out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None,
                       accumulate: bool = False, mode: str = "exact",
                       workspace: Optional[torch.Tensor] = None, nontemporal: bool = False,
                       variant: int = 0, balanced: bool = True, reference_bf16: bool = False) -> torch.Tensor:
    """Fold a client-major slab ``x[K, P]`` (row stride ``x.stride(0)``, unit column
    stride) with per-client weights ``w[K]`` into ``out[P]``.

    ``w`` is float32 (float fold) or int32 (integer fold; int32 ``x`` only): a device
    tensor, or host weights (a numpy array or CPU tensor), which then travel in the
    kernel arguments (``FJAGG_HOST_TABLES``: no upload in front of the fold on the
    stream) when the library builds that launch, and are uploaded otherwise.
    ``scale`` multiplies the fold at the end (tree_mean's f32(1/W)).
    ``accumulate`` starts the fold from ``out``'s current contents.
    ``reference_bf16`` (bfloat16 ``x`` and ``out``, float32 ``w``): the reference's
    bfloat16 arithmetic — weights and scale rounded to bf16, every product and sum
    rounded to bf16 (acc dtype FJAGG_BF16) — instead of a float32 fold.
    """
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    K, P = x.shape
    if isinstance(w, np.ndarray):
        w = torch.from_numpy(w)
    if tuple(w.shape) != (K,):
        raise ValueError(f"w must have shape ({K},), got {tuple(w.shape)}")
    acc = _lib.I32 if w.dtype == torch.int32 else _lib.F32
    if w.dtype not in (torch.float32, torch.int32) or not w.is_contiguous():
        raise TypeError("w must be a contiguous float32 or int32 tensor")
    if reference_bf16:
        if x.dtype != torch.bfloat16 or w.dtype != torch.float32:
            raise TypeError("reference_bf16 folds bfloat16 deltas with float32 weights")
        acc = _lib.BF16
    if out is None:
        if out_dtype is None:
            if acc == _lib.BF16:
                out_dtype = torch.bfloat16
            elif acc == _lib.F32:  # int32 leaves * float weights promote to float32
                out_dtype = torch.float32 if x.dtype == torch.int32 else x.dtype
            else:
                out_dtype = torch.float32 if scale is not None else torch.int32
        out = torch.empty(P, dtype=out_dtype, device=x.device)
    if out.numel() != P or not out.is_contiguous():
        raise ValueError("out must be a contiguous tensor of P elements")
    dev = _require_device(x, out) if not w.is_cuda else _require_device(x, w, out)
    flags = (_lib.SCALE if scale is not None else 0) | (_lib.ACCUMULATE if accumulate else 0)
    flags |= (_lib.NONTEMPORAL if nontemporal else 0) | ((variant & 0xFF) << 8)
    flags |= 0 if balanced else _lib.UNBALANCED
    m = {"exact": _lib.MODE_EXACT, "split": _lib.MODE_SPLIT}[mode]
    ld = x.stride(0) if K > 1 else P
    sc = float(scale if scale is not None else 1.0)
    if not w.is_cuda:
        w = w.contiguous()
        if m == _lib.MODE_EXACT:
            rc = _lib.load().fjagg_wsum_dense(dtype_code(x.dtype), acc, dtype_code(out.dtype), x.data_ptr(), ld, K, P,
                                              w.data_ptr(), sc, out.data_ptr(), flags | _lib.HOST_TABLES, m, None, 0,
                                              _stream_handle(dev))
            if rc != _EUNSUPPORTED:
                _lib.check(rc, "fjagg_wsum_dense")
                HOST_WEIGHT_PATHS["kernel_args"] += 1
                return out
        w = _lib.upload(w, dev)  # not built with kernel-argument weights
        HOST_WEIGHT_PATHS["uploaded"] += 1
    ws_ptr, ws_bytes = None, 0
    if m == _lib.MODE_SPLIT:
        need = split_workspace_bytes(K, P)
        if need:
            if workspace is None:
                workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            ws_ptr, ws_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    _lib.call("fjagg_wsum_dense", dtype_code(x.dtype), acc, dtype_code(out.dtype), x.data_ptr(), ld,
              K, P, w.data_ptr(), sc, out.data_ptr(), flags, m, ws_ptr, ws_bytes, _stream_handle(dev))
    return out


def weighted_sum_l2_dense(x: torch.Tensor, w: torch.Tensor, *, scale: Optional[float] = None,
                          out: Optional[torch.Tensor] = None, l2sq: Optional[torch.Tensor] = None,
                          accumulate: bool = False, nontemporal: bool = False,
                          workspace: Optional[torch.Tensor] = None):
    """``weighted_sum_dense`` (exact mode, float fold) plus every client's squared
    L2 norm from the same pass: returns ``(out[P], l2sq[K])``."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    K, P = x.shape
    if w.shape != (K,) or w.dtype != torch.float32 or not w.is_contiguous():
        raise TypeError(f"w must be a contiguous float32 tensor of shape ({K},)")
    if out is None:
        out = torch.empty(P, dtype=x.dtype, device=x.device)
    if l2sq is None:
        l2sq = torch.empty(K, dtype=torch.float32, device=x.device)
    dev = _require_device(x, w, out, l2sq)
    need = int(_lib.load().fjagg_wsum_l2_workspace_bytes(K, P))
    flags = (_lib.SCALE if scale is not None else 0) | (_lib.ACCUMULATE if accumulate else 0)
    flags |= _lib.NONTEMPORAL if nontemporal else 0
    if workspace is None and not _L2_COMBINE_LAUNCH:  # a zeroed-counter workspace: the fold's last
        # workgroup combines. The stream's cached one, or under a graph capture one of the capture's
        # own: a capture records the zeroing instead of running it (torch.zeros: a fill kernel every
        # replay runs; a recorded memset acts on the first replay only)
        workspace = (torch.zeros(max(need, 4096), dtype=torch.uint8, device=dev)
                     if torch.cuda.is_current_stream_capturing() else _l2_workspace(dev, need))
        flags |= _lib.ZEROED_WS
    elif workspace is None:
        workspace = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    elif workspace.numel() * workspace.element_size() < need:  # (a caller's workspace: two launches)
        workspace = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjagg_wsum_l2_dense", dtype_code(x.dtype), _lib.F32, dtype_code(out.dtype), x.data_ptr(),
              ld, K, P, w.data_ptr(), float(scale if scale is not None else 1.0), out.data_ptr(),
              l2sq.data_ptr(), flags, workspace.data_ptr(), workspace.numel() * workspace.element_size(),
              _stream_handle(dev))
    return out, l2sq


_L2_WS = {}  # (device index, stream handle) -> fused-norm workspace, counter header zero
# FJAGG_L2_COMBINE_LAUNCH=1: keep the separate norm-combine launch (as fjhost; include/fjagg.h
# FJAGG_ZEROED_WS): the in-launch hand-off follows the HIP guide's measured gfx950 recipe
_L2_COMBINE_LAUNCH = os.environ.get("FJAGG_L2_COMBINE_LAUNCH", "0") == "1"


def _l2_workspace(dev: torch.device, need: int) -> torch.Tensor:
    """The FJAGG_ZEROED_WS workspace of ``dev``'s current stream (fjagg.h): zeroed when it is
    (re)allocated; every fused-norm launch leaves its 16-byte completion counter zero, and
    launches on one stream are ordered, so they share it."""
    key = (dev.index, _stream_handle(dev))
    ws = _L2_WS.get(key)
    if ws is None and len(_L2_WS) >= 16:  # many short-lived streams: keep the cache bounded
        _L2_WS.clear()
    if ws is None or ws.numel() < need:
        ws = _L2_WS[key] = torch.zeros(max(2 * need, 4096), dtype=torch.uint8, device=dev)
    return ws


def split_workspace_bytes(K: int, P: int) -> int:
    return int(_lib.load().fjagg_split_workspace_bytes(K, P))


def ptrs_plan(in_code: int, leaf_n: Sequence[int], unaligned, narrow: bool = False,
              stripe_variant: int = 0) -> np.ndarray:
    """Workgroup table of the pytree kernel (host int64 array, 2 words per workgroup).

    ``unaligned``: a bool for the whole launch (True = element units everywhere; launch
    with ``unaligned=True``), or a per-leaf boolean array: the marked leaves take
    element units, the others 16-byte units (``fjagg_ptrs_plan_leaves``; launch with
    ``unaligned=False``). ``narrow``: 64-element stripes for k_ptrs_narrow (any
    alignment; launch with ``FJAGG_NARROW``); with ``stripe_variant`` 20 / 21 / 22:
    64 / 32 / 16-element stripes for k_ptrs_stripe (16-byte aligned pointers; launch with
    ``FJAGG_NARROW | FJAGG_VARIANT(stripe_variant)``)."""
    lib = _lib.load()
    n = np.ascontiguousarray(leaf_n, dtype=np.int64)
    if narrow:
        flags, mask = _lib.NARROW | ((stripe_variant & 0xFF) << 8), None
    elif isinstance(unaligned, (bool, np.bool_)):
        flags, mask = (_lib.UNALIGNED if unaligned else 0), None
    else:
        mask = np.ascontiguousarray(unaligned, dtype=np.uint8)
        if mask.shape != n.shape:
            raise ValueError(f"per-leaf mask of {mask.shape[0] if mask.ndim else 0} entries for {n.size} leaves")
        flags = 0
    mp = mask.ctypes.data if mask is not None else None
    need = lib.fjagg_ptrs_plan_leaves(in_code, flags, n.ctypes.data, mp, len(n), None, 0)
    _lib.check(0 if need >= 0 else int(need), "fjagg_ptrs_plan_leaves")
    blocks = np.empty(2 * max(need, 1), dtype=np.int64)
    got = lib.fjagg_ptrs_plan_leaves(in_code, flags, n.ctypes.data, mp, len(n), blocks.ctypes.data, need)
    _lib.check(0 if got >= 0 else int(got), "fjagg_ptrs_plan_leaves")
    return blocks[:2 * need]


def weighted_sum_ptrs(in_code: int, acc_code: int, out_code: int, image_dev: torch.Tensor,
                      L: int, K: int, nblk: int, w_dev: torch.Tensor, scale: Optional[float],
                      accumulate: bool = False, unaligned: bool = False,
                      nontemporal: bool = False, narrow: bool = False, stripe_variant: int = 0) -> None:
    """Launch the pytree kernel over a device plan image (see include/fjagg.h); ``narrow`` /
    ``stripe_variant`` as the plan was built (:func:`ptrs_plan`)."""
    dev = _require_device(image_dev, w_dev)
    flags = (_lib.SCALE if scale is not None else 0) | (_lib.ACCUMULATE if accumulate else 0)
    flags |= (_lib.UNALIGNED if unaligned else 0) | (_lib.NONTEMPORAL if nontemporal else 0)
    flags |= (_lib.NARROW | ((stripe_variant & 0xFF) << 8)) if narrow else 0
    _lib.call("fjagg_wsum_ptrs", in_code, acc_code, out_code, image_dev.data_ptr(), L, K, nblk,
              w_dev.data_ptr(), float(scale if scale is not None else 1.0), flags,
              _stream_handle(dev))


def l2_squared_dense(x: torch.Tensor, out: Optional[torch.Tensor] = None,
                     workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-client sum of squares of a [K, P] slab -> float32[K] (tree_util.py:105-108)."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    K, P = x.shape
    dev = _require_device(x)
    if out is None:
        out = torch.empty(K, dtype=torch.float32, device=dev)
    need = int(_lib.load().fjagg_l2sq_workspace_bytes(K, P))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need, 4), dtype=torch.uint8, device=dev)
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjagg_l2sq_dense", dtype_code(x.dtype), x.data_ptr(), ld, K, P, out.data_ptr(),
              workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream_handle(dev))
    return out


def _f32_vector(name: str, t: torch.Tensor, K: int) -> None:
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != (K,) or t.dtype != torch.float32 or not t.is_contiguous():
        raise TypeError(f"{name} must be a contiguous float32 device tensor of shape ({K},)")


def clip_scales(l2sq: torch.Tensor, max_norm: float):
    """``(norms, c)`` of K clients from their squared l2 norms ``l2sq`` (float32 [K] on the
    device): ``norms = sqrt(l2sq)`` and ``c = minimum(1, f32(max_norm) / norms)`` with the
    reference's rounding and NaN propagation (tree_clip_by_global_norm, tree_util.py:131-132),
    in one small launch; nothing visits the host."""
    K = l2sq.numel()
    _f32_vector("l2sq", l2sq, K)
    dev = _require_device(l2sq)
    norms, c = torch.empty_like(l2sq), torch.empty_like(l2sq)
    _lib.call("fjagg_clip_scales", l2sq.data_ptr(), K, float(np.float32(max_norm)), norms.data_ptr(), c.data_ptr(),
              _stream_handle(dev))
    return norms, c


def clipped_sum_dense(x: torch.Tensor, w: torch.Tensor, c: torch.Tensor, *, scale: Optional[float] = None,
                      out: Optional[torch.Tensor] = None, accumulate: bool = False, nontemporal: bool = False,
                      with_clipped_l2sq: bool = False):
    """The exact fold of a float32 slab ``x[K, P]`` with every client's elements multiplied by
    its device factor ``c[k]`` before its weight ``w[k]``: ``fl(fl(c_k x) w_k)`` summed in
    client order (then ``* scale``), the reference's sequence for clipping each delta before
    the weighted mean (tree_util.py:133, :32, :47-54). ``w`` and ``c`` are device float32 [K];
    ``c`` is any such vector (:func:`clip_scales` makes the clip factors).

    ``with_clipped_l2sq=True`` returns ``(out, l2sq_clipped)`` with ``l2sq_clipped[k] =
    sum_p fl(c_k x_k[p])^2`` from the same pass (K <= 4096)."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"the clipped fold takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    _f32_vector("w", w, K)
    _f32_vector("c", c, K)
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=x.device)
    if out.numel() != P or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of P elements")
    dev = _require_device(x, w, c, out)
    flags = (_lib.SCALE if scale is not None else 0) | (_lib.ACCUMULATE if accumulate else 0)
    flags |= _lib.NONTEMPORAL if nontemporal else 0
    l2sq, ws, ws_ptr, ws_bytes = None, None, None, 0
    if with_clipped_l2sq:
        l2sq = torch.empty(K, dtype=torch.float32, device=dev)
        ws_bytes = max(int(_lib.load().fjagg_wsum_clip_workspace_bytes(K, P)), 4)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        ws_ptr = ws.data_ptr()
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjagg_wsum_clip_dense", _lib.F32, x.data_ptr(), ld, K, P, w.data_ptr(), c.data_ptr(),
              float(scale if scale is not None else 1.0), out.data_ptr(), None if l2sq is None else l2sq.data_ptr(),
              flags, ws_ptr, ws_bytes, _stream_handle(dev))
    return (out, l2sq) if with_clipped_l2sq else out


def check_noise_stddev(noise_stddev) -> float:
    """``noise_stddev`` as the float32 value the kernels take; negative, NaN and inf raise."""
    if isinstance(noise_stddev, (bool, str)) or not isinstance(noise_stddev, (int, float, np.integer, np.floating)):
        raise TypeError(f"noise_stddev must be a real number, not {type(noise_stddev).__name__}")
    with np.errstate(over="ignore"):
        sd = float(np.float32(noise_stddev))
    if not (np.isfinite(sd) and sd >= 0.0 and float(noise_stddev) >= 0.0):
        raise ValueError(f"noise_stddev must be finite and >= 0 (as float32), got {noise_stddev}")
    return sd


def refuse_capture(what: str, why: Optional[str] = None) -> None:
    """The differentially private calls bake the noise key into the kernel arguments: a graph
    replay would add the SAME noise every time, which voids the privacy guarantee without any
    visible sign. They raise under stream capture, before anything is recorded. Other calls
    that cannot be captured give their own reason as ``why``."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        if why is None:
            why = ("its noise key is a kernel argument, so a graph replay would reuse the noise and void the "
                   "privacy guarantee")
        raise RuntimeError(f"fedjax_amd: {what} is not capturable: {why}")


_TWO_PASS = ("the selection between its two passes runs on the host over the Gram matrix, so a graph replay "
             "would fold the clients chosen at capture time")


class NoiseTable:
    """``struct fjagg_noise`` for a DP clipped fold: ``stddev`` and one ``{begin, n, k0, k1}``
    entry per leaf (``keys``: uint32 [L, 2], leaf order). More than
    ``FJAGG_NOISE_MAX_LEAVES`` leaves travel as a device table (pytree route only)."""

    def __init__(self, stddev: float, begins, sizes, keys, device: Optional[torch.device] = None):
        L = len(sizes)
        keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(L, 2)
        self.host = (_lib.NoiseLeaf * max(L, 1))()
        for l in range(L):
            self.host[l].begin, self.host[l].n = int(begins[l]), int(sizes[l])
            self.host[l].k0, self.host[l].k1 = int(keys[l, 0]), int(keys[l, 1])
        self.dev = None
        if L > _lib.NOISE_MAX_LEAVES and device is not None:
            raw = np.frombuffer(memoryview(self.host), dtype=np.uint8).copy()
            self.dev = _lib.upload(torch.from_numpy(raw), device)
        self.desc = _lib.Noise(float(stddev), L, ctypes.addressof(self.host),
                               None if self.dev is None else self.dev.data_ptr())

    @property
    def ref(self):
        return ctypes.byref(self.desc)


def dp_clipped_sum_dense(x: torch.Tensor, w: torch.Tensor, c: torch.Tensor, noise: NoiseTable, *, scale: float,
                         out: Optional[torch.Tensor] = None, nontemporal: bool = False,
                         with_clipped_l2sq: bool = False):
    """:func:`clipped_sum_dense` with ``scale`` applied and Gaussian noise added in the fold's
    epilogue (``fjagg_wsum_clip_noise_dense``): element ``i`` of leaf ``l`` of the result is
    ``fl(y + fl(stddev * z_l[i]))``, ``y`` the clipped mean's bits and ``z_l =
    random.normal(keys[l], n_l)``. Elements of a row outside every leaf get no noise. Raises
    under stream capture (:func:`refuse_capture`)."""
    refuse_capture("dp_clipped_sum_dense")
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"the clipped fold takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    _f32_vector("w", w, K)
    _f32_vector("c", c, K)
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=x.device)
    if out.numel() != P or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of P elements")
    dev = _require_device(x, w, c, out)
    flags = _lib.SCALE | (_lib.NONTEMPORAL if nontemporal else 0)
    l2sq, ws, ws_ptr, ws_bytes = None, None, None, 0
    if with_clipped_l2sq:
        l2sq = torch.empty(K, dtype=torch.float32, device=dev)
        ws_bytes = max(int(_lib.load().fjagg_wsum_clip_workspace_bytes(K, P)), 4)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        ws_ptr = ws.data_ptr()
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjagg_wsum_clip_noise_dense", _lib.F32, x.data_ptr(), ld, K, P, w.data_ptr(), c.data_ptr(),
              float(scale), out.data_ptr(), None if l2sq is None else l2sq.data_ptr(), noise.ref, flags, ws_ptr,
              ws_bytes, _stream_handle(dev))
    return (out, l2sq) if with_clipped_l2sq else out


def clip_finish(norms: torch.Tensor, c: torch.Tensor, l2sq_clipped: torch.Tensor):
    """``(clipped_norms, clipped)`` of a clipped fold: ``clipped = (c != 1)`` (bool [K]; true for
    a NaN factor) and the clipped norms — an unclipped client's norm verbatim, else the
    correctly rounded root of ``l2sq_clipped`` (mime_lite.py:139-146). One small launch."""
    K = c.numel()
    for name, t in (("norms", norms), ("c", c), ("l2sq_clipped", l2sq_clipped)):
        _f32_vector(name, t, K)
    dev = _require_device(norms, c, l2sq_clipped)
    clipped_norms = torch.empty_like(norms)
    clipped = torch.empty(K, dtype=torch.bool, device=dev)
    _lib.call("fjagg_clip_finish", norms.data_ptr(), c.data_ptr(), l2sq_clipped.data_ptr(), K,
              clipped_norms.data_ptr(), clipped.data_ptr(), _stream_handle(dev))
    return clipped_norms, clipped


def clip_flags(c: torch.Tensor) -> torch.Tensor:
    """``clipped = (c != 1)`` (bool [K]; true for a NaN factor) alone: :func:`clip_finish` for a
    fold that formed no clipped squares (``fjagg_clip_finish`` with a null clipped-norm output)."""
    K = c.numel()
    _f32_vector("c", c, K)
    dev = _require_device(c)
    clipped = torch.empty(K, dtype=torch.bool, device=dev)
    _lib.call("fjagg_clip_finish", None, c.data_ptr(), None, K, None, clipped.data_ptr(), _stream_handle(dev))
    return clipped


def clipped_update_dense(x: torch.Tensor, w: torch.Tensor, c: torch.Tensor, scale: float, desc, params: torch.Tensor,
                         m: Optional[torch.Tensor] = None, v: Optional[torch.Tensor] = None,
                         mean_out: Optional[torch.Tensor] = None, *, nontemporal: bool = False,
                         with_clipped_l2sq: bool = True) -> Optional[torch.Tensor]:
    """The clipped fold of :func:`clipped_sum_dense` over a float32 slab ``x[K, P]`` with the
    server optimizer step in its epilogue (``fjagg_server_update_clip_dense``): the clipped mean
    ``fl(sum_k fl(fl(c_k x_k) w_k) * scale)`` stays in registers and steps ``params`` (and the
    moments ``m`` / ``v`` the rule of descriptor ``desc`` reads) in place; ``mean_out`` also
    receives it. All tensors are contiguous float32 on the device, ``params`` / ``m`` / ``v`` /
    ``mean_out`` of P elements. Returns ``l2sq_clipped`` (float32 [K], the bits
    :func:`clipped_sum_dense` gives on the same slab; K <= 4096), or None without
    ``with_clipped_l2sq`` (no workspace, no combine launch)."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"the clipped fold takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    _f32_vector("w", w, K)
    _f32_vector("c", c, K)
    state = [t for t in (params, m, v, mean_out) if t is not None]
    for t in state:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != P or not t.is_contiguous():
            raise ValueError(f"params, moments and mean_out must be contiguous float32 tensors of {P} elements")
    dev = _require_device(x, w, c, *state)
    l2sq, ws_ptr, ws_bytes = None, None, 0
    if with_clipped_l2sq:
        l2sq = torch.empty(K, dtype=torch.float32, device=dev)
        ws_bytes = max(int(_lib.load().fjagg_wsum_clip_workspace_bytes(K, P)), 4)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        ws_ptr = ws.data_ptr()
    ptr = lambda t: None if t is None else t.data_ptr()
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjagg_server_update_clip_dense", _lib.F32, x.data_ptr(), ld, K, P, w.data_ptr(), c.data_ptr(),
              float(scale), ctypes.byref(desc), params.data_ptr(), ptr(m), ptr(v), ptr(mean_out), ptr(l2sq),
              _lib.NONTEMPORAL if nontemporal else 0, ws_ptr, ws_bytes, _stream_handle(dev))
    return l2sq


def check_group_ids(group_ids, K: int, num_groups: int) -> np.ndarray:
    """``group_ids`` as an int64 [K] array of ids in ``{-1} | [0, num_groups)``; ValueError for
    anything else (a wrong length, non-integers, ids out of range)."""
    G = int(num_groups)
    if G < 1:
        raise ValueError(f"num_groups must be >= 1, got {num_groups}")
    ids = np.asarray(group_ids)
    if ids.ndim != 1 or ids.shape[0] != K:
        raise ValueError(f"group_ids must hold one id per client ({K}), got shape {ids.shape}")
    if K and ids.dtype.kind not in "iu":
        raise ValueError(f"group_ids must be integers, got {ids.dtype}")
    ids = ids.astype(np.int64)
    if K and (ids.min() < -1 or ids.max() >= G):
        raise ValueError(f"group_ids must be -1 or in [0, {G})")
    return ids


class GroupTables:
    """The member tables of a grouped fold (include/fjagg.h, fjagg_wsum_group_*), built on the
    host with one stable sort and held on the device as ONE buffer
    ``order[M] | seg[G+1] | gorder[G] | wperm[M] | gscale[G]`` (4-byte words).

    ``order`` lists the members (clients whose id is not -1) sorted stably by group, so in
    client order within a group; ``gorder`` lists the groups by descending member count."""

    def __init__(self, w: np.ndarray, ids: np.ndarray, num_groups: int, scales: Optional[np.ndarray]):
        G = int(num_groups)
        members = np.flatnonzero(ids >= 0)
        order = members[np.argsort(ids[members], kind="stable")].astype(np.int32)
        counts = np.bincount(ids[members], minlength=G)
        seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        gorder = np.argsort(-counts, kind="stable").astype(np.int32)
        wperm = np.ascontiguousarray(w, dtype=np.float32)[order]
        gscale = np.ones(G, dtype=np.float32) if scales is None else np.ascontiguousarray(scales, dtype=np.float32)
        if gscale.shape != (G,):
            raise ValueError(f"scales must have shape ({G},), got {gscale.shape}")
        self.G, self.M, self.scaled = G, int(order.size), scales is not None
        self.order, self.seg, self.gorder = order, seg, gorder
        self.host = np.concatenate([order, seg, gorder, wperm.view(np.int32), gscale.view(np.int32)])
        self.dev: Optional[torch.Tensor] = None

    def upload(self, device) -> "GroupTables":
        """One pinned upload, ordered on the current stream (not capturable: :func:`_lib.upload`)."""
        if self.dev is None:
            self.dev = _lib.upload(torch.from_numpy(self.host), device)
        return self

    def ptrs(self):
        """Device addresses of (order, seg, gorder, wperm, gscale)."""
        p, M, G = self.dev.data_ptr(), self.M, self.G
        return p, p + 4 * M, p + 4 * (M + G + 1), p + 4 * (M + 2 * G + 1), p + 4 * (2 * M + 2 * G + 1)


def pack_server_opts(descs: Sequence) -> np.ndarray:
    """``opts[G]`` of struct fjagg_server_opt as int32 words; ``None`` (a group that is not
    folded: its descriptor is never read) packs as zeros."""
    words = ctypes.sizeof(_lib.ServerOpt) // 4
    out = np.zeros((len(descs), words), dtype=np.int32)
    for g, d in enumerate(descs):
        if d is not None:
            out[g] = np.frombuffer(bytes(d), dtype=np.int32)
    return out.reshape(-1)


class GroupUpdateTables:
    """What a grouped fold with the per-cluster server step reads beside the deltas
    (include/fjagg.h, fjagg_server_update_group_*), as ONE buffer and one pinned upload::

        GroupTables' words | opts[G] (struct fjagg_server_opt) | pad to 8 bytes | addrs (int64)

    ``descs``: one descriptor per group (``None`` where the group is not folded); ``addrs``: R
    int64 address tables as an [R, n] array (dense: one [G, 4] table per run of trainable
    columns; pytree: the one [G, 3, L] table). ``tables.dev`` is set to the uploaded buffer,
    whose head is the GroupTables layout, so :meth:`GroupTables.ptrs` and every call that takes
    ``tables`` work on it. The host copies stay here for the entries' checks."""

    def __init__(self, tables: GroupTables, descs: Sequence, addrs: np.ndarray):
        self.tables = tables
        self.opts = pack_server_opts(descs)
        self.addrs = np.ascontiguousarray(addrs, dtype=np.int64)
        if self.addrs.ndim != 2 or len(descs) != tables.G:
            raise ValueError("need one descriptor per group and an [R, n] array of address tables")
        head = tables.host.size + self.opts.size
        self._addr_word = head + (head & 1)
        self.host = np.concatenate([tables.host, self.opts, np.zeros(head & 1, np.int32),
                                    self.addrs.reshape(-1).view(np.int32)])

    def upload(self, device) -> "GroupUpdateTables":
        if self.tables.dev is None:
            self.tables.dev = _lib.upload(torch.from_numpy(self.host), device)
        return self

    def opts_ptr(self) -> int:
        return self.tables.dev.data_ptr() + 4 * self.tables.host.size

    def addrs_ptr(self, run: int = 0) -> int:
        """Device address of address table ``run``."""
        return self.tables.dev.data_ptr() + 4 * self._addr_word + 8 * self.addrs.shape[1] * run


def grouped_update_dense(x: torch.Tensor, up: GroupUpdateTables, run: int = 0, *, nontemporal: bool = False) -> None:
    """One launch of fjagg_server_update_group_dense over the float32 slab columns ``x[K, P]``:
    every folded group's mean and, in the epilogue, its server step through address table
    ``run`` of ``up`` (uploaded). Nothing is returned: the params and moments behind the
    addresses are updated in place."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"the grouped fold takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    t = up.tables
    dev = _require_device(x)
    if t.dev is None or not t.scaled or (t.M and int(t.order.max()) >= K):
        raise ValueError("tables were built for another grouped fold")
    if t.M == 0:
        return
    order_p, seg_p, gorder_p, wperm_p, gscale_p = t.ptrs()
    st = up.addrs[run]
    _lib.call("fjagg_server_update_group_dense", _lib.F32, x.data_ptr(), x.stride(0) if K > 1 else P, K, P, t.M, t.G,
              order_p, seg_p, wperm_p, gscale_p, gorder_p, t.order.ctypes.data, t.seg.ctypes.data, up.opts_ptr(),
              up.addrs_ptr(run), up.opts.ctypes.data, st.ctypes.data,
              _lib.SCALE | (_lib.NONTEMPORAL if nontemporal else 0), _stream_handle(dev))


def grouped_update_dense_shape(x: torch.Tensor, tables: GroupTables) -> int:
    """The kernel shape :func:`grouped_update_dense` runs with for ``x`` [K, P] and these tables
    (fjagg_group_dense_shape without an output: the params and moments need no alignment)."""
    K, P = x.shape
    nonempty = int((np.diff(tables.seg) > 0).sum())
    rc = _lib.load().fjagg_group_dense_shape(x.data_ptr(), x.stride(0) if K > 1 else P, P, tables.M, nonempty,
                                             tables.G, None, (P + 3) // 4 * 4)
    if rc < 0:
        _lib.check(rc, "fjagg_group_dense_shape")
    return rc


def grouped_sum_dense(x: torch.Tensor, w, group_ids, num_groups: int, *, scales=None,
                      out: Optional[torch.Tensor] = None, nontemporal: bool = False,
                      tables: Optional[GroupTables] = None) -> torch.Tensor:
    """Per-group exact folds of a float32 slab ``x[K, P]`` in ONE launch that reads every member
    row once (fjagg_wsum_group_dense; the per-cluster sums of hyp_cluster.py:268-303): client k
    belongs to group ``group_ids[k]`` in ``[0, num_groups)`` or, with -1, to none. Returns
    ``out[G, P]`` (row stride ``out.stride(0)``) with, for group g's members in client order,

        out[g] = fl(fl(+0 + x_m0 * w_m0) + x_m1 * w_m1 + ...) [* scales[g]]

    ``w``: host float32 weights [K]; ``scales``: host float32 [G] or None. The row of a group
    without members is NOT written; a client in no group is never loaded. The result allocated
    here has its rows padded to 16 bytes (a [G, P] view of it is returned); an ``out`` or ``x``
    whose base or row stride is not 16-byte aligned makes the whole launch walk single elements
    (:func:`grouped_dense_shape` tells). The member tables go
    up as one pinned upload (:class:`GroupTables`); pass ``tables`` (already uploaded, built
    from the same ``w``, ``group_ids`` and ``scales``) to launch without one."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"the grouped fold takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    G = int(num_groups)
    dev = _require_device(x)
    if tables is None:
        ids = check_group_ids(group_ids, K, G)
        if isinstance(w, torch.Tensor):
            w = w.detach().cpu().numpy()
        w = np.asarray(w)
        if w.shape != (K,) or w.dtype != np.float32:
            raise TypeError(f"w must be host float32 weights of shape ({K},)")
        tables = GroupTables(w, ids, G, scales)
    elif tables.G != G or tables.dev is None or (tables.M and int(tables.order.max()) >= K):
        raise ValueError("tables were built for another grouped fold")
    if out is None:  # rows padded to 16 bytes, so that the result never forces element units
        out = torch.empty(G, (P + 3) // 4 * 4, dtype=torch.float32, device=dev)[:, :P]
    if out.dim() != 2 or tuple(out.shape) != (G, P) or out.dtype != torch.float32 or out.stride(1) != 1:
        raise ValueError(f"out must be a float32 [{G}, {P}] tensor with unit column stride")
    _require_device(x, out)
    if tables.M == 0:
        return out  # every group is empty: nothing to launch, nothing written
    order_p, seg_p, gorder_p, wperm_p, gscale_p = tables.upload(dev).ptrs()
    flags = (_lib.SCALE if tables.scaled else 0) | (_lib.NONTEMPORAL if nontemporal else 0)
    ld = x.stride(0) if K > 1 else P
    out_ld = out.stride(0) if G > 1 else P
    _lib.call("fjagg_wsum_group_dense", _lib.F32, x.data_ptr(), ld, K, P, tables.M, G, order_p, seg_p, wperm_p,
              gscale_p, gorder_p, tables.order.ctypes.data, tables.seg.ctypes.data, out.data_ptr(), out_ld, flags,
              _stream_handle(dev))
    return out


def grouped_dense_shape(x: torch.Tensor, out: torch.Tensor, tables: GroupTables) -> int:
    """The kernel shape :func:`grouped_sum_dense` runs with for ``x`` [K, P], ``out`` [G, P] and
    these tables (fjagg_group_dense_shape; nothing is launched): 0 = single-element units, else
    16-byte units with 2 = E=1 x U=8, 5 = E=4 x U=4, 12 = E=8 x U=4."""
    K, P = x.shape
    nonempty = int((np.diff(tables.seg) > 0).sum())
    rc = _lib.load().fjagg_group_dense_shape(x.data_ptr(), x.stride(0) if K > 1 else P, P, tables.M, nonempty,
                                             tables.G, out.data_ptr(), out.stride(0) if tables.G > 1 else P)
    if rc < 0:
        _lib.check(rc, "fjagg_group_dense_shape")
    return rc


TRIM_MAX_CLIENTS = 128  # fjagg_trim_*: a column's K values live in one lane (fjagg.h)
_MAX_ROW_BYTES = 1 << 30


def trim_count(trim, K: int) -> int:
    """The trim count ``t`` of a trimmed mean over ``K`` clients, checked: ``trim`` is an int count
    ``t``, or a float fraction ``0 <= beta < 0.5`` giving ``t = floor(beta * K)`` (in double
    precision: 0.29 of 100 is 28, since 0.29 * 100 < 29). Raises ``TypeError`` for a bool or a
    non-number, ``ValueError`` for more than 128 clients, a fraction outside [0, 0.5), or a count
    with ``t < 0`` or ``2t >= K``. Nothing here touches the library."""
    K = int(K)
    if isinstance(trim, (bool, np.bool_)):
        raise TypeError("trim must be an int count or a float fraction in [0, 0.5), not a bool")
    if K < 1:
        raise ValueError(f"a trimmed mean needs at least 1 client, got K = {K}")
    if K > TRIM_MAX_CLIENTS:
        raise ValueError(f"the trimmed mean and median support K <= {TRIM_MAX_CLIENTS} clients, got K = {K}")
    if isinstance(trim, (int, np.integer)):
        t = int(trim)
    elif isinstance(trim, (float, np.floating)):
        beta = float(trim)
        if not (0.0 <= beta < 0.5):
            raise ValueError(f"a trim fraction must be in [0, 0.5), got {trim}")
        t = int(math.floor(beta * K))
    else:
        raise TypeError(f"trim must be an int count or a float fraction in [0, 0.5), not {type(trim).__name__}")
    if t < 0 or 2 * t >= K:
        raise ValueError(f"a trim count needs 0 <= 2t < K: t = {t} leaves no client of K = {K}")
    return t


def trim_dense(x: torch.Tensor, t: int, *, scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
               nontemporal: bool = False) -> torch.Tensor:
    """Coordinate-wise trimmed sum of a float32 slab ``x[K, P]`` (row stride ``x.stride(0)``, unit
    column stride, float32 alignment only): per column the clients of rank ``t .. K-1-t`` in the
    total order of fjagg.h are added in client order, then multiplied by ``scale`` (the trimmed
    mean passes f32(1 / (K - 2t))). One launch of ``fjagg_trim_dense``; there are no weights.
    ``K <= 128``, ``0 <= 2t < K``; everything is checked before the library is touched."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"the trimmed mean takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)):
        raise TypeError("t must be an int trim count")
    t = trim_count(int(t), K)
    if P < 1:
        raise ValueError("x must have at least one column")
    if P * 4 > _MAX_ROW_BYTES:
        raise ValueError("the trimmed mean takes rows of up to 1 GiB")
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=x.device)
    if out.dim() != 1 or out.numel() != P or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of P elements")
    dev = _require_device(x, out)
    flags = (_lib.SCALE if scale is not None else 0) | (_lib.NONTEMPORAL if nontemporal else 0)
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjagg_trim_dense", _lib.F32, x.data_ptr(), ld, K, P, t, float(scale if scale is not None else 1.0),
              out.data_ptr(), flags, _stream_handle(dev))
    return out


def trim_ptrs(image_dev: torch.Tensor, L: int, K: int, nblk: int, t: int, scale: Optional[float], *,
              unaligned: bool = False, nontemporal: bool = False) -> None:
    """Launch ``fjagg_trim_ptrs`` over a device plan image (``in_ptrs[K*L] | out_ptrs[L] |
    leaf_n[L] | blocks[2*nblk]``, the blocks of :func:`ptrs_plan` for float32 leaves):
    :func:`trim_dense`'s arithmetic on every leaf in one launch. ``unaligned`` as the plan was
    made. Checked before the library is touched."""
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)):
        raise TypeError("t must be an int trim count")
    t = trim_count(int(t), K)
    if not isinstance(image_dev, torch.Tensor) or image_dev.dtype != torch.int64 or not image_dev.is_contiguous():
        raise TypeError("image_dev must be a contiguous int64 device tensor")
    L, nblk = int(L), int(nblk)
    if L < 1 or nblk < 1 or image_dev.numel() < K * L + 2 * L + 2 * nblk:
        raise ValueError(f"bad plan: L = {L}, nblk = {nblk}, image of {image_dev.numel()} words")
    dev = _require_device(image_dev)
    flags = (_lib.SCALE if scale is not None else 0) | (_lib.NONTEMPORAL if nontemporal else 0)
    flags |= _lib.UNALIGNED if unaligned else 0
    _lib.call("fjagg_trim_ptrs", _lib.F32, image_dev.data_ptr(), L, K, nblk, t,
              float(scale if scale is not None else 1.0), flags, _stream_handle(dev))


BUCKET_MAX_CLIENTS = 4096  # fjagg_trim_bucket_*: clients behind at most TRIM_MAX_CLIENTS buckets (fjagg.h)


def bucket_count(K: int, s) -> int:
    """The number of buckets ``B = ceil(K / s)`` of ``K`` clients in buckets of ``s``, checked:
    ``TypeError`` for a bool or a non-int ``s``, ``ValueError`` for ``s < 1``, ``K < 1``, more than
    4096 clients or more than 128 buckets. Nothing here touches the library."""
    if isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, np.integer)):
        raise TypeError(f"bucket_size must be an int >= 1, not {type(s).__name__}")
    K, s = int(K), int(s)
    if s < 1:
        raise ValueError(f"bucket_size must be >= 1, got {s}")
    if K < 1:
        raise ValueError(f"bucketing needs at least 1 client, got K = {K}")
    if K > BUCKET_MAX_CLIENTS:
        raise ValueError(f"bucketing supports K <= {BUCKET_MAX_CLIENTS} clients, got K = {K}")
    B = -(-K // s)
    if B > TRIM_MAX_CLIENTS:
        raise ValueError(f"bucketing supports B = ceil(K / bucket_size) <= {TRIM_MAX_CLIENTS} buckets, got B = {B} "
                         f"(K = {K}, bucket_size = {s})")
    return B


def bucket_trim_count(trim, B: int) -> int:
    """:func:`trim_count` over ``B`` buckets: ``trim`` counts buckets, a fraction gives
    ``floor(beta * B)``. The same refusals, worded for buckets."""
    if isinstance(trim, (bool, np.bool_)):
        raise TypeError("trim must be an int count or a float fraction in [0, 0.5), not a bool")
    if isinstance(trim, (int, np.integer)):
        t = int(trim)
    elif isinstance(trim, (float, np.floating)):
        beta = float(trim)
        if not (0.0 <= beta < 0.5):
            raise ValueError(f"a trim fraction must be in [0, 0.5), got {trim}")
        t = int(math.floor(beta * B))
    else:
        raise TypeError(f"trim must be an int count or a float fraction in [0, 0.5), not {type(trim).__name__}")
    if t < 0 or 2 * t >= B:
        raise ValueError(f"a trim count needs 0 <= 2t < B: t = {t} leaves no bucket of B = {B}")
    return t


def bucket_sizes(K: int, s: int) -> np.ndarray:
    """int64 [B]: the member count of every bucket (only the last may be short)."""
    B = bucket_count(K, s)
    s = min(int(s), int(K))
    n = np.full(B, s, np.int64)
    n[-1] = K - (B - 1) * s
    return n


def check_bucket_perm(perm, K: int, *, host_only: bool = False):
    """The client table of a bucketed aggregate, checked without touching the library: ``None``
    (the identity), an int32 device tensor of ``K`` entries (returned as it is and never read
    here: the kernel clamps its entries), or a host int sequence or array, which must be a
    permutation of ``range(K)`` and is returned as an int32 array. ``host_only`` refuses the
    device tensor (the Gram-matrix rules select on the host)."""
    if perm is None:
        return None
    if isinstance(perm, torch.Tensor) and perm.is_cuda:
        if host_only:
            raise TypeError("the bucketed selection runs on the host: perm must be a host sequence or None")
        if perm.dtype != torch.int32 or perm.dim() != 1 or perm.numel() != K or not perm.is_contiguous():
            raise ValueError(f"a device perm must be a contiguous int32 tensor of K = {K} entries")
        return perm
    a = perm.numpy() if isinstance(perm, torch.Tensor) else np.asarray(perm)
    if a.dtype == np.bool_ or a.dtype.kind not in "iu":
        raise TypeError(f"perm must hold ints, got dtype {a.dtype}")
    if a.ndim != 1 or a.size != K:
        raise ValueError(f"perm must be a permutation of range({K}), got shape {a.shape}")
    a = a.astype(np.int64)
    if not np.array_equal(np.sort(a), np.arange(K)):
        raise ValueError(f"perm must be a permutation of range({K})")
    return np.ascontiguousarray(a.astype(np.int32))


def bucket_perm_device(perm, device: torch.device) -> Optional[torch.Tensor]:
    """:func:`check_bucket_perm`'s result on ``device``: a host table is uploaded (which a stream
    capture refuses), a device tensor must already live there."""
    if perm is None:
        return None
    if isinstance(perm, np.ndarray):
        return _lib.upload(torch.from_numpy(perm), device)
    if perm.device != device:
        raise ValueError(f"perm lives on {perm.device}, the deltas on {device}")
    return perm


def _check_bucket_launch(K: int, s, t, perm) -> Tuple[int, int, int]:
    B = bucket_count(K, s)
    if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)):
        raise TypeError("t must be an int trim count")
    t = bucket_trim_count(int(t), B)
    if perm is not None and (not isinstance(perm, torch.Tensor) or not perm.is_cuda or perm.dtype != torch.int32
                             or perm.dim() != 1 or perm.numel() != K or not perm.is_contiguous()):
        raise ValueError(f"perm must be None or a contiguous int32 device tensor of K = {K} entries")
    return B, int(s), t


def trim_bucket_dense(x: torch.Tensor, s: int, t: int, *, perm: Optional[torch.Tensor] = None,
                      scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
                      nontemporal: bool = False) -> torch.Tensor:
    """:func:`trim_dense` over the means of buckets of ``s`` clients (fjagg.h,
    ``fjagg_trim_bucket_dense``): bucket ``j`` holds the rows ``perm[j*s] .. perm[j*s + n_j - 1]``
    (``perm``: an int32 device tensor of ``K`` entries, never read by the host; ``None``: the
    identity), its mean is formed in float32 in table order, and ``t`` trims buckets. ``K <=
    4096``, ``B = ceil(K / s) <= 128``, ``0 <= 2t < B``; the trimmed mean passes ``scale =
    f32(1 / (B - 2t))``. One launch, nothing uploaded; everything is checked before the library
    is touched."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"the trimmed mean takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    _, s, t = _check_bucket_launch(K, s, t, perm)
    if P < 1:
        raise ValueError("x must have at least one column")
    if P * 4 > _MAX_ROW_BYTES:
        raise ValueError("the trimmed mean takes rows of up to 1 GiB")
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=x.device)
    if out.dim() != 1 or out.numel() != P or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of P elements")
    dev = _require_device(x, out) if perm is None else _require_device(x, out, perm)
    flags = (_lib.SCALE if scale is not None else 0) | (_lib.NONTEMPORAL if nontemporal else 0)
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjagg_trim_bucket_dense", _lib.F32, x.data_ptr(), ld, K, P, None if perm is None else perm.data_ptr(),
              s, t, float(scale if scale is not None else 1.0), out.data_ptr(), flags, _stream_handle(dev))
    return out


def trim_bucket_ptrs(image_dev: torch.Tensor, L: int, K: int, nblk: int, s: int, t: int, scale: Optional[float], *,
                     perm: Optional[torch.Tensor] = None, unaligned: bool = False,
                     nontemporal: bool = False) -> None:
    """Launch ``fjagg_trim_bucket_ptrs`` over a device plan image holding all ``K`` clients (as
    :func:`trim_ptrs` takes it): :func:`trim_bucket_dense`'s arithmetic on every leaf in one
    launch. Checked before the library is touched."""
    K = int(K)
    _, s, t = _check_bucket_launch(K, s, t, perm)
    if not isinstance(image_dev, torch.Tensor) or image_dev.dtype != torch.int64 or not image_dev.is_contiguous():
        raise TypeError("image_dev must be a contiguous int64 device tensor")
    L, nblk = int(L), int(nblk)
    if L < 1 or nblk < 1 or image_dev.numel() < K * L + 2 * L + 2 * nblk:
        raise ValueError(f"bad plan: L = {L}, nblk = {nblk}, image of {image_dev.numel()} words")
    dev = _require_device(image_dev) if perm is None else _require_device(image_dev, perm)
    flags = (_lib.SCALE if scale is not None else 0) | (_lib.NONTEMPORAL if nontemporal else 0)
    flags |= _lib.UNALIGNED if unaligned else 0
    _lib.call("fjagg_trim_bucket_ptrs", _lib.F32, image_dev.data_ptr(), L, K, nblk,
              None if perm is None else perm.data_ptr(), s, t, float(scale if scale is not None else 1.0), flags,
              _stream_handle(dev))


MEAMED_MAX_SLAB_ROWS = 1024  # fjagg_meamed_dense: the slab a row table selects from (the Gram pass's limit)


def keep_count(keep, K: int) -> int:
    """The keep count ``beta`` of a mean around the median over ``K`` participating clients,
    checked: an int in ``[1, K]``. Raises ``TypeError`` for a bool or a non-int, ``ValueError``
    for ``K`` outside ``[1, 128]`` or a count out of range. Nothing here touches the library."""
    K = int(K)
    if isinstance(keep, (bool, np.bool_)) or not isinstance(keep, (int, np.integer)):
        raise TypeError(f"keep must be an int count, not {type(keep).__name__}")
    if K < 1:
        raise ValueError(f"a mean around the median needs at least 1 client, got K = {K}")
    if K > TRIM_MAX_CLIENTS:
        raise ValueError(f"the mean around the median supports K <= {TRIM_MAX_CLIENTS} participating clients, "
                         f"got K = {K}")
    if not (1 <= int(keep) <= K):
        raise ValueError(f"keep must be in [1, K] = [1, {K}], got {keep}")
    return int(keep)


def _row_table(rows, K_rows: int) -> np.ndarray:
    """``rows`` as the int32 table ``fjagg_meamed_dense`` takes: strictly ascending indices into
    a slab of ``K_rows`` rows, at most 128 of them."""
    if isinstance(rows, torch.Tensor):
        rows = rows.cpu().numpy()
    table = np.asarray(rows)
    if table.ndim != 1 or not (1 <= table.size <= TRIM_MAX_CLIENTS):
        raise ValueError(f"rows must name between 1 and {TRIM_MAX_CLIENTS} slab rows, got shape {table.shape}")
    if table.dtype == np.bool_ or not np.issubdtype(table.dtype, np.integer):
        raise TypeError("rows must be a sequence of int row indices")
    table = table.astype(np.int64)
    if table[0] < 0 or table[-1] >= K_rows or (np.diff(table) <= 0).any():
        raise ValueError(f"rows must be strictly ascending in [0, K) = [0, {K_rows})")
    return np.ascontiguousarray(table, dtype=np.int32)


def meamed_dense(x: torch.Tensor, keep: int, rows=None, *, scale: Optional[float] = None,
                 out: Optional[torch.Tensor] = None, nontemporal: bool = False) -> torch.Tensor:
    """Coordinate-wise sum around the median of a float32 slab ``x[K, P]`` (row stride
    ``x.stride(0)``, unit column stride, float32 alignment only): per column the ``keep`` values
    closest to the column's lower median (fjagg.h: a tie keeps the lower side) are added in
    client order, then multiplied by ``scale`` (the mean passes f32(1 / keep)). ``rows``: the
    participating slab rows, strictly ascending, at most 128 of a slab of up to 1024 (default:
    all ``K <= 128`` rows); the table travels in the kernel arguments, so nothing is uploaded
    and no other row is read. One launch of ``fjagg_meamed_dense``; there are no weights.
    Everything is checked before the library is touched."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"the mean around the median takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    if rows is not None:
        if not (1 <= K <= MEAMED_MAX_SLAB_ROWS):
            raise ValueError(f"a row table selects from a slab of 1 <= K <= {MEAMED_MAX_SLAB_ROWS} rows, got K = {K}")
        table = _row_table(rows, K)
    else:
        table = None
    M = K if table is None else int(table.size)
    keep = keep_count(keep, M)
    if P < 1:
        raise ValueError("x must have at least one column")
    if P * 4 > _MAX_ROW_BYTES:
        raise ValueError("the mean around the median takes rows of up to 1 GiB")
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=x.device)
    if out.dim() != 1 or out.numel() != P or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of P elements")
    dev = _require_device(x, out)
    flags = (_lib.SCALE if scale is not None else 0) | (_lib.NONTEMPORAL if nontemporal else 0)
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjagg_meamed_dense", _lib.F32, x.data_ptr(), ld, K, P, None if table is None else table.ctypes.data,
              M, keep, float(scale if scale is not None else 1.0), out.data_ptr(), flags, _stream_handle(dev))
    return out


def meamed_ptrs(image_dev: torch.Tensor, L: int, K: int, nblk: int, keep: int, scale: Optional[float], *,
                unaligned: bool = False, nontemporal: bool = False) -> None:
    """Launch ``fjagg_meamed_ptrs`` over a device plan image (as :func:`trim_ptrs` takes it,
    holding only the ``K`` participating clients): :func:`meamed_dense`'s arithmetic on every
    leaf in one launch. ``unaligned`` as the plan was made. Checked before the library is
    touched."""
    keep = keep_count(keep, K)
    if not isinstance(image_dev, torch.Tensor) or image_dev.dtype != torch.int64 or not image_dev.is_contiguous():
        raise TypeError("image_dev must be a contiguous int64 device tensor")
    L, nblk = int(L), int(nblk)
    if L < 1 or nblk < 1 or image_dev.numel() < K * L + 2 * L + 2 * nblk:
        raise ValueError(f"bad plan: L = {L}, nblk = {nblk}, image of {image_dev.numel()} words")
    dev = _require_device(image_dev)
    flags = (_lib.SCALE if scale is not None else 0) | (_lib.NONTEMPORAL if nontemporal else 0)
    flags |= _lib.UNALIGNED if unaligned else 0
    _lib.call("fjagg_meamed_ptrs", _lib.F32, image_dev.data_ptr(), L, K, nblk, keep,
              float(scale if scale is not None else 1.0), flags, _stream_handle(dev))


GRAM_MAX_CLIENTS = 1024  # fjagg_gram_*: G is K x K float64, at most 8 MiB (fjagg.h)
GRAM_CHAIN = 256  # FJAGG_GRAM_CHAIN: columns per float32 fmaf chain, between float64 additions
_GRAM_WS = {}  # device index -> workspace of the Gram pass (partial sums per workgroup chunk)


def _gram_workspace(dev: torch.device, need: int) -> torch.Tensor:
    """The Gram pass's workspace of ``dev``'s current stream, cached like :func:`_l2_workspace`:
    launches on one stream are ordered, so they share it. Never zeroed; nothing is carried
    from one call to the next."""
    key = (dev.index, _stream_handle(dev))
    ws = _GRAM_WS.get(key)
    if ws is None and len(_GRAM_WS) >= 16:
        _GRAM_WS.clear()
    if ws is None or ws.numel() < need:
        ws = _GRAM_WS[key] = torch.empty(max(need, 4096), dtype=torch.uint8, device=dev)
    return ws


def _check_gram_clients(K: int) -> int:
    K = int(K)
    if K < 1:
        raise ValueError(f"the Gram matrix needs at least 1 client, got K = {K}")
    if K > GRAM_MAX_CLIENTS:
        raise ValueError(f"the Gram matrix supports K <= {GRAM_MAX_CLIENTS} clients, got K = {K}")
    return K


def _check_gram_out(out: Optional[torch.Tensor], K: int, dev: torch.device) -> torch.Tensor:
    if out is None:
        return torch.empty(K, K, dtype=torch.float64, device=dev)
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != (K, K) or out.dtype != torch.float64 \
            or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float64 [{K}, {K}] tensor")
    return out


def gram_chunk_columns(K: int, P: int) -> int:
    """Columns one workgroup of :func:`gram_dense` covers for a ``[K, P]`` slab: a multiple of
    ``GRAM_CHAIN`` and a function of ``(K, P)`` alone (``fjagg_gram_chunk_columns``)."""
    K = _check_gram_clients(K)
    if int(P) < 1:
        raise ValueError("P must be >= 1")
    return int(_lib.load().fjagg_gram_chunk_columns(K, int(P)))


def gram_dense(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gram matrix ``G[i][j] = sum_p x[i, p] * x[j, p]`` of a float32 slab ``x[K, P]`` (row
    stride ``x.stride(0)``, unit column stride, float32 alignment only) as a float64 ``[K, K]``
    device tensor: ``fjagg_gram_dense``, one pass over the slab on the f32 matrix instruction
    plus a small combine launch, no host synchronisation. Chains of ``GRAM_CHAIN`` columns
    accumulate in float32 (an fmaf chain), chains add up in float64 in a fixed order: bitwise
    reproducible, bitwise symmetric, a non-finite client confined to its row and column
    (fjagg.h). ``K <= 1024``; everything is checked before the library is touched."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"the Gram matrix takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    K = _check_gram_clients(K)
    if P < 1:
        raise ValueError("x must have at least one column")
    if P * 4 > _MAX_ROW_BYTES:
        raise ValueError("the Gram matrix takes rows of up to 1 GiB")
    dev = _require_device(x)
    out = _check_gram_out(out, K, dev)
    _require_device(x, out)
    need = int(_lib.load().fjagg_gram_workspace_bytes(K, P, 0))
    ws = _gram_workspace(dev, need)
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjagg_gram_dense", _lib.F32, x.data_ptr(), ld, K, P, out.data_ptr(), ws.data_ptr(), ws.numel(), 0,
              _stream_handle(dev))
    return out


def gram_ptrs(image_dev: torch.Tensor, L: int, K: int, nblk: int, out: Optional[torch.Tensor] = None, *,
              unaligned: bool = False) -> torch.Tensor:
    """:func:`gram_dense`'s arithmetic over a device plan image (``in_ptrs[K*L] | out_ptrs[L] |
    leaf_n[L] | blocks[2*nblk]``, the blocks of :func:`ptrs_plan` for float32 leaves;
    ``out_ptrs`` is not read): ``fjagg_gram_ptrs``, G summed over all leaves, a chain never
    crossing a leaf. ``unaligned`` as the plan was made. Checked before the library is touched."""
    K = _check_gram_clients(K)
    if not isinstance(image_dev, torch.Tensor) or image_dev.dtype != torch.int64 or not image_dev.is_contiguous():
        raise TypeError("image_dev must be a contiguous int64 device tensor")
    L, nblk = int(L), int(nblk)
    if L < 1 or nblk < 1 or image_dev.numel() < K * L + 2 * L + 2 * nblk:
        raise ValueError(f"bad plan: L = {L}, nblk = {nblk}, image of {image_dev.numel()} words")
    dev = _require_device(image_dev)
    out = _check_gram_out(out, K, dev)
    _require_device(image_dev, out)
    need = int(_lib.load().fjagg_gram_workspace_bytes(K, 0, nblk))
    ws = _gram_workspace(dev, need)
    _lib.call("fjagg_gram_ptrs", _lib.F32, image_dev.data_ptr(), L, K, nblk, out.data_ptr(), ws.data_ptr(),
              ws.numel(), _lib.UNALIGNED if unaligned else 0, _stream_handle(dev))
    return out


class DeviceGroupTables(NamedTuple):
    """The member tables of ONE group as a select kernel wrote them (fjagg.h: ``order[M_max]``,
    ``seg[2]``, ``wperm[M_max]``, ``gscale[1]``, all on the device) and the bound ``M_max`` on
    the member count that the fold's kernel shape is picked from."""
    order: torch.Tensor
    seg: torch.Tensor
    wperm: torch.Tensor
    gscale: torch.Tensor
    M_max: int


def _check_select_gram(gram: torch.Tensor) -> int:
    if not isinstance(gram, torch.Tensor) or gram.dim() != 2 or gram.shape[0] != gram.shape[1] \
            or gram.dtype != torch.float64 or not gram.is_contiguous():
        raise ValueError("gram must be a contiguous float64 [K, K] device tensor")
    K = _check_gram_clients(gram.shape[0])
    _require_device(gram)
    return K


def _select_tables(M_max: int, dev: torch.device) -> DeviceGroupTables:
    ints = torch.empty(M_max + 2, dtype=torch.int32, device=dev)  # order | seg
    floats = torch.empty(M_max + 1, dtype=torch.float32, device=dev)  # wperm | gscale
    return DeviceGroupTables(ints[:M_max], ints[M_max:], floats[:M_max], floats[M_max:], M_max)


def krum_select_device(gram: torch.Tensor, f: int, m: int):
    """Krum / multi-Krum's selection on the device over a float64 ``[K, K]`` Gram matrix
    (``fjagg_krum_select``): bit for bit :func:`fedjax_amd.robust.krum_scores` and
    ``krum_select`` of the same matrix. Returns ``(scores, selected, count, tables)``, all on
    the device: ``scores`` float64 [K]; ``selected`` int64 [m], best first, -1 padded; ``count``
    int32 scalar, the number of finite scores taken; ``tables`` the
    :class:`DeviceGroupTables` of :func:`grouped_sum_dense_device` (members in ascending client
    index, unit weights, ``gscale = f32(1 / count)``). Two small launches, no host
    synchronisation, nothing uploaded: capturable. ``K >= 2f + 3``, ``1 <= m <= K - f``."""
    from fedjax_amd import robust

    K = _check_select_gram(gram)
    f, m = robust.check_krum_args(K, f, m)  # the host route's argument checks and exceptions
    dev = gram.device
    scores = torch.empty(K, dtype=torch.float64, device=dev)
    selected = torch.empty(m, dtype=torch.int64, device=dev)
    count = torch.empty((), dtype=torch.int32, device=dev)
    tables = _select_tables(m, dev)
    _lib.call("fjagg_krum_select", gram.data_ptr(), K, f, m, scores.data_ptr(), selected.data_ptr(), count.data_ptr(),
              tables.order.data_ptr(), tables.seg.data_ptr(), tables.wperm.data_ptr(), tables.gscale.data_ptr(),
              _stream_handle(dev))
    return scores, selected, count, tables


def weiszfeld_select_device(gram: torch.Tensor, alpha=None, nu: float = 1e-6, iterations: int = 4):
    """The smoothed Weiszfeld iteration on the device over a float64 ``[K, K]`` Gram matrix
    (``fjagg_weiszfeld_select``; the rule of :func:`fedjax_amd.robust.weiszfeld_weights` with
    the order of every sum pinned: over the usable clients in ascending index, sequentially).
    ``alpha``: ``None`` for unit weights (nothing is uploaded), a float64 ``[K]`` device tensor,
    or host numbers, which are checked as the host route checks them and uploaded once (refused
    under stream capture). Returns ``(a, d, a32, count, tables)``, all on the device: the final
    weights and last distances (float64 [K]), ``a32 = float32(a)``, the number of clients with
    ``a32 > 0`` (int32 scalar) and the :class:`DeviceGroupTables` of the fold (those clients in
    ascending index, ``wperm = a32``, ``gscale = f32(1 / sum a32)``). One launch of one
    workgroup, no host synchronisation."""
    from fedjax_amd import robust

    K = _check_select_gram(gram)
    dev = gram.device
    if isinstance(alpha, torch.Tensor):
        if alpha.dtype != torch.float64 or tuple(alpha.shape) != (K,) or not alpha.is_contiguous():
            raise ValueError(f"a device alpha must be a contiguous float64 [{K}] tensor")
        _require_device(gram, alpha)
        robust.weiszfeld_weights(np.eye(1), None, nu, iterations)
        alpha_dev = alpha
    else:
        host = None if alpha is None else np.asarray(alpha)
        robust.weiszfeld_weights(np.eye(1) if host is None else np.eye(K), host, nu, 0)
        robust.weiszfeld_weights(np.eye(1), None, nu, iterations)
        alpha_dev = None if host is None else _lib.upload(torch.from_numpy(host.astype(np.float64)), dev)
    a = torch.empty(K, dtype=torch.float64, device=dev)
    d = torch.empty(K, dtype=torch.float64, device=dev)
    a32 = torch.empty(K, dtype=torch.float32, device=dev)
    count = torch.empty((), dtype=torch.int32, device=dev)
    tables = _select_tables(K, dev)
    _lib.call("fjagg_weiszfeld_select", gram.data_ptr(), K, 0 if alpha_dev is None else alpha_dev.data_ptr(),
              float(nu), int(iterations), a.data_ptr(), d.data_ptr(), a32.data_ptr(), count.data_ptr(),
              tables.order.data_ptr(), tables.seg.data_ptr(), tables.wperm.data_ptr(), tables.gscale.data_ptr(),
              _stream_handle(dev))
    return a, d, a32, count, tables


def grouped_sum_dense_device(x: torch.Tensor, tables: DeviceGroupTables, out: torch.Tensor, *,
                             nontemporal: bool = False) -> torch.Tensor:
    """The scaled exact fold of ONE group of a float32 slab ``x[K, P]`` whose member tables a
    select kernel wrote (``fjagg_wsum_group_dense_dev``): :func:`grouped_sum_dense`'s arithmetic
    and kernels, no host copy of the tables, nothing uploaded. ``out``: float32 ``[P]``; a group
    without members writes nothing, so the caller zeroes ``out`` first."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"the grouped fold takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    if tuple(out.shape) != (P,) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 [{P}] tensor")
    dev = _require_device(x, out, tables.order, tables.seg, tables.wperm, tables.gscale)
    _lib.call("fjagg_wsum_group_dense_dev", _lib.F32, x.data_ptr(), x.stride(0) if K > 1 else P, K, P, tables.M_max,
              tables.order.data_ptr(), tables.seg.data_ptr(), tables.wperm.data_ptr(), tables.gscale.data_ptr(),
              out.data_ptr(), _lib.SCALE | (_lib.NONTEMPORAL if nontemporal else 0), _stream_handle(dev))
    return out


def grouped_sum_ptrs_device(image_all: torch.Tensor, image_group: torch.Tensor, L: int, K: int, nblk: int,
                            tables: DeviceGroupTables, *, nontemporal: bool = False) -> None:
    """The same over a pytree plan: ``fjagg_gather_member_ptrs`` copies the members' leaf
    pointers from ``image_all`` (``in_ptrs[K*L]``, the Gram pass's image) into ``image_group``
    (``in_ptrs[M_max*L] | out_ptrs[L] | leaf_n[L] | blocks[2*nblk]``), then
    ``fjagg_wsum_group_ptrs_dev`` folds them into ``out_ptrs``."""
    for name, t in (("image_all", image_all), ("image_group", image_group)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous int64 device tensor")
    L, K, nblk, M = int(L), int(K), int(nblk), tables.M_max
    if L < 1 or nblk < 1 or image_all.numel() < K * L or image_group.numel() < M * L + 2 * L + 2 * nblk:
        raise ValueError(f"bad plan: L = {L}, nblk = {nblk}, images of {image_all.numel()} and "
                         f"{image_group.numel()} words")
    dev = _require_device(image_all, image_group, tables.seg, tables.wperm, tables.gscale)
    s = _stream_handle(dev)
    _lib.call("fjagg_gather_member_ptrs", image_all.data_ptr(), L, K, tables.order.data_ptr(), tables.seg.data_ptr(),
              M, image_group.data_ptr(), s)
    _lib.call("fjagg_wsum_group_ptrs_dev", _lib.F32, image_group.data_ptr(), L, K, M, nblk, tables.seg.data_ptr(),
              tables.wperm.data_ptr(), tables.gscale.data_ptr(),
              _lib.SCALE | (_lib.NONTEMPORAL if nontemporal else 0), s)


BULYAN_MAX_SELECTED = TRIM_MAX_CLIENTS  # theta = K - 2f: what the second stage's column routine takes
_BULYAN_WS = {}  # (device index, stream handle) -> workspace of fjagg_bulyan_select (the sorted rows)


class DeviceRowTables(NamedTuple):
    """What ``fjagg_bulyan_select`` leaves for the second stage (fjagg.h), all on the device:
    ``rows`` int32 [M_max], the chosen slab rows ascending, the last repeated past the count;
    ``count`` / ``keep`` int32 scalars; ``scale`` float32 scalar, f32(1 / keep) or 0; and the
    bound ``M_max`` on the count that the second stage's kernel width is picked from."""
    rows: torch.Tensor
    count: torch.Tensor
    keep: torch.Tensor
    scale: torch.Tensor
    M_max: int


def _bulyan_workspace(dev: torch.device, need: int) -> torch.Tensor:
    """The select's workspace on ``dev``'s current stream, cached like :func:`_gram_workspace`;
    under stream capture a tensor of the graph's own pool, which is not kept. Never zeroed,
    nothing carried between calls."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(need, 4096), dtype=torch.uint8, device=dev)
    key = (dev.index, _stream_handle(dev))
    ws = _BULYAN_WS.get(key)
    if ws is None and len(_BULYAN_WS) >= 16:
        _BULYAN_WS.clear()
    if ws is None or ws.numel() < need:
        ws = _BULYAN_WS[key] = torch.empty(max(need, 4096), dtype=torch.uint8, device=dev)
    return ws


def check_bulyan_args(K: int, f) -> int:
    """Bulyan's conditions on the client count alone, with the host route's exceptions and
    nothing computed: ``1 <= K <= 1024``, an int ``f >= 0`` (a bool is refused),
    ``K >= 4f + 3`` and ``K - 2f <= 128``. Returns ``f``."""
    from fedjax_amd import robust

    _check_gram_clients(K)
    f = robust.check_bulyan(K, f)
    if K - 2 * f > BULYAN_MAX_SELECTED:
        raise ValueError(f"Bulyan's second stage takes K - 2f <= {BULYAN_MAX_SELECTED} selected clients, "
                         f"got K = {K}, f = {f}")
    return f


def bulyan_select_device(gram: torch.Tensor, f: int):
    """Bulyan's first stage on the device over a float64 ``[K, K]`` Gram matrix
    (``fjagg_bulyan_select``): bit for bit :func:`fedjax_amd.robust.bulyan_select` of the same
    matrix. Returns ``(selected, count, step_scores, tables)``, all on the device: ``selected``
    int64 [theta], selection order, -1 padded (``theta = K - 2f``); ``count`` int32 scalar;
    ``step_scores`` float64 [theta], each step's winning score, +inf padded; ``tables`` the
    :class:`DeviceRowTables` of :func:`meamed_dense_device` (``keep = count - 2f`` or 0). Two
    small launches, no host synchronisation, nothing uploaded: capturable. ``K >= 4f + 3``,
    ``K - 2f <= 128``."""
    K = _check_select_gram(gram)
    f = check_bulyan_args(K, f)  # the host route's argument checks and exceptions
    dev, theta = gram.device, K - 2 * f
    selected = torch.empty(theta, dtype=torch.int64, device=dev)
    step_scores = torch.empty(theta, dtype=torch.float64, device=dev)
    ints = torch.empty(theta + 2, dtype=torch.int32, device=dev)  # rows | count | keep
    scale = torch.empty((), dtype=torch.float32, device=dev)
    tables = DeviceRowTables(ints[:theta], ints[theta], ints[theta + 1], scale, theta)
    need = int(_lib.load().fjagg_bulyan_select_workspace_bytes(K))
    ws = _bulyan_workspace(dev, need)
    _lib.call("fjagg_bulyan_select", gram.data_ptr(), K, f, ws.data_ptr(), ws.numel(), selected.data_ptr(),
              tables.count.data_ptr(), step_scores.data_ptr(), tables.keep.data_ptr(), scale.data_ptr(),
              tables.rows.data_ptr(), _stream_handle(dev))
    return selected, tables.count, step_scores, tables


def _check_row_tables(tables: DeviceRowTables) -> int:
    M = int(tables.M_max)
    if not (1 <= M <= TRIM_MAX_CLIENTS):
        raise ValueError(f"the mean around the median supports 1 <= M_max <= {TRIM_MAX_CLIENTS} participating "
                         f"clients, got M_max = {M}")
    for name, t, dtype, n in (("rows", tables.rows, torch.int32, M), ("count", tables.count, torch.int32, 1),
                              ("keep", tables.keep, torch.int32, 1), ("scale", tables.scale, torch.float32, 1)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.numel() < n or not t.is_contiguous():
            raise ValueError(f"tables.{name} must be a contiguous {dtype} device tensor of at least {n} elements")
    return M


def meamed_dense_device(x: torch.Tensor, tables: DeviceRowTables, *, out: Optional[torch.Tensor] = None,
                        nontemporal: bool = False) -> torch.Tensor:
    """:func:`meamed_dense` over a float32 slab ``x[K, P]`` with the participating rows, their
    count, the keep count and the scale read from device memory (``fjagg_meamed_dense_dev``):
    the same column routine and bits, no host copy of the tables, nothing uploaded. The kernel
    clamps the count into ``[0, M_max]``, keep into ``[0, count]`` and every row into ``[0, K)``;
    ``keep < 1`` writes +0 everywhere and loads no row. Checked before the library is touched."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"the mean around the median takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    if not (1 <= K <= MEAMED_MAX_SLAB_ROWS):
        raise ValueError(f"a row table selects from a slab of 1 <= K <= {MEAMED_MAX_SLAB_ROWS} rows, got K = {K}")
    M = _check_row_tables(tables)
    if M > K:
        raise ValueError(f"M_max must be <= K = {K}, got {M}")
    if P < 1:
        raise ValueError("x must have at least one column")
    if P * 4 > _MAX_ROW_BYTES:
        raise ValueError("the mean around the median takes rows of up to 1 GiB")
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=x.device)
    if out.dim() != 1 or out.numel() != P or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of P elements")
    dev = _require_device(x, out, tables.rows, tables.count, tables.keep, tables.scale)
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjagg_meamed_dense_dev", _lib.F32, x.data_ptr(), ld, K, P, M, tables.rows.data_ptr(),
              tables.count.data_ptr(), tables.keep.data_ptr(), tables.scale.data_ptr(), out.data_ptr(),
              _lib.SCALE | (_lib.NONTEMPORAL if nontemporal else 0), _stream_handle(dev))
    return out


def meamed_ptrs_device(image_all: torch.Tensor, image_group: torch.Tensor, L: int, K: int, nblk: int,
                       tables: DeviceRowTables, *, nontemporal: bool = False) -> None:
    """The same over a pytree plan (``fjagg_meamed_ptrs_dev``): the chosen clients' leaf pointers
    are gathered on the device from ``image_all`` (``in_ptrs[K*L]``, the Gram pass's image) into
    every member slot of ``image_group`` (``in_ptrs[M_max*L] | out_ptrs[L] | leaf_n[L] |
    blocks[2*nblk]``), then one launch covers every leaf."""
    for name, t in (("image_all", image_all), ("image_group", image_group)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous int64 device tensor")
    M = _check_row_tables(tables)
    L, K, nblk = int(L), int(K), int(nblk)
    if not (1 <= K <= MEAMED_MAX_SLAB_ROWS) or M > K:
        raise ValueError(f"need 1 <= M_max <= K <= {MEAMED_MAX_SLAB_ROWS}, got M_max = {M}, K = {K}")
    if L < 1 or nblk < 1 or image_all.numel() < K * L or image_group.numel() < M * L + 2 * L + 2 * nblk:
        raise ValueError(f"bad plan: L = {L}, nblk = {nblk}, images of {image_all.numel()} and "
                         f"{image_group.numel()} words")
    dev = _require_device(image_all, image_group, tables.rows, tables.count, tables.keep, tables.scale)
    _lib.call("fjagg_meamed_ptrs_dev", _lib.F32, image_all.data_ptr(), image_group.data_ptr(), L, K, M, nblk,
              tables.rows.data_ptr(), tables.count.data_ptr(), tables.keep.data_ptr(), tables.scale.data_ptr(),
              _lib.SCALE | (_lib.NONTEMPORAL if nontemporal else 0), _stream_handle(dev))


def check_select(select) -> bool:
    """``select="host" | "device"`` of the Krum and geometric-median surfaces: True for the
    device route; ValueError for anything else."""
    if select == "host":
        return False
    if select == "device":
        return True
    raise ValueError(f'select must be "host" or "device", got {select!r}')


CENTER_MAX_CLIENTS = 4096  # fjagg_center_*: the clipped fold's client limit (fjagg.h)
_CENTER_WS = {}  # (device index, stream handle) -> workspace of a centered-clipping round


def _center_workspace(dev: torch.device, need: int) -> torch.Tensor:
    """The workspace of a centered-clipping round on ``dev``'s current stream (squared norms and
    their block partials), cached like :func:`_gram_workspace`; under stream capture a tensor of
    the graph's own pool, which is not kept. Never zeroed, nothing carried between calls."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(need, 4096), dtype=torch.uint8, device=dev)
    key = (dev.index, _stream_handle(dev))
    ws = _CENTER_WS.get(key)
    if ws is None and len(_CENTER_WS) >= 16:
        _CENTER_WS.clear()
    if ws is None or ws.numel() < need:
        ws = _CENTER_WS[key] = torch.empty(max(need, 4096), dtype=torch.uint8, device=dev)
    return ws


def check_center_args(K: int, tau, iterations) -> Tuple[float, int]:
    """``(f32(tau), iterations)`` of a centered-clipping round over ``K`` clients, checked: ``tau``
    a number that is finite and > 0 as float32, ``iterations`` an int >= 1, ``1 <= K <= 4096``.
    A bool is refused for both. Nothing here touches the library."""
    if isinstance(tau, (bool, np.bool_)) or not isinstance(tau, (int, float, np.integer, np.floating)):
        raise TypeError(f"tau must be a number, not {type(tau).__name__}")
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)):
        raise TypeError("iterations must be an int")
    with np.errstate(over="ignore"):
        t = float(np.float32(tau))
    if not (np.isfinite(t) and t > 0.0):
        raise ValueError(f"tau must be finite and > 0 (as float32), got {tau}")
    if int(iterations) < 1:
        raise ValueError(f"iterations must be >= 1, got {iterations}")
    K = int(K)
    if K < 1:
        raise ValueError(f"centered clipping needs at least 1 client, got K = {K}")
    if K > CENTER_MAX_CLIENTS:
        raise ValueError(f"centered clipping supports K <= {CENTER_MAX_CLIENTS} clients, got K = {K}")
    return t, int(iterations)


def _check_center_slab(x: torch.Tensor) -> Tuple[int, int]:
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"centered clipping takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    if P < 1:
        raise ValueError("x must have at least one column")
    if P * 4 > _MAX_ROW_BYTES:
        raise ValueError("centered clipping takes rows of up to 1 GiB")
    return K, P


def _check_center_vectors(center: torch.Tensor, out: Optional[torch.Tensor], x: torch.Tensor) -> torch.Tensor:
    """The centre and the output of a dense centered fold over ``x[K, P]``: contiguous float32
    [P]; ``out`` may be ``center`` itself (the same storage from the same address), never a partial
    overlap, and never inside the extent of ``x``, whose rows are read while ``out`` is written."""
    (K, P), dev = x.shape, x.device
    if not isinstance(center, torch.Tensor) or center.dtype != torch.float32:
        raise TypeError("center must be a float32 tensor")
    if center.dim() != 1 or center.numel() != P or not center.is_contiguous():
        raise ValueError(f"center must be a contiguous float32 tensor of {P} elements")
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=dev)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32:
        raise TypeError("out must be a float32 tensor")
    if out.dim() != 1 or out.numel() != P or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 tensor of {P} elements")
    a, b = center.data_ptr(), out.data_ptr()
    if a != b and a < b + 4 * P and b < a + 4 * P:
        raise ValueError("out may be center itself, but must not overlap it in part")
    x0 = x.data_ptr()
    x1 = x0 + 4 * ((K - 1) * (x.stride(0) if K > 1 else P) + P)
    if b < x1 and x0 < b + 4 * P:
        raise ValueError("out must not overlap the deltas x: their rows are read while out is written")
    return out


def _check_center_image(image_dev: torch.Tensor, L: int, K: int, nblk: int) -> Tuple[int, int]:
    if not isinstance(image_dev, torch.Tensor) or image_dev.dtype != torch.int64 or not image_dev.is_contiguous():
        raise TypeError("image_dev must be a contiguous int64 device tensor")
    L, nblk = int(L), int(nblk)
    if L < 1 or nblk < 1 or image_dev.numel() < K * L + 3 * L + 2 * nblk:
        raise ValueError(f"bad plan: L = {L}, nblk = {nblk}, image of {image_dev.numel()} words")
    return L, nblk


def center_l2sq_rows(image_dev: torch.Tensor, R: int, max_n: int, *, rows_per_group: int = 1,
                     take_sqrt: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``fjagg_l2sq_rows`` with a centre per row: ``image_dev`` is the int64 device image ``ptrs[R] |
    n[R] | center_ptrs[R]`` of float32 rows, and ``out[g]`` the float32 sum of ``fl((x - v)^2)``
    over the ``rows_per_group`` rows of group ``g`` in ``fjagg_l2sq_rows``' order (its bits with a
    zero centre), or its correctly rounded root with ``take_sqrt``. The norm pass of centered
    clipping on its own."""
    if not isinstance(image_dev, torch.Tensor) or image_dev.dtype != torch.int64 or not image_dev.is_contiguous():
        raise TypeError("image_dev must be a contiguous int64 device tensor")
    R, max_n, rows_per_group = int(R), int(max_n), int(rows_per_group)
    if R < 1 or rows_per_group < 1 or R % rows_per_group or max_n < 0 or image_dev.numel() < 3 * R:
        raise ValueError(f"bad rows: R = {R}, rows_per_group = {rows_per_group}, image of {image_dev.numel()} words")
    if max_n * 4 > _MAX_ROW_BYTES:
        raise ValueError("centered norms take rows of up to 1 GiB")
    dev = _require_device(image_dev)
    G = R // rows_per_group
    if out is None:
        out = torch.empty(G, dtype=torch.float32, device=dev)
    _f32_vector("out", out, G)
    _require_device(image_dev, out)
    ws = _center_workspace(dev, int(_lib.load().fjagg_l2sq_rows_workspace_bytes(R, max_n)))
    _lib.call("fjagg_l2sq_rows_centered", _lib.F32, image_dev.data_ptr(), R, max_n, rows_per_group, int(bool(take_sqrt)),
              out.data_ptr(), ws.data_ptr(), ws.numel(), _stream_handle(dev))
    return out


def center_fold_dense(x: torch.Tensor, c: torch.Tensor, center: torch.Tensor, *, out: Optional[torch.Tensor] = None,
                      nontemporal: bool = False) -> torch.Tensor:
    """One fold of centered clipping over a float32 slab ``x[K, P]`` with any device factor vector
    ``c`` (float32 [K]): per column, from ``s = +0`` and in client order, ``s = fl(s + t_k)`` with
    ``t_k = fl(c_k * fl(x_k - v))`` for ``c_k > 0`` and ``+0`` otherwise (a NaN, zero or negative
    factor: the client's bits never reach the sum), then ``out = fl(v + fl(s * f32(1/K)))``.
    ``center`` and ``out`` are contiguous float32 [P]; ``out`` may be ``center`` itself, but must
    not overlap ``x`` (``center``, only read, may be a row of it). 16-byte
    units when the slab, the centre and the output allow it, element units otherwise: the same
    bits. ``K <= 4096``; everything is checked before the library is touched."""
    K, P = _check_center_slab(x)
    check_center_args(K, 1.0, 1)
    _f32_vector("c", c, K)
    out = _check_center_vectors(center, out, x)
    dev = _require_device(x, c, center, out)
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjagg_center_fold_dense", _lib.F32, x.data_ptr(), ld, K, P, c.data_ptr(), center.data_ptr(),
              out.data_ptr(), _lib.NONTEMPORAL if nontemporal else 0, _stream_handle(dev))
    return out


def center_fold_ptrs(image_dev: torch.Tensor, L: int, K: int, nblk: int, c: torch.Tensor, *, unaligned: bool = False,
                     nontemporal: bool = False) -> None:
    """:func:`center_fold_dense`'s arithmetic on every leaf of a device plan image in one launch:
    ``in_ptrs[K*L] | out_ptrs[L] | leaf_n[L] | blocks[2*nblk] | center_ptrs[L]``, the blocks of
    :func:`ptrs_plan` for float32 leaves made with the centre pointers counted in the per-leaf
    alignment choice. A leaf's centre may be its output. ``unaligned`` as the plan was made."""
    check_center_args(K, 1.0, 1)
    L, nblk = _check_center_image(image_dev, L, K, nblk)
    _f32_vector("c", c, K)
    dev = _require_device(image_dev, c)
    flags = (_lib.UNALIGNED if unaligned else 0) | (_lib.NONTEMPORAL if nontemporal else 0)
    _lib.call("fjagg_center_fold_ptrs", _lib.F32, image_dev.data_ptr(), L, K, nblk, c.data_ptr(), flags,
              _stream_handle(dev))


def _center_diagnostics(iterations: int, K: int, dev: torch.device):
    return (torch.empty(iterations, K, dtype=torch.float32, device=dev),
            torch.empty(iterations, K, dtype=torch.float32, device=dev))


def centered_clip_dense(x: torch.Tensor, tau, center: torch.Tensor, *, iterations: int = 1,
                        out: Optional[torch.Tensor] = None, leaf_table: Optional[torch.Tensor] = None,
                        max_n: Optional[int] = None, nontemporal: bool = False):
    """A whole round of centered clipping over a float32 slab ``x[K, P]``: ``iterations`` times the
    norm pass around the centre, the clip factors ``c = min(1, f32(tau) / n)`` on the device and
    :func:`center_fold_dense`, the first from ``center`` into ``out`` and the later ones in place
    on ``out`` (``fjagg_center_clip_dense``; ``out`` may be ``center``). Returns ``(out,
    distances, factors)``, the last two float32 ``[iterations, K]``. No host synchronisation and
    nothing uploaded: capturable. ``leaf_table``: an int64 device tensor ``off[L] | n[L]`` of the
    row's leaves (element offsets and sizes, ``max_n`` the largest size), which makes the norms
    add up leaf by leaf as the pytree route's do; default: the row is one leaf."""
    K, P = _check_center_slab(x)
    tau, iterations = check_center_args(K, tau, iterations)
    out = _check_center_vectors(center, out, x)
    dev = _require_device(x, center, out)
    if leaf_table is None:
        L, max_n, tab = 1, P, None
    else:
        if not isinstance(leaf_table, torch.Tensor) or leaf_table.dtype != torch.int64 or leaf_table.dim() != 1 \
                or leaf_table.numel() < 2 or leaf_table.numel() % 2 or not leaf_table.is_contiguous():
            raise TypeError("leaf_table must be a contiguous int64 device tensor off[L] | n[L]")
        _require_device(x, leaf_table)
        L = leaf_table.numel() // 2
        if max_n is None or not 0 <= int(max_n) <= P:
            raise ValueError("a leaf table needs max_n, its largest leaf size, in [0, P]")
        max_n, tab = int(max_n), leaf_table.data_ptr()
    distances, factors = _center_diagnostics(iterations, K, dev)
    ws = _center_workspace(dev, int(_lib.load().fjagg_center_clip_workspace_bytes(K, L, max_n)))
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjagg_center_clip_dense", _lib.F32, x.data_ptr(), ld, K, P, tab, L, max_n, tau, iterations,
              center.data_ptr(), out.data_ptr(), distances.data_ptr(), factors.data_ptr(), ws.data_ptr(), ws.numel(),
              _lib.NONTEMPORAL if nontemporal else 0, _stream_handle(dev))
    return out, distances, factors


def centered_clip_ptrs(image_dev: torch.Tensor, L: int, K: int, nblk: int, max_n: int, tau, *, iterations: int = 1,
                       unaligned: bool = False, nontemporal: bool = False):
    """:func:`centered_clip_dense` over :func:`center_fold_ptrs`' plan image
    (``fjagg_center_clip_ptrs``): the first iteration's centre is ``center_ptrs``, every later
    one's is ``out_ptrs``, in place. ``max_n`` is the largest ``leaf_n``. Returns ``(distances,
    factors)``, float32 ``[iterations, K]``; the result is behind ``out_ptrs``."""
    tau, iterations = check_center_args(K, tau, iterations)
    L, nblk = _check_center_image(image_dev, L, K, nblk)
    max_n = int(max_n)
    if max_n < 0 or max_n * 4 > _MAX_ROW_BYTES:
        raise ValueError("centered clipping takes leaves of up to 1 GiB")
    dev = _require_device(image_dev)
    distances, factors = _center_diagnostics(iterations, K, dev)
    ws = _center_workspace(dev, int(_lib.load().fjagg_center_clip_workspace_bytes(K, L, max_n)))
    flags = (_lib.UNALIGNED if unaligned else 0) | (_lib.NONTEMPORAL if nontemporal else 0)
    _lib.call("fjagg_center_clip_ptrs", _lib.F32, image_dev.data_ptr(), L, K, nblk, max_n, tau, iterations,
              distances.data_ptr(), factors.data_ptr(), ws.data_ptr(), ws.numel(), flags, _stream_handle(dev))
    return distances, factors


FLTRUST_MAX_CLIENTS = 4096  # fjagg_fltrust_*: the client limit (fjagg.h)
_FLTRUST_WS = {}  # (device index, stream handle) -> workspace of an FLTrust round or row pass


def _fltrust_workspace(dev: torch.device, need: int) -> torch.Tensor:
    """The workspace of an FLTrust round on ``dev``'s current stream (the sums, the member tables
    and the block partials), cached like :func:`_center_workspace`; under stream capture a tensor
    of the graph's own pool. Never zeroed, nothing carried between calls."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(need, 4096), dtype=torch.uint8, device=dev)
    key = (dev.index, _stream_handle(dev))
    ws = _FLTRUST_WS.get(key)
    if ws is None and len(_FLTRUST_WS) >= 16:
        _FLTRUST_WS.clear()
    if ws is None or ws.numel() < need:
        ws = _FLTRUST_WS[key] = torch.empty(max(need, 4096), dtype=torch.uint8, device=dev)
    return ws


def check_fltrust_clients(K: int) -> int:
    """``K`` of an FLTrust round, checked: ``1 <= K <= 4096``. Nothing here touches the library."""
    K = int(K)
    if K < 1:
        raise ValueError(f"fltrust needs at least 1 client, got K = {K}")
    if K > FLTRUST_MAX_CLIENTS:
        raise ValueError(f"fltrust supports K <= {FLTRUST_MAX_CLIENTS} clients, got K = {K}")
    return K


def _check_fltrust_slab(x: torch.Tensor) -> Tuple[int, int]:
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"fltrust takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    check_fltrust_clients(K)
    if P < 1:
        raise ValueError("x must have at least one column")
    if P * 4 > _MAX_ROW_BYTES:
        raise ValueError("fltrust takes rows of up to 1 GiB")
    return K, P


def _check_fltrust_vector(name: str, v: torch.Tensor, P: int) -> None:
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float32:
        raise TypeError(f"{name} must be a float32 tensor")
    if v.dim() != 1 or v.numel() != P or not v.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 tensor of {P} elements")


def _fltrust_leaf_table(leaf_table: Optional[torch.Tensor], max_n, P: int):
    """``(L, max_n, table address or None)`` of a dense row's leaf table ``off[L] | n[L]``."""
    if leaf_table is None:
        return 1, P, None
    if not isinstance(leaf_table, torch.Tensor) or leaf_table.dtype != torch.int64 or leaf_table.dim() != 1 \
            or leaf_table.numel() < 2 or leaf_table.numel() % 2 or not leaf_table.is_contiguous():
        raise TypeError("leaf_table must be a contiguous int64 device tensor off[L] | n[L]")
    L = leaf_table.numel() // 2
    if L > 65535:
        raise ValueError(f"fltrust takes up to 65535 leaves, got {L}")
    if max_n is None or isinstance(max_n, (bool, np.bool_)) or not 0 <= int(max_n) <= P:
        raise ValueError("a leaf table needs max_n, its largest leaf size, in [0, P]")
    return L, int(max_n), leaf_table.data_ptr()


def dotsq_rows(image_dev: torch.Tensor, R: int, max_n: int, *, rows_per_group: int = 1):
    """FLTrust's row pass on its own (``fjagg_dotsq_rows``): ``image_dev`` is the int64 device
    image ``ptrs[R] | n[R] | ref_ptrs[R]`` of float32 rows and of the vector each is paired with
    (4-byte alignment is all a row needs). Returns ``(dot, sq)``, float32 ``[R / rows_per_group]``:
    ``sum fl(x * ref)`` and ``sum fl(x^2)`` over a group's rows, ONE read of the rows, both in
    ``fjagg_l2sq_rows``' order (``sq`` has its bits). What a cosine-based rule starts from."""
    if not isinstance(image_dev, torch.Tensor) or image_dev.dtype != torch.int64 or not image_dev.is_contiguous():
        raise TypeError("image_dev must be a contiguous int64 device tensor")
    R, max_n, rows_per_group = int(R), int(max_n), int(rows_per_group)
    if R < 1 or rows_per_group < 1 or R % rows_per_group or max_n < 0 or image_dev.numel() < 3 * R:
        raise ValueError(f"bad rows: R = {R}, rows_per_group = {rows_per_group}, image of {image_dev.numel()} words")
    if max_n * 4 > _MAX_ROW_BYTES:
        raise ValueError("the row pass takes rows of up to 1 GiB")
    dev = _require_device(image_dev)
    G = R // rows_per_group
    both = torch.empty(2, G, dtype=torch.float32, device=dev)
    ws = _fltrust_workspace(dev, int(_lib.load().fjagg_dotsq_rows_workspace_bytes(R, max_n)))
    _lib.call("fjagg_dotsq_rows", _lib.F32, image_dev.data_ptr(), R, max_n, rows_per_group, both[0].data_ptr(),
              both[1].data_ptr(), ws.data_ptr(), ws.numel(), _stream_handle(dev))
    return both[0], both[1]


def dotsq_dense(x: torch.Tensor, ref: torch.Tensor, *, leaf_table: Optional[torch.Tensor] = None,
                max_n: Optional[int] = None, nontemporal: bool = False):
    """:func:`dotsq_rows` over a float32 slab ``x[K, P]`` against ONE shared vector ``ref`` (float32
    ``[P]``, ``fjagg_dotsq_dense``): ``(dot, sq)``, float32 ``[K]``. ``leaf_table`` / ``max_n`` as
    :func:`centered_clip_dense` takes them: the sums then add up leaf by leaf as the pytree route's
    do. The table lives on the device and is TRUSTED (checking it would take a host visit): the caller
    guarantees ``off[l] + n[l] <= P`` and ``n[l] <= max_n``; a wrong entry reads outside the rows.
    ``nontemporal`` streams the deltas past the cache, which keeps ``ref`` in it."""
    K, P = _check_fltrust_slab(x)
    _check_fltrust_vector("ref", ref, P)
    L, max_n, tab = _fltrust_leaf_table(leaf_table, max_n, P)
    dev = _require_device(x, ref) if leaf_table is None else _require_device(x, ref, leaf_table)
    both = torch.empty(2, K, dtype=torch.float32, device=dev)
    ws = _fltrust_workspace(dev, int(_lib.load().fjagg_dotsq_rows_workspace_bytes(K * L, max_n)))
    _lib.call("fjagg_dotsq_dense", _lib.F32, x.data_ptr(), x.stride(0) if K > 1 else P, K, P, tab, L, max_n,
              ref.data_ptr(), both[0].data_ptr(), both[1].data_ptr(), ws.data_ptr(), ws.numel(),
              _lib.NONTEMPORAL if nontemporal else 0, _stream_handle(dev))
    return both[0], both[1]


class FLTrustDiagnostics(NamedTuple):
    """What FLTrust's selection reports, all on the device: ``trust`` / ``cosines`` float64 [K];
    ``factors`` / ``norms`` float32 [K]; ``server_norm`` float32, ``count`` int32 and ``total``
    float64 scalars (see :class:`fedjax_amd.tree_util.FLTrustResult`)."""
    trust: torch.Tensor
    cosines: torch.Tensor
    factors: torch.Tensor
    norms: torch.Tensor
    server_norm: torch.Tensor
    count: torch.Tensor
    total: torch.Tensor


def _fltrust_diagnostics(K: int, dev: torch.device) -> FLTrustDiagnostics:
    d = torch.empty(2 * K + 1, dtype=torch.float64, device=dev)  # trust | cosines | total
    f = torch.empty(2 * K + 1, dtype=torch.float32, device=dev)  # factors | norms | server_norm
    count = torch.empty((), dtype=torch.int32, device=dev)
    return FLTrustDiagnostics(d[:K], d[K:2 * K], f[:K], f[K:2 * K], f[2 * K], count, d[2 * K])


def _fltrust_diag_args(d: FLTrustDiagnostics):
    return (d.cosines.data_ptr(), d.trust.data_ptr(), d.factors.data_ptr(), d.norms.data_ptr(),
            d.server_norm.data_ptr(), d.total.data_ptr(), d.count.data_ptr())


def fltrust_select(dot: torch.Tensor, sq: torch.Tensor, server_sq: torch.Tensor):
    """FLTrust's selection on the device (``fjagg_fltrust_select``; the rule of
    ``fedjax_amd/csrc/fjtrust_dev.h``): from the float32 sums ``dot[K]``, ``sq[K]`` of
    :func:`dotsq_dense` and the server delta's squared norm ``server_sq`` (one float32), the
    cosines, trust scores ``ts = min(max(cos, 0), 1)``, rescale factors ``c = ts |g| / |x_k|`` and
    the member tables of the fold (the clients with ``c > 0`` ascending, ``wperm = c``, ``gscale =
    f32(1 / sum ts)``). Returns ``(diagnostics, tables)``: :class:`FLTrustDiagnostics` and the
    :class:`DeviceGroupTables` of :func:`grouped_sum_dense_device`. One launch of one workgroup, no
    host synchronisation, nothing uploaded: capturable."""
    if not isinstance(dot, torch.Tensor) or dot.dim() != 1:
        raise ValueError("dot must be a float32 [K] device tensor")
    K = check_fltrust_clients(dot.numel())
    _f32_vector("dot", dot, K)
    _f32_vector("sq", sq, K)
    if not isinstance(server_sq, torch.Tensor) or server_sq.dtype != torch.float32 or server_sq.numel() != 1:
        raise ValueError("server_sq must be a float32 device tensor of one element")
    dev = _require_device(dot, sq, server_sq)
    diag = _fltrust_diagnostics(K, dev)
    tables = _select_tables(K, dev)
    _lib.call("fjagg_fltrust_select", dot.data_ptr(), sq.data_ptr(), server_sq.data_ptr(), K, *_fltrust_diag_args(diag),
              tables.order.data_ptr(), tables.seg.data_ptr(), tables.wperm.data_ptr(), tables.gscale.data_ptr(),
              _stream_handle(dev))
    return diag, tables


def fltrust_dense(x: torch.Tensor, server: torch.Tensor, *, out: Optional[torch.Tensor] = None,
                  leaf_table: Optional[torch.Tensor] = None, max_n: Optional[int] = None,
                  nontemporal: bool = False):
    """A whole FLTrust round over a float32 slab ``x[K, P]`` against the server delta ``server``
    (float32 ``[P]``; ``fjagg_fltrust_dense``): the server norm, the row pass, the selection, ``out``
    zeroed, then the grouped fold over the clients the selection trusted — the others are never
    loaded by that second read. Returns ``(out, diagnostics)``; ``out`` (float32 ``[P]``, fresh by
    default) must overlap neither ``x`` nor ``server``. No host synchronisation and nothing uploaded:
    capturable. ``leaf_table`` / ``max_n`` as :func:`dotsq_dense` takes them: the table's entries are
    trusted, not checked (:class:`~fedjax_amd.slab.ClientDeltaSlab` builds its own). ``K <= 4096``;
    every host-side argument is checked before the library is touched."""
    K, P = _check_fltrust_slab(x)
    _check_fltrust_vector("server", server, P)
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=x.device)
    _check_fltrust_vector("out", out, P)
    b, x0 = out.data_ptr(), x.data_ptr()
    if b < server.data_ptr() + 4 * P and server.data_ptr() < b + 4 * P:
        raise ValueError("out must not overlap the server delta")
    if b < x0 + 4 * ((K - 1) * (x.stride(0) if K > 1 else P) + P) and x0 < b + 4 * P:
        raise ValueError("out must not overlap the deltas x: their rows are read while out is written")
    L, max_n, tab = _fltrust_leaf_table(leaf_table, max_n, P)
    dev = _require_device(x, server, out) if leaf_table is None else _require_device(x, server, out, leaf_table)
    diag = _fltrust_diagnostics(K, dev)
    ws = _fltrust_workspace(dev, int(_lib.load().fjagg_fltrust_workspace_bytes(K, L, max_n)))
    _lib.call("fjagg_fltrust_dense", _lib.F32, x.data_ptr(), x.stride(0) if K > 1 else P, K, P, tab, L, max_n,
              server.data_ptr(), out.data_ptr(), *_fltrust_diag_args(diag), ws.data_ptr(), ws.numel(),
              _lib.NONTEMPORAL if nontemporal else 0, _stream_handle(dev))
    return out, diag


def fltrust_ptrs(image_all: torch.Tensor, image_group: torch.Tensor, L: int, K: int, nblk: int, max_n: int, *,
                 unaligned: bool = False, nontemporal: bool = False) -> FLTrustDiagnostics:
    """:func:`fltrust_dense` over pytrees (``fjagg_fltrust_ptrs``): ``image_all`` is ``in_ptrs[K*L] |
    server_ptrs[L] | leaf_n[L]``, ``image_group`` the grouped fold's plan for ``K`` member slots,
    ``in_ptrs[K*L] | out_ptrs[L] | leaf_n[L] | blocks[2*nblk]``, whose slots the round fills on the
    device. ``max_n`` is the largest ``leaf_n``; ``unaligned`` as the plan was made. The result is
    behind ``out_ptrs``; returns the :class:`FLTrustDiagnostics`."""
    for name, t in (("image_all", image_all), ("image_group", image_group)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous int64 device tensor")
    K = check_fltrust_clients(K)
    L, nblk, max_n = int(L), int(nblk), int(max_n)
    if L < 1 or L > 65535 or nblk < 1 or image_all.numel() < K * L + 2 * L \
            or image_group.numel() < K * L + 2 * L + 2 * nblk:
        raise ValueError(f"bad plan: L = {L}, nblk = {nblk}, images of {image_all.numel()} and "
                         f"{image_group.numel()} words")
    if max_n < 0 or max_n * 4 > _MAX_ROW_BYTES:
        raise ValueError("fltrust takes leaves of up to 1 GiB")
    dev = _require_device(image_all, image_group)
    diag = _fltrust_diagnostics(K, dev)
    ws = _fltrust_workspace(dev, int(_lib.load().fjagg_fltrust_workspace_bytes(K, L, max_n)))
    flags = (_lib.UNALIGNED if unaligned else 0) | (_lib.NONTEMPORAL if nontemporal else 0)
    _lib.call("fjagg_fltrust_ptrs", _lib.F32, image_all.data_ptr(), image_group.data_ptr(), L, K, nblk, max_n,
              *_fltrust_diag_args(diag), ws.data_ptr(), ws.numel(), flags, _stream_handle(dev))
    return diag


TOPK_MAX_CLIENTS = _lib.TOPK_MAX_CLIENTS  # fjcomp_topk_*: the clipped fold's client limit (fjcomp.h)
TOPK_CHUNK = _lib.TOPK_CHUNK  # elements of one row a histogram workgroup counts (FJCOMP_TOPK_CHUNK)
TOPK_MAX_PARAMS = (1 << 31) - 1  # P < 2^31: the counts and ranks of the select are 32-bit
_TOPK_WS = {}  # (device index, stream handle) -> workspace of the top-k select (histograms, prefixes, ranks)


def topk_count(k, P: int) -> int:
    """The keep count ``c`` of a top-k sparsifier over rows of ``P`` coordinates, checked: ``k`` is
    an int count ``1 <= k <= P`` taken as is, or a float fraction ``0 < beta <= 1`` giving
    ``c = max(1, floor(beta * P))`` (in double precision). Raises ``TypeError`` for a bool or a
    non-number, ``ValueError`` for ``P < 1``, ``P >= 2^31``, a count outside ``[1, P]`` or a
    fraction outside ``(0, 1]``. Nothing here touches the library."""
    if isinstance(k, (bool, np.bool_)):
        raise TypeError("k must be an int count or a float fraction in (0, 1], not a bool")
    P = int(P)
    if P < 1:
        raise ValueError(f"a top-k sparsifier needs at least 1 coordinate, got P = {P}")
    if P > TOPK_MAX_PARAMS:
        raise ValueError(f"the top-k select supports P < 2^31 coordinates per client, got P = {P}")
    if isinstance(k, (int, np.integer)):
        c = int(k)
        if not 1 <= c <= P:
            raise ValueError(f"a keep count needs 1 <= k <= P = {P}, got k = {c}")
        return c
    if isinstance(k, (float, np.floating)):
        beta = float(k)
        if not (0.0 < beta <= 1.0):
            raise ValueError(f"a keep fraction must be in (0, 1], got {k}")
        return max(1, int(math.floor(beta * P)))
    raise TypeError(f"k must be an int count or a float fraction in (0, 1], not {type(k).__name__}")


def check_topk_clients(K: int) -> int:
    K = int(K)
    if K < 1:
        raise ValueError(f"a top-k sparsified mean needs at least 1 client, got K = {K}")
    if K > TOPK_MAX_CLIENTS:
        raise ValueError(f"the top-k sparsified mean supports K <= {TOPK_MAX_CLIENTS} clients, got K = {K}")
    return K


def _topk_workspace(dev: torch.device, K: int) -> torch.Tensor:
    """The select's workspace on ``dev``'s current stream, cached like :func:`_center_workspace`;
    under stream capture a tensor of the graph's own pool. The entry zeroes it on the stream."""
    need = int(_lib.load().fjcomp_topk_workspace_bytes(K))
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(max(need, 4096), dtype=torch.uint8, device=dev)
    key = (dev.index, _stream_handle(dev))
    ws = _TOPK_WS.get(key)
    if ws is None and len(_TOPK_WS) >= 16:
        _TOPK_WS.clear()
    if ws is None or ws.numel() < need:
        ws = _TOPK_WS[key] = torch.empty(max(need, 4096), dtype=torch.uint8, device=dev)
    return ws


def _check_topk_slab(x: torch.Tensor) -> Tuple[int, int]:
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    if x.dtype != torch.float32:
        raise TypeError(f"the top-k sparsified mean takes float32 deltas, not {x.dtype}")
    K, P = x.shape
    check_topk_clients(K)
    return K, P


def _check_topk_keep(c, P: int) -> int:
    if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)):
        raise TypeError("c must be an int keep count (kernels.topk_count makes one)")
    return topk_count(int(c), P) if P else 0


def _topk_diagnostics(K: int, dev: torch.device, zero: bool = False):
    make = torch.zeros if zero else torch.empty
    return make(K, dtype=torch.float32, device=dev), make(K, dtype=torch.int32, device=dev)


def topk_select_dense(x: torch.Tensor, c: int):
    """``(thresholds, sent)`` of a float32 slab ``x[K, P]``: per client the ``c``-th largest
    magnitude key ``bits & 0x7fffffff`` of its row as a float (float32 [K]) and the count of its
    keys ``>= max(T, 1)`` (int32 [K]); exact (a three-level radix select, ``fjcomp_topk_select_dense``).
    Three passes over the slab and four small launches, no host synchronisation, nothing
    uploaded. ``K <= 4096``, ``P < 2^31``, ``1 <= c <= P``; ``P = 0`` launches nothing and gives
    zeros. Everything is checked before the library is touched."""
    K, P = _check_topk_slab(x)
    c = _check_topk_keep(c, P)
    dev = _require_device(x)
    if P == 0:
        return _topk_diagnostics(K, dev, zero=True)
    thr, sent = _topk_diagnostics(K, dev)
    ws = _topk_workspace(dev, K)
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjcomp_topk_select_dense", _lib.F32, x.data_ptr(), ld, K, P, c, thr.data_ptr(), sent.data_ptr(),
              ws.data_ptr(), ws.numel(), _stream_handle(dev))
    return thr, sent


def topk_mean_dense(x: torch.Tensor, w: torch.Tensor, c: int, *, scale: float, out: Optional[torch.Tensor] = None):
    """``(out, thresholds, sent)``: :func:`topk_select_dense`, then the exact fold of the slab with
    every coordinate below its client's threshold taken as ``+0``: ``s = fl(x~_0 w_0)``,
    ``s = fl(s + fl(x~_k w_k))`` in client order, ``out = fl(s * f32(scale))``, the multiply and the
    add separate (``fjcomp_topk_mean_dense``). All ties at the threshold are kept; a NaN has the
    largest magnitude and is kept first. ``w``: device float32 [K]. No sparsified copy, no host
    synchronisation, nothing uploaded. ``P = 0`` launches nothing."""
    K, P = _check_topk_slab(x)
    c = _check_topk_keep(c, P)
    _f32_vector("w", w, K)
    if out is None:
        out = torch.empty(P, dtype=torch.float32, device=x.device)
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32:
        raise TypeError("out must be a float32 tensor")
    if out.dim() != 1 or out.numel() != P or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 tensor of {P} elements")
    dev = _require_device(x, w, out)
    if P == 0:
        return (out,) + _topk_diagnostics(K, dev, zero=True)
    thr, sent = _topk_diagnostics(K, dev)
    ws = _topk_workspace(dev, K)
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjcomp_topk_mean_dense", _lib.F32, x.data_ptr(), ld, K, P, c, w.data_ptr(), float(np.float32(scale)),
              out.data_ptr(), thr.data_ptr(), sent.data_ptr(), ws.data_ptr(), ws.numel(), _stream_handle(dev))
    return out, thr, sent


class TopKTables:
    """The tables of the pytree route on the host: one int64 image ``in_ptrs[K*L] | out_ptrs[L] |
    leaf_n[L] | chunk_prefix[L+1] | w`` (the float32 weights packed two to a word; ``out_ptrs`` and
    ``w`` may be absent for a select) and what the entries need beside it. A histogram chunk
    never spans two leaves: leaf ``l`` owns ``ceil(leaf_n[l] / TOPK_CHUNK)`` chunks."""

    def __init__(self, in_ptrs: np.ndarray, leaf_n, out_ptrs=None, w=None):
        in_ptrs = np.ascontiguousarray(in_ptrs, dtype=np.int64)
        if in_ptrs.ndim != 2:
            raise ValueError("in_ptrs must be a [K, L] table of leaf pointers")
        self.K, self.L = in_ptrs.shape
        check_topk_clients(self.K)
        leaf_n = np.asarray(leaf_n, dtype=np.int64)
        if leaf_n.shape != (self.L,) or self.L < 1 or (leaf_n < 0).any():
            raise ValueError(f"leaf_n must hold {self.L} sizes >= 0")
        self.P = int(leaf_n.sum())
        prefix = np.concatenate([[0], np.cumsum((leaf_n + TOPK_CHUNK - 1) // TOPK_CHUNK)]).astype(np.int64)
        self.nchunks = int(prefix[-1])
        out_ptrs = np.zeros(self.L, np.int64) if out_ptrs is None else np.asarray(out_ptrs, dtype=np.int64)
        if out_ptrs.shape != (self.L,):
            raise ValueError(f"out_ptrs must hold {self.L} pointers")
        live = leaf_n > 0
        self.unaligned = bool((in_ptrs[:, live] % 16).any() or (out_ptrs[live] % 16).any())
        if w is None:
            words = np.zeros(0, np.int64)
        else:
            w = np.asarray(w, dtype=np.float32)
            if w.shape != (self.K,):
                raise ValueError(f"need {self.K} weights, got {w.size}")
            words = np.zeros((self.K + 1) // 2, dtype=np.int64)
            words.view(np.float32)[: self.K] = w
        self.has_w = w is not None
        self.host = np.concatenate([in_ptrs.ravel(), out_ptrs, leaf_n, prefix, words])

    def upload(self, device: torch.device) -> "TopKTables":
        """The image on ``device`` through the pinned upload (refused under stream capture)."""
        self.image_dev = _lib.upload(torch.from_numpy(self.host), device)
        base, KL, L = self.image_dev.data_ptr(), self.K * self.L, self.L
        self.in_p, self.out_p, self.n_p, self.prefix_p = base, base + 8 * KL, base + 8 * (KL + L), base + 8 * (KL + 2 * L)
        self.w_p = base + 8 * (KL + 3 * L + 1)
        return self


def _topk_ptrs_args(tables: TopKTables, c: int):
    if not isinstance(tables, TopKTables) or not hasattr(tables, "image_dev"):
        raise TypeError("tables must be uploaded TopKTables")
    c = _check_topk_keep(c, tables.P)
    return c, _require_device(tables.image_dev)


def topk_select_ptrs(tables: TopKTables, c: int):
    """:func:`topk_select_dense` over uploaded :class:`TopKTables`: client ``k``'s row is its ``L``
    leaves back to back, and ONE histogram per client spans all of them (a global top-k, not a
    per-leaf one). ``fjcomp_topk_select_ptrs``."""
    c, dev = _topk_ptrs_args(tables, c)
    if tables.P == 0:
        return _topk_diagnostics(tables.K, dev, zero=True)
    thr, sent = _topk_diagnostics(tables.K, dev)
    ws = _topk_workspace(dev, tables.K)
    _lib.call("fjcomp_topk_select_ptrs", _lib.F32, tables.in_p, tables.K, tables.L, tables.n_p, tables.prefix_p,
              tables.nchunks, tables.P, c, thr.data_ptr(), sent.data_ptr(), ws.data_ptr(), ws.numel(),
              _lib.UNALIGNED if tables.unaligned else 0, _stream_handle(dev))
    return thr, sent


def topk_mean_ptrs(tables: TopKTables, c: int, *, scale: float):
    """:func:`topk_mean_dense`'s arithmetic over uploaded :class:`TopKTables` made with output
    pointers and weights: the result goes behind ``out_ptrs``; returns ``(thresholds, sent)``.
    ``fjcomp_topk_mean_ptrs``."""
    c, dev = _topk_ptrs_args(tables, c)
    if not tables.has_w:
        raise ValueError("topk_mean_ptrs needs tables made with weights and output pointers")
    if tables.P == 0:
        return _topk_diagnostics(tables.K, dev, zero=True)
    thr, sent = _topk_diagnostics(tables.K, dev)
    ws = _topk_workspace(dev, tables.K)
    _lib.call("fjcomp_topk_mean_ptrs", _lib.F32, tables.in_p, tables.K, tables.L, tables.n_p, tables.prefix_p,
              tables.nchunks, tables.P, c, tables.w_p, float(np.float32(scale)), tables.out_p, thr.data_ptr(),
              sent.data_ptr(), ws.data_ptr(), ws.numel(), _lib.UNALIGNED if tables.unaligned else 0,
              _stream_handle(dev))
    return thr, sent


def fill_synth(x: torch.Tensor, *, k0: int = 0, seed: int = 0, amp: float = 0.01) -> torch.Tensor:
    """Synthetic deltas x[k, p] = amp * u(seed, k0 + k, p) (tests/bench only)."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be a [K, P] tensor with unit column stride")
    dev = _require_device(x)
    K, P = x.shape
    ld = x.stride(0) if K > 1 else P
    _lib.call("fjagg_fill_synth", dtype_code(x.dtype), x.data_ptr(), ld, K, P, k0, seed, amp,
              _stream_handle(dev))
    return x
