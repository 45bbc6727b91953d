"""JAX-compatible PRNG keys and draws for the compression aggregators.

FedJAX's compression aggregators draw from ``jax.random`` (threefry2x32, with
``jax_threefry_partitionable`` off as in ``compression_test.py:22``) and iterate
client keys with ``haiku.PRNGSequence`` (``compression.py:195-197``). Keys here are
plain ``numpy.uint32[2]`` arrays with the same bits as a raw ``jax.random.PRNGKey``
(``np.asarray(jax_key)`` converts one), so a round seeded here draws exactly what the
reference would draw:

* key algebra (``PRNGKey``, ``split``, ``PRNGSequence``) runs on the host in the C++
  of ``libfjagg.so`` (``fjcomp_random_split`` / ``fjcomp_prng_sequence``): a few
  threefry blocks per client, sequential by nature;
* the per-element draws (``random_bits``, ``uniform``, ``rademacher``, ``normal``) are HIP
  kernels writing device tensors (``fjcomp_random_bits`` / ``fjcomp_uniform`` /
  ``fjcomp_normal``).
"""

from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from fedjax_amd import _lib

Key = np.ndarray  # uint32[2]
Shape = Union[int, Sequence[int]]


def _key(key) -> np.ndarray:
    k = np.ascontiguousarray(np.asarray(key, dtype=np.uint32).reshape(-1))
    if k.shape != (2,):
        raise ValueError(f"a PRNG key is two uint32 words, got shape {np.shape(key)}")
    return k


def strict_key(key) -> np.ndarray:
    """``key`` as uint32[2], refusing what is not two uint32 words: another dtype than an
    integer one, another shape, a word outside [0, 2^32). (The differentially private calls
    use this: a key silently wrapped or truncated would still draw noise, from the wrong stream.)"""
    a = np.asarray(key)
    if a.dtype.kind not in "iu":
        raise TypeError(f"a PRNG key is two uint32 words, got dtype {a.dtype}")
    if a.shape != (2,):
        raise ValueError(f"a PRNG key is two uint32 words, got shape {a.shape}")
    if a.dtype != np.uint32 and ((a < 0).any() or (a > 0xFFFFFFFF).any()):
        raise ValueError("a PRNG key is two uint32 words, got a word outside [0, 2^32)")
    return np.ascontiguousarray(a.astype(np.uint32))


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def PRNGKey(seed: int) -> np.ndarray:  # noqa: N802 (jax.random.PRNGKey)
    """``jax.random.PRNGKey(seed)``: ``[seed >> 32, seed & 0xffffffff]`` (uint32)."""
    seed = int(seed)
    return np.array([(seed >> 32) & 0xFFFFFFFF, seed & 0xFFFFFFFF], dtype=np.uint32)


def split(key, num: int = 2) -> np.ndarray:
    """``jax.random.split(key, num)`` -> uint32 [num, 2]."""
    return split_many(_key(key)[None], num)[0]


def split_many(keys, num: int) -> np.ndarray:
    """Split each of ``keys`` [n, 2] into ``num`` keys -> uint32 [n, num, 2]."""
    keys = np.ascontiguousarray(np.asarray(keys, dtype=np.uint32).reshape(-1, 2))
    out = np.empty((keys.shape[0], int(num), 2), dtype=np.uint32)
    _lib.call("fjcomp_random_split", _ptr(keys), keys.shape[0], int(num), _ptr(out))
    return out


class PRNGSequence:
    """``haiku.PRNGSequence`` over a key: each ``next`` reserves one subkey
    (``key, sub = split(key)``). ``take(n)`` draws n subkeys in one host call."""

    def __init__(self, key_or_seed):
        if isinstance(key_or_seed, (int, np.integer)):
            key_or_seed = PRNGKey(int(key_or_seed))
        self._key = _key(key_or_seed).copy()

    def __iter__(self):
        return self

    def __next__(self) -> np.ndarray:
        return self.take(1)[0]

    def take(self, n: int) -> np.ndarray:
        out = np.empty((int(n), 2), dtype=np.uint32)
        _lib.call("fjcomp_prng_sequence", _ptr(self._key), int(n), _ptr(out))
        return out

    @property
    def internal_state(self) -> np.ndarray:
        return self._key.copy()


def _size(shape: Shape) -> Tuple[Tuple[int, ...], int]:
    shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
    n = int(np.prod(shape)) if shape else 1
    if n >= 1 << 32:
        raise ValueError("draws of 2^32 or more elements use a different counter layout in jax; not supported")
    return shape, n


def _device(device) -> torch.device:
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.FjaggError("fedjax_amd draws on a ROCm GPU; torch.cuda.is_available() is False")
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def random_bits(key, shape: Shape = (), device=None) -> torch.Tensor:
    """``jax.random.bits(key, shape, uint32)``, as an int32 tensor holding the bits."""
    k = _key(key)
    shape, n = _size(shape)
    dev = _device(device)
    out = torch.empty(shape, dtype=torch.int32, device=dev)
    _lib.call("fjcomp_random_bits", int(k[0]), int(k[1]), n, out.data_ptr(),
              torch.cuda.current_stream(dev).cuda_stream)
    return out


def uniform(key, shape: Shape = (), device=None) -> torch.Tensor:
    """``jax.random.uniform(key, shape)`` (float32 in [0, 1))."""
    k = _key(key)
    shape, n = _size(shape)
    dev = _device(device)
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    _lib.call("fjcomp_uniform", int(k[0]), int(k[1]), n, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return out


def normal(key, shape: Shape = (), device=None) -> torch.Tensor:
    """``jax.random.normal(key, shape)`` (float32): jax's bits and its uniform on (-1, 1),
    then ``sqrt(2) * erfinv(u)`` evaluated in float64 and rounded once to float32
    (``fjcomp_normal``; XLA's own float32 ``erf_inv`` polynomial is not reproduced, so the
    last step may differ from a JAX run in the last place). Every value is finite."""
    k = _key(key)
    shape, n = _size(shape)
    dev = _device(device)
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    _lib.call("fjcomp_normal", _ptr(k), n, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return out


def normal_from_bits(bits: torch.Tensor) -> torch.Tensor:
    """The bits -> value map of :func:`normal` alone (``fjcomp_normal_from_bits``):
    ``normal(key, shape)`` is ``normal_from_bits(random_bits(key, shape))``. ``bits``: a
    contiguous int32 device tensor holding the 32-bit words, as :func:`random_bits` returns."""
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.int32 or not bits.is_contiguous():
        raise TypeError("bits must be a contiguous int32 tensor (the words of random_bits)")
    if not bits.is_cuda:
        raise ValueError("bits must be a device tensor")
    _size(tuple(bits.shape))
    out = torch.empty(bits.shape, dtype=torch.float32, device=bits.device)
    _lib.call("fjcomp_normal_from_bits", bits.data_ptr(), bits.numel(), out.data_ptr(),
              torch.cuda.current_stream(bits.device).cuda_stream)
    return out


def rademacher(key, shape: Shape = (), device=None) -> torch.Tensor:
    """``jax.random.rademacher(key, shape)``: int32 +-1 (+1 where uniform < 0.5)."""
    u = uniform(key, shape, device)
    return torch.where(u < 0.5, 1, -1).to(torch.int32)


def permutation(key, n: int, device=None) -> torch.Tensor:
    """A permutation of ``range(n)`` as an int32 device tensor: the stable argsort (ties to the
    lower index) of the ``n`` words ``random_bits(key, (n,))`` compared as unsigned 32-bit
    integers. This is this project's own rule, fixed here so that a shuffle can be reproduced from
    its key; it is NOT ``jax.random.permutation``'s bits. The draw and the sort both run on the
    device, in stream order, with no host step: the table a bucketed aggregate takes as ``perm``."""
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)):
        raise TypeError(f"n must be an int >= 1, not {type(n).__name__}")
    if n < 1:
        raise ValueError(f"a permutation needs n >= 1, got {n}")
    words = random_bits(key, (int(n),), device).to(torch.int64) & 0xFFFFFFFF
    return torch.sort(words, stable=True).indices.to(torch.int32)


__all__ = ["PRNGKey", "PRNGSequence", "normal", "normal_from_bits", "permutation", "rademacher", "random_bits", "split",
           "split_many", "strict_key", "uniform"]
