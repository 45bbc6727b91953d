"""TEST INFRASTRUCTURE ONLY — numpy / torch-CPU restatement of ``jax.random.normal`` (float32)
as ``fedjax_amd.random.normal`` defines it (include/fjcomp.h, fjcomp_normal):

* bits   ``oracle.jax_random_ref.random_bits`` (threefry_2x32 over iota(n), JAX's counter layout)
* u      ``f = bitcast((bits >> 9) | 0x3f800000) - 1``; ``lo = nextafter(-1f, 0f)``;
         ``u = max(lo, fl(fl(f * fl(1f - lo)) + lo))`` — jax.random.uniform(minval=lo, maxval=1)
* z      ``sqrt(2) * erfinv(u)`` in float64 (torch's CPU erfinv), rounded once to float32

The product's map runs on the device (fjrand_dev.h) with the device's float64 erfinv; the two
float64 values differ in their last places at most, so the float32 results differ only where
that flips a rounding: by one float32 ulp at most.
"""
import numpy as np
import torch

from oracle import jax_random_ref as jr

LO = np.nextafter(np.float32(-1.0), np.float32(0.0))
SPAN = np.float32(np.float32(1.0) - LO)  # fl(1 - lo): exactly 2


def uniform_from_bits(bits: np.ndarray) -> np.ndarray:
    """float32 u in [lo, 1) from uint32 words."""
    bits = np.asarray(bits, np.uint32)
    f = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    return np.maximum(LO, (f * SPAN).astype(np.float32) + LO).astype(np.float32)


def normal_from_bits(bits: np.ndarray) -> np.ndarray:
    """float32 z from uint32 words (any shape)."""
    u = torch.from_numpy(uniform_from_bits(bits).astype(np.float64))
    z = np.sqrt(2.0) * torch.special.erfinv(u)
    return z.to(torch.float32).numpy()


def normal(key, shape) -> np.ndarray:
    """jax.random.normal(key, shape, float32) as restated above."""
    shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
    n = int(np.prod(shape)) if shape else 1
    return normal_from_bits(jr.random_bits(np.asarray(key, np.uint32), n)).reshape(shape)


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in float32 ulps between finite arrays (ordered-integer view)."""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-0x80000000) - i, i)
    return np.abs(ordered(a) - ordered(b))
