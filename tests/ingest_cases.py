"""Host-conversion cases shared by tests/test_ingest.py (CPU, ``_host_view``) and
tests/test_gpu_ingest.py (the same leaves through ``DeltaIngestor.put``): an independent
float32 -> bfloat16 reference, a matrix of leaf containers and values, and the bytes a slab
row must hold for each. Nothing here calls the code under test."""
import numpy as np
import torch

from fedjax_amd.ingest import BF16Array


def ref_bf16_bits(u32):
    """bfloat16 bits of float32 bit patterns, without the add-and-shift trick of the code
    under test: for a finite value take its two neighbouring bfloat16 values (the one towards
    zero and the next one away from it, +-2^128 where that overflows), compare the distances
    in float64 (exact: the three values share a binade or two) and take the nearer, the even
    mantissa on a tie; 2^128 becomes the infinity. An infinity stays. A NaN keeps its sign
    and upper payload and gets the quiet bit: the device's rule (``f32_to_bf16``)."""
    u32 = np.asarray(u32, np.uint32)
    hi = (u32 >> np.uint32(16)).astype(np.uint32)
    mag = u32 & np.uint32(0x7FFFFFFF)
    finite = mag < np.uint32(0x7F800000)
    lo_hi = hi & np.uint32(0x7FFF)
    up_hi = lo_hi + np.uint32(1)
    with np.errstate(invalid="ignore"):  # (signalling NaNs among the patterns; masked out below)
        x = np.abs(u32.view(np.float32).astype(np.float64))
        lo_v = (lo_hi << np.uint32(16)).view(np.float32).astype(np.float64)
        up_v = np.where(up_hi == np.uint32(0x7F80), 2.0 ** 128,
                        (np.minimum(up_hi, np.uint32(0x7F80)) << np.uint32(16)).view(np.float32).astype(np.float64))
        d_lo, d_up = x - lo_v, up_v - x
    take_up = (d_up < d_lo) | ((d_up == d_lo) & ((lo_hi & np.uint32(1)) == 1))
    rounded = np.where(take_up, up_hi, lo_hi) | (hi & np.uint32(0x8000))
    nan = mag > np.uint32(0x7F800000)
    return np.where(finite, rounded, np.where(nan, hi | np.uint32(0x40), hi)).astype(np.uint16)


def widen(bits_u16):
    return (np.asarray(bits_u16, np.uint32) << np.uint32(16)).view(np.float32)


# float32 bit patterns, 24 of them (a 4 x 6 leaf): +-0, subnormals, the smallest normal, +-inf,
# NaNs of both signs with payloads (quiet and signalling), +-3.4e38, the largest finite value,
# the values around the overflow tie (0x7F7F8000 rounds to +inf), ties to even both ways
F32_BITS = np.array([
    0x00000000, 0x80000000, 0x3F800000, 0xBFC00000, 0x00000001, 0x807FFFFF,
    0x00800000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001,
    0xFFFFFFFF, 0x7FA12345, 0xFF812345, 0x7F7FC99E, 0xFF7FC99E, 0x7F7FFFFF,
    0x7F7F7FFF, 0x7F7F8000, 0x3F808000, 0x3F818000, 0x3F808001, 0x00008000], np.uint32)
# float64 values that float32 cannot hold: beyond its range, below its subnormals, the ties at
# the bottom of its range, NaNs whose payload sits in the low bits only
F64_BITS = np.array([
    0x4810000000000000, 0xFE37E43C8800759C, 0x3590000000000000, 0x3680000000000000,
    0x3688000000000000, 0xB690000000000001, 0x7FF0000000000001, 0xFFF8000000000001,
    0x47EFFFFFF0000000, 0x47EFFFFFEFFFFFFF, 0x3FF0000010000000, 0x3FF0000010000001], np.uint64)
F16_BITS = np.array([0x0000, 0x8000, 0x3C00, 0x0001, 0x83FF, 0x7C00, 0xFC00, 0x7E01, 0xFE00, 0x7D55, 0x7BFF, 0xFBFF],
                    np.uint16)
BF16_BITS = np.array([
    0x0000, 0x8000, 0x3F80, 0xBFC0, 0x0001, 0x807F, 0x0080, 0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7F81,
    0xFFFF, 0x7FA1, 0xFF81, 0x7F7F, 0xFF7F, 0x3F81, 0x0040, 0x4049, 0xC2F7, 0x7F00, 0x0100, 0x8001], np.uint16)
I32 = np.array([0, 1, -1, 16777216, 16777217, 16777219, -16777217, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 65, 123456789, -7],
               np.int32)


def _bf16_tensor(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


def leaf_cases():
    """name -> leaf. Names sort in the order the cases are listed (jax's dict order is sorted)."""
    f32 = F32_BITS.view(np.float32).reshape(4, 6).copy()
    with np.errstate(invalid="ignore"):
        f64 = np.concatenate([f32.ravel().astype(np.float64), F64_BITS.view(np.float64)]).reshape(6, 6)
    f16 = F16_BITS.view(np.float16).reshape(3, 4).copy()
    bf = BF16_BITS.reshape(4, 6).copy()
    i32 = I32.reshape(2, 6).copy()
    boolean = (np.arange(10) % 3 == 0).reshape(2, 5)
    cases = [
        ("np_f16", f16), ("np_f32", f32), ("np_f64", f64), ("np_i32", i32), ("np_bool", boolean),
        ("np_0d_f32", np.array(F32_BITS[14:15].view(np.float32)[0])), ("np_0d_f64", np.array(1e39)),
        ("np_0d_bool", np.array(True)),
        ("scalar_f16", np.float16(-1.5)), ("scalar_f32", F32_BITS[13:14].view(np.float32)[0]),
        ("scalar_f64", np.float64(-1e300)), ("scalar_i32", np.int32(16777217)), ("scalar_bool", np.bool_(True)),
        ("bf16", BF16Array(bf)), ("bf16_0d", BF16Array(np.array(0xFFC1, np.uint16))),
        ("torch_f32", torch.from_numpy(f32.copy())), ("torch_f64", torch.from_numpy(f64.copy())),
        ("torch_bf16", _bf16_tensor(bf)), ("torch_0d_f32", torch.from_numpy(f32.copy())[2, 3]),
        ("torch_f16", torch.from_numpy(f16.copy())), ("torch_i32", torch.from_numpy(i32.copy())),
        ("view_t_np_f32", f32.T), ("view_t_np_f64", f64.T), ("view_t_bf16", BF16Array(bf).T),
        ("view_t_torch_f32", torch.from_numpy(f32.copy()).t()), ("view_t_torch_bf16", _bf16_tensor(bf).t()),
        ("view_s_np_f32", f32[::2]), ("view_s_np_f64", f64[:, ::2]), ("view_s_bf16", BF16Array(bf)[::2, 1::2]),
        ("view_s_torch_f32", torch.from_numpy(f32.copy())[::2]), ("view_s_torch_bf16", _bf16_tensor(bf)[:, ::2]),
        ("view_f_np_f32", np.asfortranarray(f32)), ("view_f_np_f64", np.asfortranarray(f64)),
        ("view_f_bf16", BF16Array(np.asfortranarray(bf))),
        ("zero_np_f32", np.zeros((0,), np.float32)), ("zero_np_f64", np.zeros((0, 3), np.float64)),
        ("zero_bf16", BF16Array(np.zeros((3, 0), np.uint16))), ("zero_torch_f32", torch.zeros(0)),
        ("zero_torch_bf16", torch.zeros((2, 0), dtype=torch.bfloat16)),
        ("np_f32_single", np.array([-3.0], np.float32)),  # 513 elements in all: a padded row
    ]
    # a numbered prefix keeps dict (sorted-key) order equal to list order
    return {f"{j:02d}_{name}": leaf for j, (name, leaf) in enumerate(cases)}


def _is_bf16(leaf):
    return isinstance(leaf, BF16Array) or (isinstance(leaf, torch.Tensor) and leaf.dtype == torch.bfloat16)


def _bf16_bits_of(leaf):
    if isinstance(leaf, torch.Tensor):
        return leaf.contiguous().view(torch.int16).numpy().view(np.uint16).ravel(order="C")
    return np.asarray(leaf, np.uint16).ravel(order="C")


def ref_f32(leaf):
    """Flat float32 values a float32 slab row holds for ``leaf`` (C order): numpy's
    round-to-nearest cast, bfloat16 widened by 16 bits."""
    if _is_bf16(leaf):
        return widen(_bf16_bits_of(leaf))
    a = leaf.numpy() if isinstance(leaf, torch.Tensor) else np.asarray(leaf)
    with np.errstate(over="ignore", invalid="ignore"):
        return a.astype(np.float32).ravel(order="C")


def ref_bf16(leaf):
    """Flat bfloat16 bits a bfloat16 slab row holds for ``leaf``: bfloat16 leaves verbatim,
    everything else through float32 and :func:`ref_bf16_bits`."""
    if _is_bf16(leaf):
        return _bf16_bits_of(leaf).copy()
    return ref_bf16_bits(ref_f32(leaf).view(np.uint32))


def expected_bytes(leaf, slab_dtype):
    ref = ref_f32(leaf) if slab_dtype == torch.float32 else ref_bf16(leaf)
    return np.ascontiguousarray(ref).view(np.uint8).reshape(-1)


def template_of(cases):
    """A slab template with the cases' structure and leaf shapes."""
    return {k: np.zeros(tuple(v.shape), np.float32) for k, v in cases.items()}
