"""Compression aggregators on the GPU (``fedjax/aggregators/compression.py``).

Same names, arguments, state and randomness as the reference: a round seeded with
``fedjax_amd.random.PRNGKey(s)`` (bit-identical to ``jax.random.PRNGKey(s)``) draws
exactly the reference's jax.random stream, client keys come from a
haiku.PRNGSequence-equivalent, per-leaf keys from ``split(client_key, num_leaves)``.

Where the reference runs, per client and per leaf, a jitted quantizer and then
tree_mean's fold, a round here is a few kernel launches over every client and leaf
at once (fedjax_amd/_compress.py, include/fjcomp.h):

* uniform / terngrad: one statistics pass, then ONE kernel that draws the uniform
  bits, quantizes and folds the clients in order (the quantized deltas never reach
  HBM); the fold is tree_mean's (``fl(q * w_k)`` summed in client order, then
  ``* f32(1/W)``), bitwise;
* rotated uniform: the rotation key is shared by all clients (compression.py:241),
  so the mean is taken in the rotated domain and inverted once;
* DRIVE: per-client rotation, per-client scale, inverse rotation, dense fold.

``num_bits`` follows the reference's float32 arithmetic (``tree_size`` is an int32
there), so ``num_bits`` compares equal to the reference's values.

Leaves must be float32 (int32 leaves are converted exactly below 2^24; bfloat16
raises TypeError). Numerics: DESIGN.md §4.
"""

from __future__ import annotations

import itertools
import math
from dataclasses import field as _field
from typing import Any, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from fedjax_amd import _compress as C
from fedjax_amd import _lib, dataclasses, kernels, pytree, random, tree_util
from fedjax_amd.aggregators import aggregator

PyTree = Any
F32 = np.float32


@dataclasses.dataclass
class CompressionState:
    """compression.py:32-40: bits transmitted so far and the aggregator's key."""
    num_bits: Any
    rng: Any


# ----------------------------------------------------------------------------- helpers
def _f32_leaf(x, device) -> torch.Tensor:
    t = tree_util._device_leaf(x, device)
    if t.dtype == torch.float32:
        return t
    if t.dtype == torch.bfloat16:
        raise TypeError("bfloat16 leaves are not supported by the compression kernels (float32 only)")
    return t.to(torch.float32)


def _rows(trees: Sequence[PyTree]):
    """Client leaves as float32 device tensors; _client_rows has already checked every
    client against client 0's structure, shapes and dtypes (the kernels size every row
    from client 0), so only client 0's dtypes need looking at."""
    td, rows = tree_util._client_table(trees)
    if rows[0] and not all(x.dtype == torch.float32 for x in rows[0]):
        td, rows = tree_util._client_rows(trees)
        device = rows[0][0].device
        rows = [[_f32_leaf(x, device) for x in r] for r in rows]
    return td, rows


def _weights(weights: Sequence[Any]) -> Tuple[np.ndarray, Optional[float]]:
    """f32(w_k) and tree_mean's f32(1/W) (tree_util.py:85-96)."""
    sum_weight = 0.0
    hw = []
    for w in weights:
        w = tree_util._host_weight(w)
        tree_util._weight_kind(w)
        hw.append(w)
        sum_weight += w
    return np.array([np.float32(w) for w in hw], dtype=np.float32), float(np.float32(tree_util._inverse(sum_weight)))


def _single(v, method: int, rng, *, num_levels: int = 2, v_min=None, v_max=None) -> torch.Tensor:
    """One leaf quantized with one key (K = 1, weight 1, no scale: q * 1 is exact)."""
    device = tree_util._find_device([v])
    t = _f32_leaf(v, device)
    out = torch.empty(t.shape, dtype=torch.float32, device=device)
    if t.numel() == 0:
        raise ValueError("cannot quantize an empty array (the reference fails on amin of an empty array)")
    keys = np.asarray(rng, np.uint32).reshape(1, 1, 2)
    qp = None
    if v_min is not None or v_max is not None:
        if v_min is None or v_max is None:
            stats, _ = C.row_stats([(t.data_ptr(), t.numel())], method, device, want_qparams=False)
            s = np.frombuffer(stats.cpu().numpy().tobytes(), dtype=C.STATS)[0]
            v_min = s["min"] if v_min is None else v_min
            v_max = s["max"] if v_max is None else v_max
        host = C.qparams_host(v_min, v_max)
        qp = torch.from_numpy(host.view(np.uint8).copy()).to(device)
    C.quantized_mean(method, [[t]], keys, np.ones(1, np.float32), None, [out], num_levels=num_levels, qparams=qp)
    return out


# ----------------------------------------------------------------------------- quantizers
def binary_stochastic_quantize(v, rng, v_min: Optional[float] = None, v_max: Optional[float] = None) -> torch.Tensor:
    """compression.py:43-63."""
    return _single(v, _lib.COMP_BINARY, rng, v_min=v_min, v_max=v_max)


def uniform_stochastic_quantize(v, num_levels: int, rng, v_min: Optional[float] = None,
                                v_max: Optional[float] = None) -> torch.Tensor:
    """compression.py:66-97."""
    return _single(v, _lib.COMP_UNIFORM, rng, num_levels=int(num_levels), v_min=v_min, v_max=v_max)


def terngrad_quantize(v, rng) -> torch.Tensor:
    """compression.py:323-336."""
    return _single(v, _lib.COMP_TERNGRAD, rng)


def _quantize_pytree(params: PyTree, rng, method: int, num_levels: int = 2) -> PyTree:
    td, rows = _rows([params])
    if not rows[0]:
        return params
    L = len(rows[0])
    keys = random.split(rng, L).reshape(1, L, 2)
    outs = [torch.empty(x.shape, dtype=torch.float32, device=x.device) for x in rows[0]]
    C.quantized_mean(method, rows, keys, np.ones(1, np.float32), None, outs, num_levels=num_levels)
    return pytree.unflatten(td, outs)


def uniform_stochastic_quantize_pytree(params: PyTree, num_levels: int, rng) -> PyTree:
    """compression.py:100-118 (leaf keys = split(rng, num_leaves))."""
    return _quantize_pytree(params, rng, _lib.COMP_UNIFORM, int(num_levels))


def terngrad_quantize_pytree(params: PyTree, rng) -> PyTree:
    """compression.py:339-353."""
    return _quantize_pytree(params, rng, _lib.COMP_TERNGRAD)


def num_leaves(pytree_: PyTree) -> int:
    """compression.py:121-122."""
    return len(pytree.leaves_of(pytree_))


def arithmetic_encoding_num_bits(v) -> np.float32:
    """compression.py:143-149: bits to store v with arithmetic coding."""
    device = tree_util._find_device([v])
    t = _f32_leaf(v, device).reshape(-1)
    t = torch.nan_to_num(t, nan=0.0, posinf=float(np.finfo(np.float32).max), neginf=-float(np.finfo(np.float32).max))
    _, counts = torch.unique(t, sorted=True, return_counts=True)
    return C.arithmetic_bits_from_counts(counts.cpu().numpy(), t.numel())


def drive_pytree(params: PyTree) -> PyTree:
    """compression.py:269-277: every leaf becomes sum(y^2) * sign(y) / sum(|y|)."""
    leaves, td = pytree.flatten(params)
    if not leaves:
        return params
    device = tree_util._find_device(leaves)
    ts = [_f32_leaf(x, device) for x in leaves]
    stats, _ = C.row_stats([(t.data_ptr(), t.numel()) for t in ts], 0, device, want_qparams=False)
    s = np.frombuffer(stats.cpu().numpy().tobytes(), dtype=C.STATS)
    out = []
    for t, st in zip(ts, s):
        a, b = float(np.float32(st["sumsq"])), float(np.float32(st["sumabs"]))
        sign = torch.where(t > 0, 1.0, torch.where(t < 0, -1.0, t))
        out.append((a * sign) / b)
    return pytree.unflatten(td, out)


# ----------------------------------------------------------------------------- bits
def _bits_per_param(per_param: float, P: int, L: int) -> np.float32:
    """``per_param * tree_size + 32 * 2 * num_leaves`` with tree_size an int32 array."""
    return F32(F32(F32(per_param) * F32(P)) + F32(32 * 2 * L))


def _consume(clients: Iterable) -> Tuple[list, list]:
    trees, weights = [], []
    for _, params, weight in clients:  # client ids are ignored (aggregator.py:69)
        trees.append(params)
        weights.append(weight)
    return trees, weights


def _mean_round(trees, weights, client_keys, method, num_levels=2, hist=False):
    """tree_mean over the quantized client deltas, one fused launch."""
    td, rows = _rows(trees)
    if not rows[0]:
        return pytree.unflatten(td, []), td, rows, None
    K, L = len(rows), len(rows[0])
    leaf_keys = random.split_many(client_keys, L)
    w, scale = _weights(weights)
    outs = [torch.empty(x.shape, dtype=torch.float32, device=x.device) for x in rows[0]]
    h, qp = C.quantized_mean(method, rows, leaf_keys, w, scale, outs, num_levels=num_levels, hist=hist)
    bits = C.arithmetic_bits(h, qp, K, [x.numel() for x in rows[0]], num_levels) if hist else None
    return pytree.unflatten(td, outs), td, rows, bits


# ----------------------------------------------------------------------------- aggregators
def uniform_stochastic_quantizer(num_levels: int, rng, encode_algorithm: Optional[str] = None) -> aggregator.Aggregator:
    """compression.py:152-221."""

    def init():
        return CompressionState(0.0, np.asarray(rng, np.uint32))

    def apply(clients_params_and_weights, aggregator_state):
        if encode_algorithm is not None:
            assert encode_algorithm == "arithmetic"
        new_rng, use_rng = random.split(aggregator_state.rng)
        trees, weights = _consume(clients_params_and_weights)
        client_keys = random.PRNGSequence(use_rng).take(len(trees))
        arith = encode_algorithm == "arithmetic"
        if not trees:
            agg, P, L, bits = None, 0, 0, []
        else:
            agg, _, rows, bits = _mean_round(trees, weights, client_keys, _lib.COMP_UNIFORM, int(num_levels), arith)
            P, L = sum(x.numel() for x in rows[0]), len(rows[0])
        if arith:
            new_bits = F32(F32(sum(bits)) / F32(len(bits))) if bits else 0.0
        else:
            new_bits = _bits_per_param(math.log2(num_levels), P, L)
        return agg, CompressionState(F32(aggregator_state.num_bits + new_bits), new_rng)

    return aggregator.Aggregator(init, apply)


def rotated_uniform_stochastic_quantizer(num_levels: int, rng, *,
                                         workspace_bytes: int = C.DEFAULT_WORKSPACE_BYTES) -> aggregator.Aggregator:
    """compression.py:224-266. ``workspace_bytes`` bounds the rotated-delta batch
    kept in HBM (a build-side knob; the reference holds one client at a time)."""

    def init():
        return CompressionState(0.0, np.asarray(rng, np.uint32))

    def apply(clients_params_and_weights, aggregator_state):
        new_rng, rotation_rng = random.split(aggregator_state.rng)
        new_rng, use_rng = random.split(new_rng)
        trees, weights = _consume(clients_params_and_weights)
        client_keys = random.PRNGSequence(use_rng).take(len(trees))
        agg, P, L = None, 0, 0
        if trees:
            td, rows = _rows(trees)
            L = len(rows[0])
            if L:
                P = sum(x.numel() for x in rows[0])
                w, scale = _weights(weights)
                outs = [torch.empty(x.shape, dtype=torch.float32, device=x.device) for x in rows[0]]
                C.rotated_quantized_mean(rows, random.split(rotation_rng, L), random.split_many(client_keys, L),
                                         w, scale, outs, num_levels=int(num_levels), workspace_bytes=workspace_bytes)
                agg = pytree.unflatten(td, outs)
            else:
                agg = pytree.unflatten(td, [])
        new_bits = _bits_per_param(math.log2(num_levels), P, L)
        return agg, CompressionState(F32(aggregator_state.num_bits + new_bits), new_rng)

    return aggregator.Aggregator(init, apply)


def structured_drive_quantizer(rng, *, workspace_bytes: int = C.DEFAULT_WORKSPACE_BYTES) -> aggregator.Aggregator:
    """compression.py:280-320."""

    def init():
        return CompressionState(0.0, np.asarray(rng, np.uint32))

    def apply(clients_params_and_weights, aggregator_state):
        new_rng, rotation_rng = random.split(aggregator_state.rng)
        trees, weights = _consume(clients_params_and_weights)
        client_keys = random.PRNGSequence(rotation_rng).take(len(trees))
        agg, P, L = None, 0, 0
        if trees:
            td, rows = _rows(trees)
            L = len(rows[0])
            if L:
                P = sum(x.numel() for x in rows[0])
                w, scale = _weights(weights)
                flat = torch.empty(P, dtype=torch.float32, device=rows[0][0].device)
                C.drive_mean(rows, random.split_many(client_keys, L), w, scale, flat,
                             workspace_bytes=workspace_bytes)
                outs, o = [], 0
                for x in rows[0]:
                    outs.append(flat[o:o + x.numel()].view(x.shape))
                    o += x.numel()
                agg = pytree.unflatten(td, outs)
            else:
                agg = pytree.unflatten(td, [])
        new_bits = F32(P + 32 * 2 * L)  # int32 tree_size + int, then float32 accumulation
        return agg, CompressionState(F32(aggregator_state.num_bits + new_bits), new_rng)

    return aggregator.Aggregator(init, apply)


def terngrad_quantizer(rng) -> aggregator.Aggregator:
    """compression.py:356-400."""

    def init():
        return CompressionState(0.0, np.asarray(rng, np.uint32))

    def apply(clients_params_and_weights, aggregator_state):
        new_rng, use_rng = random.split(aggregator_state.rng)
        trees, weights = _consume(clients_params_and_weights)
        client_keys = random.PRNGSequence(use_rng).take(len(trees))
        agg, P, L = None, 0, 0
        if trees:
            agg, _, rows, _ = _mean_round(trees, weights, client_keys, _lib.COMP_TERNGRAD)
            P, L = sum(x.numel() for x in rows[0]), len(rows[0])
        new_bits = _bits_per_param(math.log2(3), P, L)
        return agg, CompressionState(F32(aggregator_state.num_bits + new_bits), new_rng)

    return aggregator.Aggregator(init, apply)


# ----------------------------------------------------------------------------- transmitted form
@dataclasses.dataclass
class EncodedDelta:
    """A uniformly quantized delta as a client transmits it: ``codes``, a pytree of uint8 device
    tensors shaped like the delta's leaves (the level index of every element), ``minmax``, a
    float32 ``[L, 2]`` tensor of every leaf's (amin, amax), and ``num_levels`` (2 .. 256). A code
    ``c`` of leaf ``l`` stands for ``vmin + lev[c] * (vmax - vmin)``, ``lev[c] = f32(c) / f32(num_levels - 1)``,
    in float32: the value ``uniform_stochastic_quantize`` returns (compression.py:84-97).

    ``bits`` is 8 (that form) or 1, 2 or 4 with ``2**bits >= num_levels``: every code leaf is then a
    1-D uint8 tensor of ``ceil(n * bits / 8)`` bytes, element ``i`` in byte ``i // (8 // bits)`` at
    bit offset ``bits * (i % (8 // bits))``, low bits first (:func:`pack_codes`), and ``shapes``
    carries the delta's leaf shapes in flatten order, which the packed bytes no longer tell."""
    codes: Any
    minmax: Any
    num_levels: int = _field(metadata={"pytree_node": False})
    bits: int = _field(default=8, metadata={"pytree_node": False})
    shapes: Optional[Tuple[Tuple[int, ...], ...]] = _field(default=None, metadata={"pytree_node": False})


def pack_codes(codes_u8: torch.Tensor, bits: int) -> torch.Tensor:
    """The packed form of uint8 level codes below ``2**bits`` (``bits`` 1, 2 or 4): a 1-D uint8
    tensor of ``ceil(n * bits / 8)`` bytes, element ``i`` of the flattened codes in byte
    ``i // (8 // bits)`` at bit offset ``bits * (i % (8 // bits))``, padding bits zero. Plain torch
    ops, for interchange and tests (the encoder writes this form itself)."""
    if C.check_bits(bits, 2) == 8:
        raise ValueError("pack_codes packs to 1, 2 or 4 bits")
    if not isinstance(codes_u8, torch.Tensor) or codes_u8.dtype != torch.uint8:
        raise TypeError("codes must be a uint8 tensor")
    per = 8 // bits
    flat = codes_u8.reshape(-1)
    fields = torch.zeros(C.packed_bytes(flat.numel(), bits) * per, dtype=torch.int32, device=flat.device)
    fields[:flat.numel()] = flat & ((1 << bits) - 1)
    shifts = bits * torch.arange(per, dtype=torch.int32, device=flat.device)
    return (fields.view(-1, per) << shifts).sum(dim=1).to(torch.uint8)


def unpack_codes(packed: torch.Tensor, n: int, bits: int) -> torch.Tensor:
    """The ``n`` uint8 codes of a :func:`pack_codes` buffer (its padding bits are ignored)."""
    if C.check_bits(bits, 2) == 8:
        raise ValueError("unpack_codes unpacks 1, 2 or 4 bits")
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.uint8 or packed.dim() != 1:
        raise TypeError("packed codes must be a 1-D uint8 tensor")
    if packed.numel() != C.packed_bytes(int(n), bits):
        raise ValueError(f"{n} codes of {bits} bits are {C.packed_bytes(int(n), bits)} bytes, got {packed.numel()}")
    shifts = bits * torch.arange(8 // bits, dtype=torch.int32, device=packed.device)
    fields = (packed.to(torch.int32)[:, None] >> shifts) & ((1 << bits) - 1)
    return fields.reshape(-1)[:int(n)].to(torch.uint8)


def _template_shapes(template) -> Tuple[Tuple[int, ...], ...]:
    return tuple(tuple(tree_util._to_tensor(x).shape) for x in pytree.leaves_of(template))


def _encoded_rows(deltas: Sequence[Any], num_levels: int, shapes=None, bits: int = 8):
    """(treedef, codes [K][L], minmax [K], shapes) of EncodedDelta clients after every check the
    kernels rely on: uint8 codes, one structure and leaf shapes (``shapes``, default client 0's),
    float32 ``[L, 2]`` minmax, and ``num_levels`` and ``bits`` everywhere. With ``bits`` < 8 the
    shapes are the deltas' ``shapes`` fields and a code leaf is 1-D, ``ceil(n * bits / 8)`` bytes."""
    td, rows, mms = None, [], []
    for k, d in enumerate(deltas):
        if not isinstance(d, EncodedDelta):
            raise TypeError(f"client {k}: expected an EncodedDelta, got {type(d).__name__}")
        if C.check_num_levels(d.num_levels) != num_levels:
            raise ValueError(f"client {k} was encoded with num_levels={d.num_levels}, expected {num_levels}")
        if C.check_bits(d.bits, num_levels) != bits:
            raise ValueError(f"client {k} was encoded with bits={d.bits}, expected {bits}")
        if td is None:
            leaves, td = pytree.flatten(d.codes)
        else:
            leaves = pytree.flatten_as(td, d.codes)
        if bits < 8:
            if d.shapes is None:
                raise ValueError(f"client {k}: packed codes need the leaf shapes in EncodedDelta.shapes")
            mine = tuple(tuple(int(v) for v in sh) for sh in d.shapes)
            if shapes is None:
                shapes = mine
            if mine != tuple(tuple(sh) for sh in shapes):
                raise ValueError(f"client {k} has leaf shapes {mine}, expected {tuple(shapes)}")
        if shapes is None:
            shapes = [tuple(x.shape) if isinstance(x, torch.Tensor) else None for x in leaves]
        if len(leaves) != len(shapes):
            raise ValueError(f"client {k} has {len(leaves)} leaves, expected {len(shapes)}")
        for l, (x, sh) in enumerate(zip(leaves, shapes)):
            if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
                raise TypeError(f"client {k} leaf {l}: codes must be uint8 tensors, got "
                                f"{x.dtype if isinstance(x, torch.Tensor) else type(x).__name__}")
            want = sh if bits == 8 else (C.packed_bytes(int(np.prod(sh, dtype=np.int64)), bits),)
            if tuple(x.shape) != want:
                raise ValueError(f"client {k} leaf {l} has shape {tuple(x.shape)}, expected {want}")
        mm = d.minmax
        if not isinstance(mm, torch.Tensor) or mm.dtype != torch.float32:
            raise TypeError(f"client {k}: minmax must be a float32 tensor")
        if tuple(mm.shape) != (len(shapes), 2):
            raise ValueError(f"client {k}: minmax has shape {tuple(mm.shape)}, expected {(len(shapes), 2)}")
        rows.append(leaves)
        mms.append(mm)
    return td, rows, mms, shapes


def uniform_stochastic_encode_pytree(params: PyTree, num_levels: int, rng, bits: int = 8) -> EncodedDelta:
    """The client side of :func:`encoded_mean_aggregator`: ``uniform_stochastic_quantize_pytree``'s
    draws and decisions (leaf keys = split(rng, num_leaves)) kept as level indices, one byte per
    element, instead of decoded float32 values; with ``bits`` 1, 2 or 4 the same indices packed
    (:class:`EncodedDelta`), written in that form by the encoder."""
    num_levels = C.check_num_levels(num_levels)
    bits = C.check_bits(bits, num_levels)
    td, rows = _rows([params])
    L = len(rows[0])
    shapes = None if bits == 8 else tuple(tuple(x.shape) for x in rows[0])
    if not L:
        return EncodedDelta(pytree.unflatten(td, []), torch.empty(0, 2, dtype=torch.float32), num_levels, bits, shapes)
    codes, minmax = C.encode_uniform(rows, random.split(rng, L).reshape(1, L, 2), num_levels, bits)
    return EncodedDelta(pytree.unflatten(td, codes[0]), minmax[0], num_levels, bits, shapes)


def encoded_mean_aggregator(num_levels: int, bits: int = 8, template: Optional[PyTree] = None) -> aggregator.Aggregator:
    """The server side of a round whose clients transmit :class:`EncodedDelta`: ``apply`` takes
    ``(client_id, EncodedDelta, weight)`` triples and returns ``tree_mean`` over the decoded deltas,
    folded straight from the codes in one launch (a quarter of the float32 fold's bytes, no
    decoded copy), and a :class:`CompressionState` whose ``num_bits`` grows as the reference's
    ``uniform_stochastic_quantizer`` counts them. With clients encoded by
    :func:`uniform_stochastic_encode_pytree` under that aggregator's keys the mean is bit for bit
    its mean. ``bits`` 1, 2 or 4: the clients' codes are packed and folded in that form (an
    eighth to a thirty-second of the float32 bytes); the leaf shapes are the deltas' ``shapes``
    fields, checked against ``template``'s (a pytree of the model's leaves) when one is given."""
    num_levels = C.check_num_levels(num_levels)
    bits = C.check_bits(bits, num_levels)
    expect = None if template is None else _template_shapes(template)

    def init():
        return CompressionState(0.0, None)

    def apply(clients_params_and_weights, aggregator_state):
        deltas, weights = _consume(clients_params_and_weights)
        agg, P, L = None, 0, 0
        if deltas:
            td, rows, mms, shapes = _encoded_rows(deltas, num_levels, expect, bits)
            L = len(rows[0])
            if L:
                device = tree_util._find_device(rows[0])
                rows = [[x.to(device).contiguous() for x in r] for r in rows]
                w, scale = _weights(weights)
                outs = [torch.empty(sh, dtype=torch.float32, device=device) for sh in shapes]
                P = sum(x.numel() for x in outs)
                minmax = torch.stack([m.to(device) for m in mms])
                C.codes_mean(rows, minmax, w, scale, outs, num_levels, bits)
                agg = pytree.unflatten(td, outs)
            else:
                agg = pytree.unflatten(td, [])
        new_bits = _bits_per_param(math.log2(num_levels), P, L)
        return agg, CompressionState(F32(aggregator_state.num_bits + new_bits), aggregator_state.rng)

    return aggregator.Aggregator(init, apply)


@dataclasses.dataclass
class DriveDelta:
    """A DRIVE-compressed delta as a client transmits it: ``signs``, a pytree shaped like the delta
    whose every leaf is a 1-D uint8 tensor of ``ceil(d / 8)`` bytes, ``d = 2 ** ceil(log2(n))`` the
    leaf's rotated length: rotated coordinate ``i`` in byte ``i // 8`` at bit ``i % 8``, low bit
    first (:func:`pack_codes`' order), 1 where the rotated value is ``< 0`` (zeros, ``-0.0`` and NaNs
    are sent as 0; the padding bits of a leaf with ``d < 8`` are written as zero and ignored on
    reading); ``scales``, a float32 ``[L, 2]`` tensor of every rotated leaf's
    ``(f32(sum y**2), f32(sum |y|))``; ``shapes``, the delta's leaf shapes in flatten order. A sign
    ``s`` of leaf ``l`` stands for ``(A * s) / b`` in float32 with ``(A, b) = scales[l]``:
    ``drive_pytree``'s value (compression.py:269-277)."""
    signs: Any
    scales: Any
    shapes: Tuple[Tuple[int, ...], ...] = _field(metadata={"pytree_node": False})


def drive_round_keys(rng, num_clients: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(new_rng, client_keys [num_clients, 2])``: the key stream of one
    ``structured_drive_quantizer`` round (compression.py:298-301), so that clients and server
    derive the same rotation keys. Client ``k`` encodes with ``client_keys[k]``."""
    new_rng, rotation_rng = random.split(np.asarray(rng, np.uint32))
    return new_rng, random.PRNGSequence(rotation_rng).take(int(num_clients))


def drive_encode_pytree(params: PyTree, rng) -> DriveDelta:
    """The client side of :func:`drive_mean_aggregator`: every leaf rotated under its key of
    ``split(rng, num_leaves)`` (``structured_rotation_pytree``'s rotation), then only the sign bits
    and the two sums ``drive_pytree`` needs are kept (:class:`DriveDelta`). Float32 leaves."""
    td, rows = _rows([params])
    L = len(rows[0])
    shapes = tuple(tuple(x.shape) for x in rows[0])
    if not L:
        return DriveDelta(pytree.unflatten(td, []), torch.empty(0, 2, dtype=torch.float32), shapes)
    bits, scales = C.drive_encode(rows, random.split(rng, L))
    return DriveDelta(pytree.unflatten(td, bits), scales, shapes)


def _drive_rows(deltas: Sequence[Any], shapes=None):
    """(treedef, sign leaves [K][L], scales [K], shapes) of DriveDelta clients after every check the
    kernels rely on: one structure, equal ``shapes`` (``shapes``, default client 0's), 1-D uint8
    leaves of ``ceil(d / 8)`` bytes and float32 ``[L, 2]`` scales."""
    td, rows, scs = None, [], []
    for k, d in enumerate(deltas):
        if not isinstance(d, DriveDelta):
            raise TypeError(f"client {k}: expected a DriveDelta, got {type(d).__name__}")
        if td is None:
            leaves, td = pytree.flatten(d.signs)
        else:
            leaves = pytree.flatten_as(td, d.signs)
        mine = tuple(tuple(int(v) for v in sh) for sh in d.shapes)
        if shapes is None:
            shapes = mine
        if mine != tuple(tuple(sh) for sh in shapes):
            raise ValueError(f"client {k} has leaf shapes {mine}, expected {tuple(shapes)}")
        if len(leaves) != len(shapes):
            raise ValueError(f"client {k} has {len(leaves)} leaves, expected {len(shapes)}")
        for l, (x, sh) in enumerate(zip(leaves, shapes)):
            if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
                raise TypeError(f"client {k} leaf {l}: sign bits must be uint8 tensors, got "
                                f"{x.dtype if isinstance(x, torch.Tensor) else type(x).__name__}")
            want = ((C.padded_size(int(np.prod(sh, dtype=np.int64))) + 7) // 8,)
            if tuple(x.shape) != want:
                raise ValueError(f"client {k} leaf {l} has shape {tuple(x.shape)}, expected {want}")
        sc = d.scales
        if not isinstance(sc, torch.Tensor) or sc.dtype != torch.float32:
            raise TypeError(f"client {k}: scales must be a float32 tensor")
        if tuple(sc.shape) != (len(shapes), 2):
            raise ValueError(f"client {k}: scales has shape {tuple(sc.shape)}, expected {(len(shapes), 2)}")
        rows.append(leaves)
        scs.append(sc)
    return td, rows, scs, shapes


def drive_mean_aggregator(rng, template: Optional[PyTree] = None, *,
                          workspace_bytes: int = C.DEFAULT_WORKSPACE_BYTES) -> aggregator.Aggregator:
    """The server side of a round whose clients transmit :class:`DriveDelta`: ``apply`` takes
    ``(client_id, DriveDelta, weight)`` triples, advances its key as ``structured_drive_quantizer``
    does (:func:`drive_round_keys`) and returns ``tree_mean`` over the decoded, inverse-rotated
    deltas: one inverse Walsh-Hadamard transform per client straight from the sign bits, the fold
    in the epilogue of its last pass, so neither the decoded nor the unrotated deltas reach HBM
    (leaves of at most 8192 padded elements touch no intermediate at all). ``num_bits`` grows as
    ``structured_drive_quantizer`` counts it. With clients encoded by :func:`drive_encode_pytree`
    under this round's keys the mean is bit for bit that aggregator's over clients with no rotated
    coordinate that is exactly zero or NaN. Such a coordinate is sent as ``+``: it decodes to
    ``+A/b`` where the fused round has ``sign(0) = 0``, which moves every output of that leaf by
    ``(A/b) / sqrt(d) * w_k / W``. With billions of rotated coordinates a round (1024 clients x
    millions of parameters) a few tens of them occur in every round, so the two means then differ
    by a few 1e-5 (DESIGN.md §3za has the counts). ``template`` (a pytree of the model's leaves) checks the
    clients' ``shapes``; ``workspace_bytes`` bounds the batch of clients whose workspace rows
    (leaves above 8192 padded elements only) and rotation signs are held at once."""
    expect = None if template is None else _template_shapes(template)

    def init():
        return CompressionState(0.0, np.asarray(rng, np.uint32))

    def apply(clients_params_and_weights, aggregator_state):
        deltas, weights = _consume(clients_params_and_weights)
        new_rng, client_keys = drive_round_keys(aggregator_state.rng, len(deltas))
        agg, P, L = None, 0, 0
        if deltas:
            td, rows, scs, shapes = _drive_rows(deltas, expect)
            L = len(rows[0])
            if L:
                device = tree_util._find_device(rows[0])
                rows = [[x.to(device).contiguous() for x in r] for r in rows]
                w, scale = _weights(weights)
                leaf_n = [int(np.prod(sh, dtype=np.int64)) for sh in shapes]
                P = sum(leaf_n)
                flat = torch.empty(P, dtype=torch.float32, device=device)
                scales = torch.stack([s.to(device) for s in scs]).contiguous()
                C.drive_signs_mean(rows, scales, random.split_many(client_keys, L), w, scale, leaf_n, flat,
                                   workspace_bytes=workspace_bytes)
                outs, o = [], 0
                for sh, n in zip(shapes, leaf_n):
                    outs.append(flat[o:o + n].view(sh))
                    o += n
                agg = pytree.unflatten(td, outs)
            else:
                agg = pytree.unflatten(td, [])
        new_bits = F32(P + 32 * 2 * L)
        return agg, CompressionState(F32(aggregator_state.num_bits + new_bits), new_rng)

    return aggregator.Aggregator(init, apply)


@dataclasses.dataclass
class SparsifierState:
    """State of :func:`top_k_sparsifier`: the bits transmitted so far, ``0.0`` at first and a 0-d
    float64 device tensor after the first non-empty round (reading it is the only synchronisation)."""
    num_bits: Any


def top_k_sparsifier(k) -> aggregator.Aggregator:
    """Top-k sparsification: every client sends only its ``k`` largest-magnitude coordinates
    (``k`` an int count or a float fraction of the model size, :func:`fedjax_amd.kernels.topk_count`),
    and the server takes the weighted mean of the sparsified deltas
    (:func:`fedjax_amd.tree_util.tree_topk_mean`: a global threshold per client, all ties kept, a NaN
    kept first). There is no reference counterpart; the mean is ``tree_mean``'s over the
    sparsified deltas, bit for bit.

    Each round adds ``mean_k(sent_k) * (32 + ceil(log2 P))`` to ``num_bits``: a float32 value and
    an index per transmitted coordinate, averaged over the clients, formed with torch ops on the
    stream from the device counts. An empty round returns ``None`` and leaves the state as it is."""
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, float, np.integer, np.floating)):
        raise TypeError(f"k must be an int count or a float fraction in (0, 1], not {type(k).__name__}")

    def init():
        return SparsifierState(0.0)

    def apply(clients_params_and_weights, aggregator_state):
        trees, weights = _consume(clients_params_and_weights)
        if not trees:
            return None, aggregator_state
        res = tree_util.tree_topk_mean(list(zip(trees, weights)), k)
        P = sum(int(x.numel()) for x in map(tree_util._to_tensor, pytree.leaves_of(trees[0])))
        if P == 0:
            return res.mean, aggregator_state
        per_coordinate = 32 + (P - 1).bit_length()  # value bits + ceil(log2 P) index bits
        new_bits = res.sent.to(torch.float64).mean() * per_coordinate
        return res.mean, SparsifierState(aggregator_state.num_bits + new_bits)

    return aggregator.Aggregator(init, apply)


@dataclasses.dataclass
class SparseDelta:
    """A top-k sparsified delta as a client transmits it: ``indices``, a 1-D int32 tensor, strictly
    increasing, in ``[0, P)``; ``values``, a 1-D float32 tensor of the same length, the kept
    elements verbatim; ``shapes``, the delta's leaf shapes in flatten order. An index counts the
    elements of the client's row, its leaves back to back in flatten order (``P < 2^31``). A list
    from :func:`topk_encode_pytree` holds exactly the coordinates whose magnitude key
    ``bits & 0x7fffffff`` is ``>= max(T, 1)``, ``T`` the client's ``k``-th largest key: all ties at
    the threshold, a NaN first, never a zero."""
    indices: Any
    values: Any
    shapes: Tuple[Tuple[int, ...], ...] = _field(metadata={"pytree_node": False})


def topk_encode_pytree(params: PyTree, k) -> SparseDelta:
    """The client side of :func:`sparse_mean_aggregator`: the existing top-k select over the whole
    delta (``k`` as in :func:`top_k_sparsifier`), then an order-preserving compaction of the kept
    coordinates into a :class:`SparseDelta` on the device. The list's length is the select's
    ``sent``, which is read back once to size the two tensors: one host synchronisation, so the
    call is refused under stream capture. Float32 leaves."""
    kernels.refuse_capture("topk_encode_pytree", "it reads the number of kept coordinates back to size the lists")
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, float, np.integer, np.floating)):
        raise TypeError(f"k must be an int count or a float fraction in (0, 1], not {type(k).__name__}")
    td, rows = _rows([params])
    shapes = tuple(tuple(x.shape) for x in rows[0])
    leaf_n = np.array([x.numel() for x in rows[0]], dtype=np.int64)
    device = tree_util._find_device(rows[0])
    if not leaf_n.sum():
        return SparseDelta(torch.empty(0, dtype=torch.int32, device=device),
                           torch.empty(0, dtype=torch.float32, device=device), shapes)
    tables = kernels.TopKTables(tree_util._ptr_table(rows), leaf_n).upload(device)
    thr, sent = kernels.topk_select_ptrs(tables, kernels.topk_count(k, tables.P))
    offsets = kernels.sparse_offsets(sent)
    n = int(sent.item())  # the one synchronisation
    indices = torch.empty(n, dtype=torch.int32, device=device)
    values = torch.empty(n, dtype=torch.float32, device=device)
    kernels.topk_compact_ptrs(tables, thr, offsets, indices, values)
    return SparseDelta(indices, values, shapes)


def _sparse_rows(deltas: Sequence[Any], shapes=None):
    """(indices [K], values [K], shapes) of SparseDelta clients after every check the fold relies
    on: int32 indices and float32 values, both 1-D and of one length (at most ``P``), and equal
    ``shapes`` (``shapes``, default client 0's)."""
    idx, val = [], []
    for k, d in enumerate(deltas):
        if not isinstance(d, SparseDelta):
            raise TypeError(f"client {k}: expected a SparseDelta, got {type(d).__name__}")
        mine = tuple(tuple(int(v) for v in sh) for sh in d.shapes)
        if shapes is None:
            shapes = mine
        if mine != tuple(tuple(sh) for sh in shapes):
            raise ValueError(f"client {k} has leaf shapes {mine}, expected {tuple(shapes)}")
        for name, x, dt in (("indices", d.indices, torch.int32), ("values", d.values, torch.float32)):
            if not isinstance(x, torch.Tensor) or x.dtype != dt:
                raise TypeError(f"client {k}: {name} must be a {str(dt).split('.')[-1]} tensor, got "
                                f"{x.dtype if isinstance(x, torch.Tensor) else type(x).__name__}")
            if x.dim() != 1:
                raise ValueError(f"client {k}: {name} must be 1-D, got shape {tuple(x.shape)}")
        if d.indices.numel() != d.values.numel():
            raise ValueError(f"client {k} has {d.indices.numel()} indices and {d.values.numel()} values")
        P = sum(int(np.prod(sh, dtype=np.int64)) for sh in mine)
        if d.indices.numel() > P:
            raise ValueError(f"client {k} sends {d.indices.numel()} coordinates of a delta of {P}")
        idx.append(d.indices)
        val.append(d.values)
    return idx, val, shapes


def sparse_mean_aggregator(template: Optional[PyTree] = None) -> aggregator.Aggregator:
    """The server side of a round whose clients transmit :class:`SparseDelta`: ``apply`` takes
    ``(client_id, SparseDelta, weight)`` triples and returns ``tree_mean`` over the sparsified
    deltas, folded straight from the lists: one table image uploaded, one launch, no dense copy
    (``fjcomp_sparse_fold``). With clients encoded by :func:`topk_encode_pytree` the mean is
    :func:`top_k_sparsifier`'s bit for bit, except that a coordinate whose every term is a zero
    comes out as ``+0`` where that fold can give ``-0``. The state is a :class:`SparsifierState`
    whose ``num_bits`` grows by ``mean_k(len_k) * (32 + ceil(log2 P))`` in float64, the value
    :func:`top_k_sparsifier` adds for the same clients (formed on the host from the list lengths).
    The mean's leaves are views into one flat tensor, arranged as ``template`` (a pytree of the
    model's leaves, whose shapes the clients' ``shapes`` are checked against) or, without one, as
    a list in flatten order. An empty round returns ``None`` and the state unchanged."""
    expect = None if template is None else _template_shapes(template)
    treedef = None if template is None else pytree.flatten(template)[1]

    def init():
        return SparsifierState(0.0)

    def apply(clients_params_and_weights, aggregator_state):
        deltas, weights = _consume(clients_params_and_weights)
        if not deltas:
            return None, aggregator_state
        idx, val, shapes = _sparse_rows(deltas, expect)
        kernels.check_topk_clients(len(deltas))
        device = tree_util._find_device(idx)
        idx = [x.to(device).contiguous() for x in idx]
        val = [x.to(device).contiguous() for x in val]
        w, scale = _weights(weights)
        leaf_n = [int(np.prod(sh, dtype=np.int64)) for sh in shapes]
        P = sum(leaf_n)
        flat = torch.empty(P, dtype=torch.float32, device=device)
        counts = [x.numel() for x in idx]
        tables = kernels.SparseTables([x.data_ptr() for x in idx], [x.data_ptr() for x in val], counts, P, w)
        kernels.sparse_fold(tables.upload(device), scale=scale, out=flat)
        outs, o = [], 0
        for sh, n in zip(shapes, leaf_n):
            outs.append(flat[o:o + n].view(sh))
            o += n
        agg = outs if treedef is None else pytree.unflatten(treedef, outs)
        if P == 0:
            return agg, aggregator_state
        new_bits = np.float64(np.mean(np.array(counts, dtype=np.float64)) * (32 + (P - 1).bit_length()))
        return agg, SparsifierState(aggregator_state.num_bits + new_bits)

    return aggregator.Aggregator(init, apply)


# ----------------------------------------------------------------------------- sign bits, majority vote
@dataclasses.dataclass
class SignDelta:
    """A delta as a signSGD client transmits it: ``signs``, a pytree shaped like the delta whose
    every leaf is a 1-D uint8 tensor of ``ceil(n / 8)`` bytes: coordinate ``i`` of the flattened
    leaf in byte ``i // 8`` at bit ``i % 8``, low bit first (``pack_codes(codes, 1)``'s order), 1
    exactly where the value is ``< 0`` (``+0``, ``-0`` and NaN are sent as 0; the padding bits of
    the last byte are written as 0 and ignored by the server); ``shapes``, the delta's leaf shapes
    in flatten order."""
    signs: Any
    shapes: Tuple[Tuple[int, ...], ...] = _field(metadata={"pytree_node": False})


def sign_encode_pytree(params: PyTree) -> SignDelta:
    """The client side of :func:`majority_vote_aggregator`: one bit per coordinate, written packed
    by one launch over all leaves, with no host synchronisation. Float32 leaves (int32 leaves are
    converted; bfloat16 raises ``TypeError``)."""
    kernels.refuse_capture("sign_encode_pytree", "it uploads the leaf table through a pinned staging buffer")
    td, rows = _rows([params])
    shapes = tuple(tuple(x.shape) for x in rows[0])
    if not rows[0]:
        return SignDelta(pytree.unflatten(td, []), shapes)
    return SignDelta(pytree.unflatten(td, C.sign_pack([x.contiguous() for x in rows[0]])), shapes)


def _sign_rows(deltas: Sequence[Any], shapes=None):
    """(treedef, sign leaves [K][L], shapes) of SignDelta clients after every check the kernel relies
    on: one structure, equal ``shapes`` (``shapes``, default client 0's) and 1-D uint8 leaves of
    ``ceil(n / 8)`` bytes."""
    td, rows = None, []
    for k, d in enumerate(deltas):
        if not isinstance(d, SignDelta):
            raise TypeError(f"client {k}: expected a SignDelta, got {type(d).__name__}")
        if td is None:
            leaves, td = pytree.flatten(d.signs)
        else:
            leaves = pytree.flatten_as(td, d.signs)
        mine = tuple(tuple(int(v) for v in sh) for sh in d.shapes)
        if shapes is None:
            shapes = mine
        if mine != tuple(tuple(sh) for sh in shapes):
            raise ValueError(f"client {k} has leaf shapes {mine}, expected {tuple(shapes)}")
        if len(leaves) != len(shapes):
            raise ValueError(f"client {k} has {len(leaves)} leaves, expected {len(shapes)}")
        for l, (x, sh) in enumerate(zip(leaves, shapes)):
            if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
                raise TypeError(f"client {k} leaf {l}: sign bits must be uint8 tensors, got "
                                f"{x.dtype if isinstance(x, torch.Tensor) else type(x).__name__}")
            want = (C.packed_bytes(int(np.prod(sh, dtype=np.int64)), 1),)
            if tuple(x.shape) != want:
                raise ValueError(f"client {k} leaf {l} has shape {tuple(x.shape)}, expected {want}")
        rows.append(leaves)
    return td, rows, shapes


def majority_vote_aggregator(output: str = "sign", template: Optional[PyTree] = None) -> aggregator.Aggregator:
    """signSGD with majority vote (Bernstein et al., ICLR 2019), the server side of a round whose
    clients transmit :class:`SignDelta`: ``apply`` takes ``(client_id, SignDelta, weight)`` triples.
    The weights are ignored, as in every robust rule here: a client must not scale its own vote.
    Per coordinate, with ``c`` of the ``K`` clients sending a 1 (negative):

    * ``output="sign"``: float32 ``-1.0`` if ``2c > K``, ``+1.0`` if ``2c < K``, ``+0.0`` on a tie;
    * ``output="mean"``: the mean of the clients' signs, ``fl(f32(K - 2c) * f32(1 / K))``.

    One launch counts the bits in bit-sliced integer counters (``fjcomp_sign_vote``), so the result
    does not depend on any order and two rounds over the same bits agree bit for bit. The state is
    a :class:`CompressionState` whose ``num_bits`` grows by ``F32(P)`` a round (one bit per
    parameter, nothing else) and whose ``rng`` stays ``None``. ``1 <= K <= 4096``. ``template`` (a
    pytree of the model's leaves) checks the clients' ``shapes``. An empty round returns ``None``
    and the state unchanged. Not capturable into a graph: the call uploads a pointer table."""
    mode = C.check_vote_output(output)
    expect = None if template is None else _template_shapes(template)

    def init():
        return CompressionState(0.0, None)

    def apply(clients_params_and_weights, aggregator_state):
        deltas, _ = _consume(clients_params_and_weights)
        if not deltas:
            return None, aggregator_state
        kernels.refuse_capture("majority_vote_aggregator", "it uploads a pointer table through a pinned staging buffer")
        td, rows, shapes = _sign_rows(deltas, expect)
        C.check_vote_clients(len(rows))
        if not rows[0]:
            return pytree.unflatten(td, []), aggregator_state
        device = tree_util._find_device(rows[0])
        rows = [[x.to(device).contiguous() for x in r] for r in rows]
        outs = [torch.empty(sh, dtype=torch.float32, device=device) for sh in shapes]
        C.sign_vote(rows, mode, outs)
        P = sum(x.numel() for x in outs)
        return pytree.unflatten(td, outs), CompressionState(F32(aggregator_state.num_bits + F32(P)), None)

    return aggregator.Aggregator(init, apply)


__all__ = ["CompressionState", "SparsifierState", "top_k_sparsifier", "EncodedDelta", "encoded_mean_aggregator",
           "SparseDelta", "topk_encode_pytree", "sparse_mean_aggregator",
           "SignDelta", "sign_encode_pytree", "majority_vote_aggregator",
           "uniform_stochastic_encode_pytree", "pack_codes", "unpack_codes", "DriveDelta", "drive_round_keys",
           "drive_encode_pytree", "drive_mean_aggregator",
           "arithmetic_encoding_num_bits", "binary_stochastic_quantize", "drive_pytree",
           "num_leaves", "rotated_uniform_stochastic_quantizer", "structured_drive_quantizer", "terngrad_quantize",
           "terngrad_quantize_pytree", "terngrad_quantizer", "uniform_stochastic_quantize",
           "uniform_stochastic_quantize_pytree", "uniform_stochastic_quantizer"]
