"""The msgpack wire format of fedjax_amd.ingest (CPU): the hand-written zero-copy decoder
against ``msgpack_deserialize`` over a seeded structural sweep and over encodings the packer
never chooses, its single exception type on malformed input, and the serializer's treatment
of host tensors, strided arrays and tuples.

``msgpack_deserialize`` (msgpack's own unpacker plus the reference's ext hook) is the
reference throughout: the view decoder must return the same structure, Python types,
dtypes, shapes and bits. Floats compare as bit patterns. The one allowed difference is
asserted too: ndarray leaves of the view decoder are read-only and share memory with the
payload."""
import struct

import msgpack
import numpy as np
import pytest
import torch

from fedjax_amd import ingest
from fedjax_amd.ingest import BF16Array

SEED = 20260
NUM_CASES = 300


# ------------------------------------------------------------------ comparison
def _f64_bits(x):
    return struct.pack("<d", x)


def assert_same(ref, got, enc, path="$"):
    """``got`` (view decoder) is ``ref`` (msgpack_deserialize): types, structure, bits."""
    assert type(got) is type(ref), f"{path}: {type(got).__name__} for {type(ref).__name__}"
    if isinstance(ref, dict):
        assert [(type(k), k) for k in got] == [(type(k), k) for k in ref], path
        for k in ref:
            assert_same(ref[k], got[k], enc, f"{path}[{k!r:.20}]")
    elif isinstance(ref, list):
        assert len(got) == len(ref), path
        for j, (r, g) in enumerate(zip(ref, got)):
            assert_same(r, g, enc, f"{path}[{j}]")
    elif isinstance(ref, np.ndarray):
        assert got.dtype == ref.dtype and got.shape == ref.shape, f"{path}: {got.dtype}{got.shape}"
        if ref.dtype == object:
            for r, g in zip(ref.ravel().tolist(), got.ravel().tolist()):
                assert type(g) is type(r) and g == r, path
            return
        assert got.tobytes() == ref.tobytes(), path
        assert not got.flags.writeable, f"{path}: a writeable array"
        if got.size:
            assert np.shares_memory(got, np.frombuffer(enc, np.uint8)), f"{path}: a copy, not a view"
    elif isinstance(ref, np.generic):
        assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes(), path
    elif isinstance(ref, float):
        assert _f64_bits(got) == _f64_bits(ref), path
    elif isinstance(ref, complex):
        assert (_f64_bits(got.real), _f64_bits(got.imag)) == (_f64_bits(ref.real), _f64_bits(ref.imag)), path
    else:  # int, bool, None, str, bytes, msgpack.ExtType
        assert got == ref, path


def check_agreement(enc):
    ref = ingest.msgpack_deserialize(enc)
    got = ingest.msgpack_deserialize_view(enc)
    assert_same(ref, got, enc)
    return got


# ------------------------------------------------------- an independent header walk
def walk_headers(buf, i=0, out=None):
    """(offset, kind, header bytes) of every msgpack header of the object at buf[i:], the
    (shape, dtype, data) triple inside ndarray / npscalar ext payloads included. Returns
    (headers, next offset). It decodes no values: it only tells the sweep which header
    kinds a payload holds and the truncation test where the headers are."""
    out = [] if out is None else out
    b = buf[i]
    fixed = {0xC0: 0, 0xC2: 0, 0xC3: 0, 0xCA: 4, 0xCB: 8, 0xCC: 1, 0xCD: 2, 0xCE: 4, 0xCF: 8,
             0xD0: 1, 0xD1: 2, 0xD2: 4, 0xD3: 8}

    def length(nbytes):
        return int.from_bytes(buf[i + 1:i + 1 + nbytes], "big")

    def ext(hdr, n):
        code = struct.unpack_from(">b", buf, i + hdr - 1)[0]
        if code in (1, 3):
            walk_headers(buf, i + hdr, out)
        return i + hdr + n

    def items(hdr, n):
        j = i + hdr
        for _ in range(n):
            _, j = walk_headers(buf, j, out)
        return j

    if b <= 0x7F or b >= 0xE0:
        return out, i + 1
    if b <= 0x8F:
        out.append((i, "fixmap", 1))
        return out, items(1, 2 * (b & 0x0F))
    if b <= 0x9F:
        out.append((i, "fixarray", 1))
        return out, items(1, b & 0x0F)
    if b <= 0xBF:
        out.append((i, "fixstr", 1))
        return out, i + 1 + (b & 0x1F)
    if b in fixed:
        out.append((i, "scalar", 1 + fixed[b]))
        return out, i + 1 + fixed[b]
    for base, name, payload in ((0xC4, "bin", False), (0xD9, "str", False), (0xC7, "ext", True)):
        if base <= b <= base + 2:
            nb = 1 << (b - base)
            hdr = 1 + nb + (1 if payload else 0)
            out.append((i, f"{name}{8 * nb}", hdr))
            return out, (ext(hdr, length(nb)) if payload else i + hdr + length(nb))
    if 0xD4 <= b <= 0xD8:
        out.append((i, "fixext", 2))
        return out, ext(2, 1 << (b - 0xD4))
    if b in (0xDC, 0xDD, 0xDE, 0xDF):
        nb = 4 if b & 1 else 2
        is_map = b >= 0xDE
        out.append((i, f"{'map' if is_map else 'array'}{8 * nb}", 1 + nb))
        return out, items(1 + nb, length(nb) * (2 if is_map else 1))
    raise AssertionError(f"byte 0x{b:02x}")


# ------------------------------------------------------------------ the sweep
INT_EDGES = sorted({s * (2 ** p) + d for p in (7, 8, 15, 16, 31, 32) for s in (1, -1) for d in (-1, 0, 1)}
                   | {-32, -33, -31, 2 ** 64 - 1, 2 ** 64 - 2, -2 ** 63, -2 ** 63 + 1, 0, 1, -1, 127})
FLOATS = [0.0, -0.0, 1.5, -2.75e-300, 5e-324, float("inf"), float("-inf"), float("nan"),
          struct.unpack("<d", struct.pack("<Q", 0xFFF8000000001234))[0], 3.4e38, 1e308]
SCALAR_DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64,
                 np.float16, np.float32, np.float64, np.complex64, np.complex128, np.bool_]
ARRAY_DTYPES = [np.float16, np.float32, np.float64, np.int8, np.int16, np.int32, np.int64,
                np.uint8, np.uint16, np.uint32, np.uint64, np.bool_, np.complex64]
SHAPES = [(), (0,), (0, 3), (1,), (3, 4)]
KEY_LENGTHS = [0, 31, 32, 255, 256]
EXT_PAYLOAD_EDGES = [255, 256, 65535, 65536]


def _array(rng, dtype, shape):
    n = int(np.prod(shape, dtype=np.int64))
    raw = rng.randint(0, 256, size=n * np.dtype(dtype).itemsize).astype(np.uint8)
    if dtype is np.bool_:
        return (raw & 1).astype(np.bool_).reshape(shape)
    return raw.view(dtype).reshape(shape)  # every bit pattern: NaNs and subnormals too


def _array_with_ext_payload(rng, nbytes):
    """A uint8 vector whose ndarray ext payload is exactly ``nbytes`` long."""
    for n in range(nbytes, max(0, nbytes - 32), -1):
        if len(msgpack.packb(((n,), "uint8", bytes(n)), use_bin_type=True)) == nbytes:
            return _array(rng, np.uint8, (n,))
    raise AssertionError(nbytes)


def _key(rng, n):
    return "".join(chr(rng.randint(0x61, 0x7B)) for _ in range(n))


def _leaf(rng):
    kind = rng.randint(0, 10)
    if kind == 0:
        return INT_EDGES[rng.randint(len(INT_EDGES))]
    if kind == 1:
        return FLOATS[rng.randint(len(FLOATS))]
    if kind == 2:
        return [None, True, False, complex(1.5, -0.0), complex(float("nan"), float("inf"))][rng.randint(5)]
    if kind == 3:
        dt = SCALAR_DTYPES[rng.randint(len(SCALAR_DTYPES))]
        return _array(rng, dt, ())[()]
    if kind == 4:
        return BF16Array(_array(rng, np.uint16, SHAPES[rng.randint(len(SHAPES))]))
    if kind == 5:
        shape = [(3, 1), (0,), (2, 2), (1,)][rng.randint(4)]
        n = int(np.prod(shape))
        flat = [bytes(rng.randint(0, 256, size=rng.randint(0, 5)).astype(np.uint8)) for _ in range(n)]
        a = np.empty(n, dtype=object)
        a[:] = flat
        return a.reshape(shape)
    if kind == 6:
        return _key(rng, [0, 1, 31, 32, 255, 256, 300][rng.randint(7)])
    if kind == 7:  # a bin value
        return bytes(rng.randint(0, 256, size=[0, 3, 255, 256][rng.randint(4)]).astype(np.uint8))
    return _array(rng, ARRAY_DTYPES[rng.randint(len(ARRAY_DTYPES))], SHAPES[rng.randint(len(SHAPES))])


def _tree(rng, depth):
    if depth == 0 or rng.rand() < 0.3:
        return _leaf(rng)
    n = rng.randint(0, 4)
    if rng.rand() < 0.5:
        return [_tree(rng, depth - 1) for _ in range(n)]
    return {_key(rng, rng.randint(0, 6)) + str(j): _tree(rng, depth - 1) for j in range(n)}


def _edge(rng, j):
    """The j-th forced edge of the sweep, as a subtree."""
    edges = (
        [lambda n=n: {_key(rng, n): _leaf(rng)} for n in KEY_LENGTHS]
        + [lambda n=n: [_leaf(rng) if q % 5 == 0 else q for q in range(n)] for n in (15, 16)]
        + [lambda n=n: {f"k{q:02d}": (_leaf(rng) if q % 5 == 0 else q) for q in range(n)} for n in (15, 16)]
        + [lambda n=n: _array_with_ext_payload(rng, n) for n in EXT_PAYLOAD_EDGES]
        + [lambda: [[[[[[_leaf(rng)]]]], {"a": {"b": {"c": {"d": {"e": _leaf(rng)}}}}}]]]
        + [lambda: list(INT_EDGES), lambda: list(FLOATS)]
        + [lambda: [_array(rng, dt, ())[()] for dt in SCALAR_DTYPES]]
        + [lambda s=s: [_array(rng, dt, s) for dt in ARRAY_DTYPES] for s in SHAPES]
        + [lambda n=n: _array(rng, np.float32, (n,)) for n in (16384, 16400)]  # ext32 through f32
    )
    return edges[j % len(edges)]()


def _case(i):
    rng = np.random.RandomState(SEED + i)
    tree = _tree(rng, 5)
    edge = _edge(rng, i)
    if isinstance(tree, dict):
        tree["edge"] = edge
        return tree
    return [tree, edge]


def test_decoders_agree_on_seeded_structural_sweep():
    counts = {k: 0 for k in ("ext8", "ext16", "ext32", "str8", "str16", "array16", "map16")}
    for i in range(NUM_CASES):
        enc = ingest.msgpack_serialize(_case(i))
        check_agreement(enc)
        headers, end = walk_headers(enc)
        assert end == len(enc)
        kinds = {k for _, k, _ in headers}
        for k in counts:
            counts[k] += k in kinds
    # a change to the generator must not quietly drop an edge
    assert all(v >= 5 for v in counts.values()), counts


def test_sweep_reaches_the_ext_and_container_edges_exactly():
    """The edges themselves, not only their header kinds: ext payloads of 255 / 256 and
    65535 / 65536 bytes, 15 / 16 entries, key lengths 31 / 32 and 255 / 256."""
    rng = np.random.RandomState(SEED)
    for nbytes, kind in ((255, "ext8"), (256, "ext16"), (65535, "ext16"), (65536, "ext32")):
        enc = ingest.msgpack_serialize(_array_with_ext_payload(rng, nbytes))
        assert walk_headers(enc)[0][0][1] == kind
        check_agreement(enc)
    for n, kind in ((15, "fixarray"), (16, "array16")):
        enc = ingest.msgpack_serialize(list(range(n)))
        assert walk_headers(enc)[0][0][1] == kind
        check_agreement(enc)
    for n, kind in ((15, "fixmap"), (16, "map16")):
        enc = ingest.msgpack_serialize({str(q): q for q in range(n)})
        assert walk_headers(enc)[0][0][1] == kind
        check_agreement(enc)
    for n, kind in ((0, "fixstr"), (31, "fixstr"), (32, "str8"), (255, "str8"), (256, "str16")):
        enc = ingest.msgpack_serialize({"x" * n: 1})
        assert walk_headers(enc)[0][1][1] == kind
        check_agreement(enc)


# --------------------------------------------- encodings the packer never chooses
def _u32(n):
    return struct.pack(">I", n)


def _nd_payload(shape, name, data):
    return msgpack.packb((shape, name, data), use_bin_type=True)


HAND_BUILT = {
    "float32": b"\x92\xca" + struct.pack(">f", 1.1) + b"\xca" + struct.pack(">I", 0xFFC00001),
    "str32": b"\xdb" + _u32(2) + b"ab",
    "str32 empty": b"\xdb" + _u32(0),
    "bin32": b"\xc6" + _u32(3) + b"\x00\xff\x80",
    "array32": b"\xdd" + _u32(2) + b"\x01\xa1x",
    "map32": b"\xdf" + _u32(1) + b"\xa1k\x07",
    "array16 of 1": b"\xdc\x00\x01\xc0",
    "map16 of 0": b"\xde\x00\x00",
    "ext32 ndarray": b"\xc9" + _u32(len(_nd_payload((2,), "float32", bytes(range(8))))) + b"\x01"
                     + _nd_payload((2,), "float32", bytes(range(8))),
    "ext32 npscalar": b"\xc9" + _u32(len(_nd_payload((), "int16", b"\x01\x02"))) + b"\x03"
                      + _nd_payload((), "int16", b"\x01\x02"),
    "ext16 bf16": b"\xc8" + struct.pack(">H", len(_nd_payload((2,), "bfloat16", b"\x80\x3f\xc0\x7f"))) + b"\x01"
                  + _nd_payload((2,), "bfloat16", b"\x80\x3f\xc0\x7f"),
    "fixext1 unknown code": b"\xd4\x07\xab",
    "fixext2 unknown code": b"\xd5\x7f\xab\xcd",
    "fixext4 complex": b"\xd6\x02\x92\x01\xcc\x02",
    "fixext4 bytes ndarray": b"\xd6\x04\x92\x91\x00\x90",
    "fixext8 ndarray": b"\xd7\x01" + _nd_payload((), "u1", b"\x09"),
    "fixext8 npscalar": b"\xd7\x03" + _nd_payload((), "u1", b"\x09"),
    "fixext16 ndarray": b"\xd8\x01" + _nd_payload((1, 1, 1, 1, 1), "uint8", b"\x09"),
    "uint64 small": b"\xcf" + struct.pack(">Q", 5),
    "int64 small": b"\xd3" + struct.pack(">q", -5),
    "uint32 / int16 / int8 small": b"\x93\xce" + _u32(1) + b"\xd1\xff\xff\xd0\x05",
    "bin8 key and value": b"\x81\xc4\x01k\xc4\x02vv",
    "bin16 key and value": b"\x81\xc5\x00\x01k\xc5\x00\x02vv",
    "bin32 key and value": b"\x81\xc6" + _u32(1) + b"k\xc6" + _u32(2) + b"vv",
    "bin and str keys together": b"\x82\xc4\x01k\x01\xa1k\x02",
    "empty bin value": b"\x91\xc4\x00",
    "dtype name as bin": b"\xc7" + bytes([len(b"\x93\x91\x02\xc4\x04int8\xc4\x02\x01\x02")]) + b"\x01"
                         + b"\x93\x91\x02\xc4\x04int8\xc4\x02\x01\x02",
}
assert len(_nd_payload((), "u1", b"\x09")) == 8 and len(_nd_payload((1, 1, 1, 1, 1), "uint8", b"\x09")) == 16


@pytest.mark.parametrize("name", sorted(HAND_BUILT))
def test_decoders_agree_on_encodings_the_packer_never_chooses(name):
    enc = HAND_BUILT[name]
    assert walk_headers(enc)[1] == len(enc)  # the hand-built bytes are one whole object
    check_agreement(enc)


def test_hand_built_values():
    """A few of the hand-built encodings against values stated here (agreement alone would
    not notice both decoders being wrong in the same way)."""
    view = ingest.msgpack_deserialize_view
    assert view(HAND_BUILT["bin8 key and value"]) == {b"k": b"vv"}
    assert view(HAND_BUILT["bin and str keys together"]) == {b"k": 1, "k": 2}
    f = view(HAND_BUILT["float32"])
    assert f[0] == float(np.float32(1.1)) and np.isnan(f[1])
    a = view(HAND_BUILT["fixext16 ndarray"])
    assert a.shape == (1, 1, 1, 1, 1) and a.dtype == np.uint8 and a.item() == 9
    s = view(HAND_BUILT["fixext8 npscalar"])
    assert type(s) is np.uint8 and s == 9
    b = view(HAND_BUILT["ext16 bf16"])
    assert type(b) is BF16Array and np.asarray(b, np.uint16).tolist() == [0x3F80, 0x7FC0]
    assert view(HAND_BUILT["fixext4 complex"]) == complex(1, 2)
    assert view(HAND_BUILT["uint32 / int16 / int8 small"]) == [1, -1, 5]


# ---------------------------------------------------- the decided disagreements
def test_bin_keys_stay_bytes_and_bin_values_are_bytes_copies():
    payload = bytearray(msgpack.packb({b"k": 1, "s": b"value", "l": [b"", b"x" * 300]}, use_bin_type=True))
    out = ingest.msgpack_deserialize_view(payload)
    assert list(out) == [b"k", "s", "l"] and all(type(k) in (bytes, str) for k in out)
    assert type(out["s"]) is bytes and [type(v) for v in out["l"]] == [bytes, bytes]
    check_agreement(bytes(payload))
    payload[:] = b"\xff" * len(payload)  # the values are copies: releasing the payload leaves them whole
    assert out == {b"k": 1, "s": b"value", "l": [b"", b"x" * 300]}


@pytest.mark.parametrize("key", [1, -3, 2 ** 40, 1.5, None, True, [1], {"a": 1}, np.float32(1)])
def test_map_key_that_is_neither_str_nor_bytes_is_refused(key):
    if isinstance(key, (list, dict)):
        packed = msgpack.packb(key)
    else:
        packed = ingest.msgpack_serialize(key)
    enc = b"\x81" + packed + b"\x01"
    with pytest.raises(ValueError):
        ingest.msgpack_deserialize(enc)
    with pytest.raises(ValueError, match="map key"):
        ingest.msgpack_deserialize_view(enc)


# ------------------------------------------------------------- malformed input
def _refused(enc, what):
    """ValueError from the view decoder, with a message that names the problem."""
    with pytest.raises(ValueError) as e:
        ingest.msgpack_deserialize_view(enc)
    msg = str(e.value).lower()
    assert "truncated" in msg or "malformed" in msg, f"{what}: {e.value!r}"
    assert "trailing" not in msg, f"{what}: {e.value!r}"


def test_every_proper_prefix_of_a_small_payload_is_refused():
    enc = ingest.msgpack_serialize({"a": np.arange(5, dtype=np.float32), "s": "hello", "n": 7})
    check_agreement(enc)
    for cut in range(len(enc)):
        _refused(enc[:cut], f"prefix of {cut} bytes")
        _refused(memoryview(bytearray(enc))[:cut], f"prefix of {cut} bytes (memoryview)")


def test_cuts_of_a_large_payload_are_refused():
    enc = ingest.msgpack_serialize({"big": np.arange(70_000, dtype=np.float32), "s": "y" * 300, "n": 2 ** 40,
                                    "l": list(range(20)), "bf": BF16Array(np.arange(200, dtype=np.uint16))})
    check_agreement(enc)
    headers, end = walk_headers(enc)
    assert end == len(enc)
    assert {"ext32", "ext16", "bin32", "bin16", "str16", "array16", "fixmap", "fixarray", "fixstr"} <= {
        k for _, k, _ in headers}
    cuts = {0, 1, len(enc) - 1, len(enc) // 2}
    for off, _, size in headers:
        cuts.update(range(off, off + size + 1))  # before, inside (one short of each length field) and after
    data_start = next(off + size for off, k, size in headers if k == "bin32")
    cuts.update({data_start + 1, data_start + 4 * 35_000 + 1, data_start + 4 * 70_000 - 1})  # mid-data
    assert len(headers) >= 20 and len(cuts) >= 3 * len(headers)
    for cut in sorted(cuts):
        _refused(memoryview(enc)[:cut], f"cut at {cut}")


def _ext(code, payload):
    return b"\xc9" + _u32(len(payload)) + struct.pack(">b", code) + payload


MALFORMED = {
    "bin32 longer than the buffer": b"\xc6" + _u32(100) + b"abc",
    "bin8 longer than the buffer": b"\xc4\x05abc",
    "ext32 longer than the buffer": b"\xc9" + _u32(100) + b"\x01abc",
    "ext8 longer than the buffer": b"\xc7\x64\x01abc",
    "str32 longer than the buffer": b"\xdb" + _u32(100) + b"abc",
    "fixstr longer than the buffer": b"\xbfabc",
    "array32 longer than the buffer": b"\xdd" + _u32(2 ** 32 - 1) + b"\x01",
    "array32 one entry short": b"\xdd" + _u32(3) + b"\x01\x02",
    "map32 longer than the buffer": b"\xdf" + _u32(2 ** 31) + b"\xa1k\x01",
    "fixext16 cut": b"\xd8\x01" + b"\x00" * 15,
    "ndarray bytes short of its shape": _ext(1, _nd_payload((3,), "float32", bytes(8))),
    "ndarray bytes beyond its shape": _ext(1, _nd_payload((1,), "float32", bytes(8))),
    "ndarray bytes no multiple of the item size": _ext(1, _nd_payload((2,), "float32", bytes(7))),
    "bf16 bytes short of its shape": _ext(1, _nd_payload((3,), "bfloat16", bytes(4))),
    "npscalar with two elements": _ext(3, _nd_payload((), "int16", bytes(4))),
    "bytes after the triple": _ext(1, _nd_payload((2,), "float32", bytes(8)) + b"\x00"),
    "triple cut inside the ext": _ext(1, _nd_payload((2,), "float32", bytes(8))[:-1]),
    "a pair, not a triple": _ext(1, msgpack.packb(((2,), "float32"))),
    "not an array at all": _ext(1, b"\x01"),
    "unknown dtype": _ext(1, _nd_payload((2,), "float33", bytes(8))),
    "object dtype": _ext(1, _nd_payload((1,), "object", bytes(8))),
    "negative dimension": _ext(1, _nd_payload((-1,), "int8", b"")),
    "non-integer dimension": _ext(1, _nd_payload((1.0,), "int8", b"\x00")),
    "data as str": _ext(1, msgpack.packb(((1,), "int8", "a"))),
    "dtype name that is not UTF-8": _ext(1, b"\x93\x91\x01\xc4\x02\xff\xfe\xc4\x01\x00"),
    "str that is not UTF-8": b"\xa2\xff\xfe",
    "map key that is not UTF-8": b"\x81\xd9\x02\xc3\x28\x01",
    "complex ext holding a scalar": _ext(2, b"\x01"),
    "complex ext holding one number": _ext(2, b"\x91\x01"),
    "complex ext cut short": _ext(2, msgpack.packb((1.5, 2.5))[:-1]),
    "complex ext with bytes after it": _ext(2, msgpack.packb((1.5, 2.5)) + b"\x00"),
    "bytes ndarray short of its shape": _ext(4, msgpack.packb(((3,), [b"a"]), use_bin_type=True)),
    "bytes ndarray that is no pair": _ext(4, b"\x01"),
    "list nested 5000 deep": b"\x91" * 5000 + b"\x01",
    "map nested 5000 deep": b"\x81\xa1k" * 5000 + b"\x01",
    "never-used byte 0xc1": b"\xc1",
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_input_is_refused_with_value_error(name):
    _refused(MALFORMED[name], name)


def test_trailing_bytes_are_named_only_when_bytes_really_trail():
    enc = ingest.msgpack_serialize({"a": 1})
    with pytest.raises(ValueError, match="trailing"):
        ingest.msgpack_deserialize_view(enc + b"\x00")
    with pytest.raises(ValueError):
        ingest.msgpack_deserialize(enc + b"\x00")


def test_nesting_within_the_limit_decodes():
    enc = b"\x91" * 400 + b"\x01"
    v = check_agreement(enc)
    for _ in range(400):
        (v,) = v
    assert v == 1


# ------------------------------------------------------------------ serializer
def _bf16_tensor(bits):
    return torch.from_numpy(np.asarray(bits, np.uint16).view(np.int16).copy()).view(torch.bfloat16)


def test_host_tensors_serialize_as_their_numpy_equivalent():
    rng = np.random.RandomState(SEED)
    for dt in (np.float32, np.float64, np.int32):
        a = _array(rng, dt, (3, 4))
        assert ingest.msgpack_serialize({"x": torch.from_numpy(a.copy())}) == ingest.msgpack_serialize({"x": a})
        # a transposed view serializes as its C-order copy, a 0-d tensor as a 0-d array
        assert ingest.msgpack_serialize(torch.from_numpy(a.copy()).t()) == ingest.msgpack_serialize(
            np.ascontiguousarray(a.T))
        assert ingest.msgpack_serialize(torch.from_numpy(a.copy())[1, 2]) == ingest.msgpack_serialize(a[1, 2:3].reshape(()))
    bits = _array(rng, np.uint16, (3, 4))
    t = _bf16_tensor(bits)
    assert t.dtype == torch.bfloat16
    assert ingest.msgpack_serialize([t]) == ingest.msgpack_serialize([BF16Array(bits)])
    assert ingest.msgpack_serialize(t.t()) == ingest.msgpack_serialize(BF16Array(np.ascontiguousarray(bits.T)))
    assert ingest.msgpack_serialize(t[2, 3]) == ingest.msgpack_serialize(BF16Array(bits[2, 3:4].reshape(())))
    back = ingest.msgpack_deserialize_view(ingest.msgpack_serialize(t.t()))
    assert type(back) is BF16Array and np.array_equal(np.asarray(back, np.uint16), bits.T)


def test_strided_and_fortran_arrays_serialize_as_their_c_order_copy():
    rng = np.random.RandomState(SEED + 1)
    a = _array(rng, np.float32, (6, 8))
    for v in (np.asfortranarray(a), a.T, a[::2], a[:, ::3], a[::-1], BF16Array(_array(rng, np.uint16, (6, 8)))[::2, 1::2]):
        c = np.ascontiguousarray(v)
        assert not v.flags.c_contiguous and c.flags.c_contiguous
        c = BF16Array(c) if isinstance(v, BF16Array) else c
        enc = ingest.msgpack_serialize(v)
        assert enc == ingest.msgpack_serialize(c)
        back = check_agreement(enc)
        assert back.shape == v.shape and back.tobytes() == c.tobytes()


def test_tuples_are_refused_as_in_the_reference():
    """fedjax/core/serialization.py packs with strict_types=True: a tuple goes to the
    ``default`` hook, comes back unchanged, and msgpack raises TypeError."""
    for tree in ((1, 2), {"a": (np.zeros(2, np.float32),)}, [(), 1]):
        with pytest.raises(TypeError):
            ingest.msgpack_serialize(tree)
    assert "TypeError" in ingest.msgpack_serialize.__doc__ and "tuples become lists" not in ingest.msgpack_serialize.__doc__
