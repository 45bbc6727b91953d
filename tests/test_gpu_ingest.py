"""DeltaIngestor on the GPU: the ring of pinned staging rows and its three stream orderings
(per-slot events, the copy stream's wait for earlier readers of the slab, ``ready()``), the
payload's lifetime, rows and padding, every host dtype end to end, failures, and degenerate
templates. Every comparison is bit for bit against the host arrays; no tolerance anywhere.

The races are made deterministic with ``torch.cuda._sleep(SLEEP_CYCLES)`` on the stream the
hazard waits behind. Each test that relies on a sleep records an event after it and asserts
``not event.query()`` at the point where the hazard would occur: if that assertion fails the
sleep was too short for the machine (lengthen it; the assertion stays)."""
import numpy as np
import pytest
import torch

import fedjax_amd
from fedjax_amd import ingest, kernels, tree_util as tu
from fedjax_amd.ingest import BF16Array
from oracle import tree_util_ref as ref
from tests import ingest_cases as ic

pytestmark = pytest.mark.gpu

P = 1001  # row stride 1004: the padding is visible
# torch.cuda._sleep(50_000_000) lasts some 20 ms on MI355X, less than a first put or a first
# mean in a fresh process takes on the host (the pending-event assertions of slot reuse and of
# the next round failed with it): four times that, behind a warm-up of everything lazy
SLEEP_CYCLES = 200_000_000
SENTINEL = 0x7FC0DEAD  # a NaN pattern no delta below holds


@pytest.fixture(scope="module", autouse=True)
def warm(cuda):
    """One put, ``ready()`` and mean before any timed window: stream and pinned-memory set-up,
    lazily loaded kernels and compiled pytree accessors are paid for here."""
    slab = fedjax_amd.ClientDeltaSlab(_template(), 2, device=cuda)
    ing = ingest.DeltaIngestor(slab, depth=2)
    row = np.zeros(P, np.float32)
    ing.put(0, _delta(row))
    ing.put(1, ingest.msgpack_serialize(_delta(row)))
    ing.ready()
    slab.mean([1, 2])
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()


def _template():
    return {"a": np.zeros((7, 11), np.float32), "b": np.zeros(P - 77, np.float32)}


def _delta(row):
    return {"a": row[:77].reshape(7, 11), "b": row[77:]}


def _rows(K, seed):
    return np.random.RandomState(seed).standard_normal((K, P)).astype(np.float32)


def _slab(cuda, K, template=None, dtype=torch.float32, sentinel=True):
    slab = fedjax_amd.ClientDeltaSlab(_template() if template is None else template, K, dtype=dtype, device=cuda)
    if sentinel:
        _fill_sentinel(slab)
    torch.cuda.synchronize()
    return slab


def _fill_sentinel(slab):
    if slab.dtype == torch.float32:
        slab.storage.view(torch.int32).fill_(SENTINEL)
    else:
        slab.storage.view(torch.int16).fill_(SENTINEL >> 16)


def _bits(slab):
    """The whole storage, padding included, as unsigned bit patterns on the host."""
    if slab.dtype == torch.float32:
        return slab.storage.view(torch.int32).cpu().numpy().view(np.uint32)
    return slab.storage.view(torch.int16).cpu().numpy().view(np.uint16)


def _expect(slab, rows):
    """Storage bits with ``rows`` ({k: flat host row}) in place and the sentinel elsewhere."""
    f32 = slab.dtype == torch.float32
    want = np.full((slab.num_clients, slab.row_stride), SENTINEL if f32 else SENTINEL >> 16,
                   np.uint32 if f32 else np.uint16)
    for k, row in rows.items():
        want[k, : slab.num_params] = np.asarray(row).view(want.dtype)
    return want


def _sleep_then_event():
    """Keep the current stream busy; the event stays pending until the sleep is over."""
    torch.cuda._sleep(SLEEP_CYCLES)
    ev = torch.cuda.Event()
    ev.record()
    return ev


def _flat_mean(m):
    return np.concatenate([m["a"].cpu().numpy().ravel(), m["b"].cpu().numpy().ravel()])


def _oracle_mean(coracle, x, wi):
    return coracle.wsum_f32(x, np.float32(wi), scale=ref.mean_scale(wi))


def _weights(K, seed):
    return [int(v) for v in ref.fedavg_weights(K, seed=seed)]


# ------------------------------------------------------------------ C1 slot reuse
@pytest.mark.parametrize("depth", [1, 2, 3, 8])
def test_slot_reuse_waits_for_the_slots_last_copy(cuda, depth):
    """K = 3 * depth + 1 puts while the copy stream is held behind a sleep: the first
    ``depth`` puts fill the ring without one DMA having run, and put ``depth + 1`` restages
    slot 0, so it must block on that slot's event (returning only once the sleep is over).
    Without the wait the rows would hold later clients' data."""
    K = 3 * depth + 1
    x = _rows(K, seed=depth)
    slab = _slab(cuda, K)
    ing = ingest.DeltaIngestor(slab, depth=depth)
    assert len(ing.staging) == depth
    ev = _sleep_then_event()
    for k in range(depth):
        ing.put(k, _delta(x[k]) if k % 2 else ingest.msgpack_serialize(_delta(x[k])))
    assert not ev.query()  # nothing has been copied yet: every slot is still waiting for its DMA
    ing.put(depth, _delta(x[depth]))
    assert ev.query()  # the put blocked on slot 0's event, which completes only after the sleep
    for k in range(depth + 1, K):
        ing.put(k, _delta(x[k]) if k % 2 else ingest.msgpack_serialize(_delta(x[k])))
    assert ing.n == K
    ing.ready()
    assert np.array_equal(_bits(slab), _expect(slab, dict(enumerate(x))))


# -------------------------------------------- C2 write-after-read across rounds
def test_next_round_waits_for_the_fold_of_the_previous_one(cuda, coracle):
    """Round 2 is put into the same rows while round 1's mean is still queued behind a sleep:
    the copy stream must wait for that reader, so the mean sees round 1 only."""
    K = 12
    x1, x2 = _rows(K, seed=21), _rows(K, seed=22)
    wi = _weights(K, seed=23)
    slab = _slab(cuda, K)
    ing = ingest.DeltaIngestor(slab, depth=K)  # no put blocks on a slot: the host runs ahead of the GPU
    for k in range(K):
        ing.put(k, _delta(x1[k]))
    ing.ready()
    ev = _sleep_then_event()
    m1 = slab.mean(wi)
    ing.put(0, _delta(x2[0]))
    assert not ev.query()  # the mean of round 1 has not started; the copy is queued behind it
    for k in range(1, K):
        ing.put(k, ingest.msgpack_serialize(_delta(x2[k])))
    assert not ev.query()
    ing.ready()
    m2 = slab.mean(wi)
    got1, got2 = _flat_mean(m1), _flat_mean(m2)
    assert np.array_equal(got1.view(np.uint32), _oracle_mean(coracle, x1, wi).view(np.uint32))
    assert np.array_equal(got2.view(np.uint32), _oracle_mean(coracle, x2, wi).view(np.uint32))
    assert np.array_equal(_bits(slab), _expect(slab, dict(enumerate(x2))))


# ------------------------------------------- C3 read-after-write through ready()
def _ready_orders_the_fold(cuda, coracle, seed):
    """On the current stream: sleep, 40 puts, ``ready()``, the mean, no host synchronisation in
    between. The copy stream is given a second sleep behind the first, so a fold that did not
    wait for the copies would run some 50 ms ahead of them and read the sentinel."""
    K = 40
    x = _rows(K, seed=seed)
    wi = _weights(K, seed=seed + 1)
    slab = _slab(cuda, K)
    ing = ingest.DeltaIngestor(slab, depth=K)
    ev = _sleep_then_event()
    ing.stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(ing.stream):
        torch.cuda._sleep(SLEEP_CYCLES)
    for k in range(K):
        ing.put(k, ingest.msgpack_serialize(_delta(x[k])) if k % 2 else _delta(x[k]))
    ing.ready()
    m = slab.mean(wi)
    assert not ev.query()  # the fold was enqueued before a single copy had run
    got = _flat_mean(m)
    assert np.array_equal(got.view(np.uint32), _oracle_mean(coracle, x, wi).view(np.uint32))
    assert np.array_equal(_bits(slab), _expect(slab, dict(enumerate(x))))


def test_ready_orders_the_fold_after_the_copies(cuda, coracle):
    _ready_orders_the_fold(cuda, coracle, seed=31)


def test_ready_orders_the_fold_after_the_copies_on_a_side_stream(cuda, coracle):
    """The puts, ``ready()`` and the mean all on a non-default stream."""
    side = torch.cuda.Stream(cuda)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _ready_orders_the_fold(cuda, coracle, seed=33)
        side.synchronize()
    torch.cuda.synchronize()


# ------------------------------------------------------------ C4 payload lifetime
def test_payload_and_leaves_may_be_released_once_put_returns(cuda):
    """Staging is synchronous on the host: with nothing copied to the device yet, the
    payload is overwritten and a numpy leaf mutated, and the rows still get the original
    values."""
    x = _rows(3, seed=41)
    slab = _slab(cuda, 3)
    ing = ingest.DeltaIngestor(slab, depth=3)
    ev = _sleep_then_event()
    payload = bytearray(ingest.msgpack_serialize(_delta(x[0])))
    ing.put(0, payload)
    payload[:] = b"\xff" * len(payload)
    view_payload = bytearray(ingest.msgpack_serialize(_delta(x[1])))
    ing.put(1, memoryview(view_payload))
    view_payload[:] = bytes(len(view_payload))
    leaves = _delta(x[2].copy())
    ing.put(2, leaves)
    leaves["a"].fill(np.nan)
    leaves["b"][:] = -1.0
    del payload, view_payload, leaves
    assert not ev.query()  # all of that happened before the first byte reached the device
    ing.ready()
    assert np.array_equal(_bits(slab), _expect(slab, dict(enumerate(x))))


# ------------------------------------------------------- C5 rows, padding, order
def test_rows_padding_and_order(cuda):
    K = 11
    x = _rows(K + 1, seed=51)
    slab = _slab(cuda, K)
    assert slab.row_stride == 1004 and slab.num_params == P
    ing = ingest.DeltaIngestor(slab, depth=3)
    left_out = {2, 7, 10}
    order = [k for k in np.random.RandomState(52).permutation(K).tolist() if k not in left_out]
    twice = order[1]
    ing.put(twice, _delta(x[K]))  # put again below: the last one wins
    for k in order:
        ing.put(k, ingest.msgpack_serialize(_delta(x[k])) if k % 3 == 0 else _delta(x[k]))
    ing.ready()
    want = _expect(slab, {k: x[k] for k in order})
    got = _bits(slab)
    assert np.array_equal(got[:, P:], want[:, P:])  # the padding keeps the sentinel
    assert np.array_equal(got[sorted(left_out)], want[sorted(left_out)])  # rows left out, too
    assert np.array_equal(got, want)


# ---------------------------------------------------------- C6 dtype end to end
def _set_client_leaf(leaf):
    """The same host values as ``leaf`` in a container ``slab.set_client`` takes."""
    if isinstance(leaf, BF16Array):
        a = np.ascontiguousarray(np.asarray(leaf, np.uint16))
        return torch.from_numpy(a.view(np.int16)).view(torch.bfloat16).reshape(leaf.shape)
    if isinstance(leaf, (np.bool_, np.ndarray)) and np.asarray(leaf).dtype == np.bool_:
        return np.asarray(leaf).astype(np.float32)
    return leaf


@pytest.mark.parametrize("slab_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_every_host_dtype_end_to_end(cuda, slab_dtype):
    """The host-conversion matrix of tests/ingest_cases through ``put``, as a pytree and as
    msgpack bytes / bytearray / memoryview: the slab holds the bits of the reference worked
    out there. ``slab.set_client`` of the same deltas gives the same rows (its conversion is
    torch's: every NaN counts as one pattern)."""
    cases = ic.leaf_cases()
    slab = _slab(cuda, 5, template=ic.template_of(cases), dtype=slab_dtype)
    want_row = np.concatenate([ic.expected_bytes(cases[k], slab_dtype) for k in sorted(cases)])
    want_row = want_row.view(np.uint32 if slab_dtype == torch.float32 else np.uint16)
    assert want_row.size == slab.num_params
    enc = ingest.msgpack_serialize(cases)
    ing = ingest.DeltaIngestor(slab, depth=2)
    ing.put(0, cases)
    ing.put(1, enc)
    ing.put(2, bytearray(enc))
    ing.put(3, memoryview(enc))
    ing.ready()
    slab.set_client(4, {k: _set_client_leaf(v) for k, v in cases.items()})
    got = _bits(slab)
    for k in range(4):
        assert np.array_equal(got[k, : slab.num_params], want_row), f"row {k}"
    assert np.all(got[:, slab.num_params:] == (SENTINEL if slab_dtype == torch.float32 else SENTINEL >> 16))
    if slab_dtype == torch.float32:
        nan = np.isnan(want_row.view(np.float32))
        assert np.all(np.isnan(got[4, : slab.num_params].view(np.float32)[nan]))
    else:
        nan = (want_row & 0x7FFF) > 0x7F80
        assert np.all((got[4, : slab.num_params][nan] & 0x7FFF) > 0x7F80)
    assert np.array_equal(got[4, : slab.num_params][~nan], want_row[~nan])


def test_bf16_put_is_the_devices_own_conversion(cuda):
    """float32 data put into a bfloat16 slab against the device's conversion of the same data
    (a K = 1 fold, weight 1, no scale, bfloat16 output, of a float32 copy), NaNs included bit
    for bit: both keep the sign and set the quiet bit. numpy and host torch leaves alike."""
    grid = (np.arange(65536, dtype=np.uint32)[:, None] << np.uint32(16)
            | np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], np.uint32)[None, :]).reshape(-1)
    a = np.concatenate([grid[::5], ic.F32_BITS]).view(np.float32)
    n = a.size
    slab = _slab(cuda, 3, template={"x": np.zeros(n, np.float32)}, dtype=torch.bfloat16)
    ing = ingest.DeltaIngestor(slab, depth=2)
    ing.put(0, {"x": a})
    ing.put(1, {"x": torch.from_numpy(a.copy())})
    ing.put(2, ingest.msgpack_serialize({"x": torch.from_numpy(a.copy())}))
    ing.ready()
    x_dev = torch.from_numpy(a.copy()).to(cuda).reshape(1, n)
    assert np.array_equal(x_dev.view(torch.int32).cpu().numpy().view(np.uint32).ravel(), a.view(np.uint32))
    y = kernels.weighted_sum_dense(x_dev, np.ones(1, np.float32), out_dtype=torch.bfloat16)
    assert y.dtype == torch.bfloat16
    dev_bits = y.view(torch.int16).cpu().numpy().view(np.uint16)
    got = _bits(slab)
    for k in range(3):
        bad = np.flatnonzero(got[k, :n] != dev_bits)
        assert bad.size == 0, (k, [(hex(a.view(np.uint32)[i]), hex(got[k, i]), hex(dev_bits[i])) for i in bad[:5]])
    assert np.array_equal(dev_bits, ic.ref_bf16_bits(a.view(np.uint32)))


def test_bf16_ingest_then_mean_in_reference_mode(cuda, coracle):
    """One bfloat16 round from the host through the ring into ``slab.mean`` under the
    reference's bfloat16 arithmetic, against the C oracle's restatement of it."""
    K, n = 20, 3000
    xb = coracle.synth_bf16(K, n, seed=61)
    wi = _weights(K, seed=62)
    W = 0.0
    for w in wi:
        W += w
    template = {"a": np.zeros(1000, np.float32), "b": [np.zeros((10, 100), np.float32), np.zeros(1000, np.float32)]}
    slab = _slab(cuda, K, template=template, dtype=torch.bfloat16, sentinel=False)
    ing = ingest.DeltaIngestor(slab, depth=3)
    for k in range(K):
        row = BF16Array(xb[k])
        d = {"a": row[:1000], "b": [row[1000:2000].reshape(10, 100), row[2000:]]}
        if k % 3 == 1:
            d = ingest.msgpack_serialize(d)
        elif k % 3 == 2:  # the same values as float32: exact in bfloat16
            d = {"a": ic.widen(xb[k, :1000]), "b": [torch.from_numpy(ic.widen(xb[k, 1000:2000]).reshape(10, 100)),
                                                     ic.widen(xb[k, 2000:]).astype(np.float64)]}
        ing.put(k, d)
    ing.ready()
    tu.set_bf16_semantics("reference")
    try:
        m = slab.mean(wi)
    finally:
        tu.set_bf16_semantics("f32")
    leaves = [m["a"], m["b"][0], m["b"][1]]
    assert all(x.dtype == torch.bfloat16 for x in leaves)
    got = np.concatenate([x.reshape(-1).view(torch.int16).cpu().numpy().view(np.uint16) for x in leaves])
    want = coracle.wsum_bf16_refsem(xb, np.float32(wi), np.float32(1.0 / W))
    assert np.array_equal(got, want)
    assert np.array_equal(_bits(slab)[:, :n], xb)


# -------------------------------------------- C7 failures leave the ingestor usable
def test_failures_leave_the_ingestor_usable(cuda):
    K = 12  # three rows, then a good put after each of the nine failures
    x = _rows(K, seed=71)
    slab = _slab(cuda, K)
    ing = ingest.DeltaIngestor(slab, depth=2)
    threads = torch.get_num_threads()
    good = ingest.msgpack_serialize(_delta(x[3]))
    failures = [
        ("a leaf of the wrong size", 3, {"a": x[3, :77].reshape(7, 11), "b": x[3, 77:-1]}, ValueError),
        ("a wrong size inside a payload", 3, ingest.msgpack_serialize({"a": x[3, :77], "b": x[3, 76:]}), ValueError),
        ("a missing key", 3, {"a": x[3, :77]}, ValueError),
        ("an extra key", 3, dict(_delta(x[3]), c=x[3, :1]), ValueError),
        ("a device-tensor leaf", 3, {"a": x[3, :77], "b": torch.zeros(P - 77, device=cuda)}, ValueError),
        ("k past the last row", K, _delta(x[3]), IndexError),
        ("a negative k", -1, _delta(x[3]), IndexError),
        ("a truncated payload", 3, good[:-5], ValueError),
        ("a payload cut inside its header", 3, good[:3], ValueError),
    ]
    done = {}
    for k in range(3):
        ing.put(k, _delta(x[k]))
        done[k] = x[k]
    for what, k, delta, exc in failures:
        n = ing.n
        with pytest.raises(exc):
            ing.put(k, delta)
        assert ing.n == n, what
        assert torch.get_num_threads() == threads, what
        ing.ready()
        assert np.array_equal(_bits(slab), _expect(slab, done)), what  # row k and its neighbours are unchanged
        # the round goes on, through the slot the failed put was staging into
        nxt = len(done)
        if nxt < K:
            ing.put(nxt, _delta(x[nxt]) if nxt % 2 else ingest.msgpack_serialize(_delta(x[nxt])))
            done[nxt] = x[nxt]
    assert len(done) == K and ing.n == K
    ing.ready()
    assert np.array_equal(_bits(slab), _expect(slab, done))
    assert torch.get_num_threads() == threads


# ------------------------------------------------------ C8 degenerate templates
def test_template_without_parameters(cuda):
    K = 3
    template = {"a": np.zeros(0, np.float32), "b": np.zeros((0, 3), np.float32)}
    slab = _slab(cuda, K, template=template)
    assert slab.num_params == 0
    ing = ingest.DeltaIngestor(slab)
    ing.put(0, {"a": np.zeros(0, np.float32), "b": np.zeros((0, 3), np.float64)})
    ing.put(1, ingest.msgpack_serialize({"a": np.zeros(0, np.float32), "b": np.zeros((0, 3), np.float32)}))
    ing.put(2, {"a": torch.zeros(0), "b": BF16Array(np.zeros((0, 3), np.uint16))})
    ing.ready()
    m = slab.mean([1, 2, 3])
    assert tuple(m["a"].shape) == (0,) and tuple(m["b"].shape) == (0, 3)
    assert np.array_equal(_bits(slab), _expect(slab, {}))  # nothing was written


@pytest.mark.parametrize("slab_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_single_parameter_row(cuda, slab_dtype):
    """One element per row in a 16-byte row stride."""
    K = 5
    slab = _slab(cuda, K, template={"a": np.zeros(1, np.float32)}, dtype=slab_dtype)
    assert slab.row_stride * slab.storage.element_size() == 16
    vals = np.array([1.5, -2.0, 3.25, -0.0, 1e-3], np.float32)
    ing = ingest.DeltaIngestor(slab, depth=2)
    for k in range(K):
        d = {"a": vals[k:k + 1]}
        ing.put(k, ingest.msgpack_serialize(d) if k % 2 else d)
    ing.ready()
    rows = {k: vals[k:k + 1] if slab_dtype == torch.float32 else ic.ref_bf16_bits(vals[k:k + 1].view(np.uint32))
            for k in range(K)}
    assert np.array_equal(_bits(slab), _expect(slab, rows))


def test_template_of_scalar_leaves(cuda):
    K = 4
    template = {"a": np.float32(0), "b": np.zeros((), np.float32), "c": [np.float32(0), np.zeros((), np.float32)]}
    slab = _slab(cuda, K, template=template)
    assert slab.num_params == 4
    x = np.random.RandomState(81).standard_normal((K, 4)).astype(np.float32)
    ing = ingest.DeltaIngestor(slab, depth=2)
    ing.put(0, {"a": x[0, 0], "b": np.array(x[0, 1]), "c": [x[0, 2], np.float64(x[0, 3])]})
    ing.put(1, ingest.msgpack_serialize({"a": x[1, 0], "b": np.array(x[1, 1]), "c": [x[1, 2], x[1, 3]]}))
    ing.put(2, {"a": float(x[2, 0]), "b": torch.tensor(x[2, 1]), "c": [x[2, 2:3].reshape(()), x[2, 3]]})
    ing.put(3, ingest.msgpack_serialize({"a": float(x[3, 0]), "b": x[3, 1], "c": [x[3, 2], np.array(x[3, 3])]}))
    ing.ready()
    assert np.array_equal(_bits(slab), _expect(slab, dict(enumerate(x))))


@pytest.mark.parametrize("slab_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_three_hundred_small_leaves(cuda, slab_dtype):
    """300 leaves of 1 to 7 elements: the staging offsets fall on every element alignment."""
    K = 4
    rng = np.random.RandomState(91)
    sizes = rng.randint(1, 8, size=300)
    assert set(sizes.tolist()) == set(range(1, 8))
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    elem = 4 if slab_dtype == torch.float32 else 2
    assert {int(o) * elem % 16 for o in offsets[:-1]} == set(range(0, 16, elem))
    template = [np.zeros(int(s), np.float32) for s in sizes]
    slab = _slab(cuda, K, template=template, dtype=slab_dtype)
    n = int(offsets[-1])
    assert slab.num_params == n
    x = rng.standard_normal((K, n)).astype(np.float32)
    ing = ingest.DeltaIngestor(slab, depth=2)
    for k in range(K):
        d = [x[k, offsets[j]:offsets[j + 1]] for j in range(300)]
        ing.put(k, ingest.msgpack_serialize(d) if k % 2 else d)
    ing.ready()
    rows = {k: x[k] if slab_dtype == torch.float32 else ic.ref_bf16_bits(x[k].view(np.uint32)) for k in range(K)}
    assert np.array_equal(_bits(slab), _expect(slab, rows))
