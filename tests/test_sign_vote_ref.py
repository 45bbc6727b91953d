"""signSGD with majority vote without a GPU: the two new symbols, the host-side refusals of both C
entries (each returns before any HIP call) and the Python-side checks, which raise before the
library is touched."""
import os

import numpy as np
import pytest
import torch

from fedjax_amd import _compress as C
from fedjax_amd import _lib, aggregators
from fedjax_amd.aggregators import compression as comp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_symbols_and_header_constants():
    hdr = open(os.path.join(ROOT, "include", "fjcomp.h")).read()
    for sym in ("fjcomp_sign_pack", "fjcomp_sign_vote"):
        assert sym in _lib.SYMBOLS and f"int {sym}(" in hdr
    for name in ("SignDelta", "sign_encode_pytree", "majority_vote_aggregator"):
        assert name in comp.__all__ and getattr(aggregators, name) is getattr(comp, name)
    for name in ("VOTE_SIGN", "VOTE_MEAN", "VOTE_TILE", "VOTE_MAX_CLIENTS", "SIGN_PACK_BLOCK"):
        assert f"#define FJCOMP_{name} {getattr(_lib, name)}\n" in hdr
    assert "#define FJCOMP_ABI_VERSION 1" in hdr


def test_c_entries_refuse_on_the_host():
    lib = _lib.load()
    err = lambda: lib.fjagg_last_error().decode()
    vote = lambda K, L=1, mode=0, nblocks=1, tab=16, out=16: lib.fjcomp_sign_vote(tab, K, L, tab, tab, nblocks, mode,
                                                                                 1.0, out, None)
    assert vote(0) == -1 and "K must be" in err()
    assert vote(4097) == -3 and "4096" in err()
    assert vote(3, L=0) == -1 and "L must be" in err()
    assert vote(3, mode=2) == -1 and "mode" in err()
    assert vote(3, mode=-1) == -1 and "mode" in err()
    assert vote(3, nblocks=-1) == -1 and "nblocks" in err()
    assert vote(3, tab=None) == -1 and "null" in err()
    assert vote(3, out=None) == -1 and "null" in err()
    assert vote(3, nblocks=0) == 0  # nothing to launch
    pack = lambda R, nblocks=1, tab=16, out=16: lib.fjcomp_sign_pack(tab, R, tab, tab, nblocks, out, None)
    assert pack(0) == -1 and "R must be" in err()
    assert pack(2, nblocks=-1) == -1 and "nblocks" in err()
    assert pack(2, tab=None) == -1 and "null" in err()
    assert pack(2, out=None) == -1 and "null" in err()
    assert pack(2, nblocks=0) == 0


def test_python_checks_raise_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "call", lambda *a, **k: pytest.fail("the library was called"))
    with pytest.raises(ValueError, match="'sign' or 'mean'"):
        comp.majority_vote_aggregator("median")
    agg = comp.majority_vote_aggregator("mean", template={"a": np.zeros((3, 5), np.float32)})
    state = agg.init()
    assert isinstance(state, comp.CompressionState) and state.num_bits == 0.0 and state.rng is None
    assert agg.apply([], state) == (None, state)  # an empty round
    good = comp.SignDelta({"a": torch.zeros(2, dtype=torch.uint8)}, ((3, 5),))
    cases = [(torch.zeros(2, dtype=torch.uint8), TypeError, "SignDelta"),
             (comp.SignDelta({"a": torch.zeros(2, dtype=torch.int8)}, ((3, 5),)), TypeError, "uint8"),
             (comp.SignDelta({"a": torch.zeros(3, dtype=torch.uint8)}, ((3, 5),)), ValueError, r"expected \(2,\)"),
             (comp.SignDelta({"a": torch.zeros(1, 2, dtype=torch.uint8)}, ((3, 5),)), ValueError, r"expected \(2,\)"),
             (comp.SignDelta({"a": torch.zeros(2, dtype=torch.uint8)}, ((5, 3),)), ValueError, "leaf shapes"),
             (comp.SignDelta({"b": torch.zeros(2, dtype=torch.uint8)}, ((3, 5),)), Exception, None)]
    for bad, kind, word in cases:
        with pytest.raises(kind, match=word):
            agg.apply([(0, good, 1.0), (1, bad, 1.0)], state)
    with pytest.raises(ValueError, match="1 <= K <= 4096"):
        agg.apply([(k, good, 1.0) for k in range(4097)], state)
    with pytest.raises(ValueError, match="1 <= K <= 4096"):
        C.check_vote_clients(0)
