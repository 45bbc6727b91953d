"""pack_codes / unpack_codes: the round trip, and the documented bit positions."""
import numpy as np
import pytest
import torch

from fedjax_amd.aggregators import compression as comp


@pytest.mark.parametrize("n", [0, 1, 8, 16, 17, 1027])  # whole bytes, and a partial last byte for every bits
@pytest.mark.parametrize("bits", [1, 2, 4])
def test_unpack_inverts_pack(bits, n):
    c = torch.from_numpy(np.random.RandomState(n + bits).randint(0, 1 << bits, n).astype(np.uint8))
    packed = comp.pack_codes(c, bits)
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == ((n * bits + 7) // 8,)
    assert torch.equal(comp.unpack_codes(packed, n, bits), c)


def test_documented_bit_positions():
    # element i: byte i // (8 // bits), bit offset bits * (i % (8 // bits)), low bits first, padding zero
    c4 = torch.tensor([0x1, 0x2, 0xF, 0x0, 0x7], dtype=torch.uint8)
    assert comp.pack_codes(c4, 4).tolist() == [0x21, 0x0F, 0x07]
    c2 = torch.tensor([1, 2, 3, 0, 0, 0, 0, 3, 2], dtype=torch.uint8)
    assert comp.pack_codes(c2, 2).tolist() == [0b00111001, 0b11000000, 0b00000010]
    c1 = torch.tensor([1, 0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1], dtype=torch.uint8)
    assert comp.pack_codes(c1, 1).tolist() == [0x81, 0x06, 0x01]
    assert comp.unpack_codes(torch.tensor([0x21, 0x0F, 0xF7], dtype=torch.uint8), 5, 4).tolist() == c4.tolist()
