"""Inputs shared by the selection kernel's tests."""
import numpy as np


def trims(K):
    return sorted({t for t in (0, 1, (K - 1) // 2) if 0 <= 2 * t < K})  # (K-1)//2 is the largest valid t


def families(K, P, seed=0):
    """float32 [K, P]: all clients equal (every cut is a tie cut); keys that differ in their lowest 3 bits only
    (the descent must reach its last step); keys 0 and 0xFFFFFFFF, 1 + p % 4 of each in column p (t = 1 keeps one)."""
    rng = np.random.RandomState(31 * K + P + seed)
    equal = np.repeat(rng.standard_normal((1, P)).astype(np.float32), K, axis=0)
    low3 = (np.uint32(0x3F800000) | rng.randint(0, 8, (K, P)).astype(np.uint32)).view(np.float32)
    ends = rng.standard_normal((K, P)).astype(np.float32).view(np.uint32)
    for p in range(P):
        n = min(1 + p % 4, K // 2)
        rows = rng.permutation(K)[:2 * n]
        ends[rows[:n], p] = 0xFFFFFFFF  # key 0x00000000: the -NaN with every payload bit set
        ends[rows[n:], p] = 0x7FFFFFFF  # key 0xFFFFFFFF
    return {"equal": equal, "low3": low3, "ends": ends.view(np.float32)}
