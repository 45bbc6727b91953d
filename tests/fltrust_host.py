"""FLTrust's selection rule (fedjax_amd/csrc/fjtrust_dev.h) built for the host as the stand-alone
program tests/fltrust_select_host.cpp, and run over cases: what the CPU tests compare with numpy and
the GPU tests compare the kernel with."""
import os
import shutil
import struct
import subprocess

import numpy as np

F32, F64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("cos", "trust", "factors", "norms", "server_norm", "total", "count", "order", "seg", "wperm", "gscale")


def _compiler():
    for name in ("c++", "g++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    return shutil.which("clang++", path="/opt/rocm/llvm/bin")


def build(directory, sanitize=False):
    """Compiles the program into ``directory`` and returns its path. ``sanitize``: with the address and
    undefined-behaviour sanitizers where the toolchain has their runtimes (the CPU suite's build; the
    GPU tests build it plain: -ffp-contract=off is what fixes the bits)."""
    cxx = _compiler()
    assert cxx is not None, "no C++ compiler"
    exe = os.path.join(str(directory), "fltrust_select_host")
    plain = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "fedjax_amd", "csrc"),
             os.path.join(ROOT, "tests", "fltrust_select_host.cpp"), "-o", exe]
    if sanitize:
        cmd = plain[:5] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + plain[5:]
        if subprocess.run(cmd, capture_output=True).returncode == 0:
            return exe
    subprocess.run(plain, check=True, capture_output=True)  # (also: a toolchain without the sanitizer runtimes)
    return exe


def _take(buf, at, dtype, n):
    size = np.dtype(dtype).itemsize * n
    return np.frombuffer(buf[at:at + size], dtype=dtype), at + size


def run(exe, cases, directory):
    """cases: (a [K] float32, q [K] float32, q_s). Returns per case a dict of FIELDS plus
    ``combined``, the ordered float32 sum of ``a``."""
    blob = [struct.pack("<i", len(cases))]
    for a, q, qs in cases:
        a, q = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(q, dtype=F32)
        blob += [struct.pack("<i", a.size), np.array([qs], dtype=F32).tobytes(), a.tobytes(), q.tobytes()]
    src, dst = os.path.join(str(directory), "cases.bin"), os.path.join(str(directory), "results.bin")
    with open(src, "wb") as f:
        f.write(b"".join(blob))
    done = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    with open(dst, "rb") as f:
        buf = f.read()
    at, out = 0, []
    for a, _, _ in cases:
        K = np.asarray(a).size
        r = {}
        r["cos"], at = _take(buf, at, F64, K)
        r["trust"], at = _take(buf, at, F64, K)
        r["factors"], at = _take(buf, at, F32, K)
        r["norms"], at = _take(buf, at, F32, K)
        for name, dt in (("server_norm", F32), ("total", F64), ("count", np.int32)):
            v, at = _take(buf, at, dt, 1)
            r[name] = v[0]
        r["order"], at = _take(buf, at, np.int32, K)
        r["seg"], at = _take(buf, at, np.int32, 2)
        r["wperm"], at = _take(buf, at, F32, K)
        for name in ("gscale", "combined"):
            v, at = _take(buf, at, F32, 1)
            r[name] = v[0]
        out.append(r)
    assert at == len(buf)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want, what=""):
    """Every field of FIELDS that both hold, bit for bit."""
    for name in FIELDS:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, name, g, w)


def seeded_rows(seed, K):
    """(a, q, q_s) of one seeded selection case: plausible sums with the specials mixed in — NaN and
    inf sums, zeros, a q that underflowed, exact multiples (cos at the clamp), negatives."""
    rng = np.random.RandomState(seed)
    q = (rng.uniform(0.1, 4.0, K) ** 2).astype(F32)
    qs = F32(rng.uniform(0.1, 4.0) ** 2)
    cos = rng.uniform(-1.0, 1.0, K)
    a = (cos * np.sqrt(q.astype(F64) * F64(qs))).astype(F32)
    special = rng.randint(0, 12, K)
    with np.errstate(all="ignore"):
        a = np.where(special == 0, F32(np.nan), a)
        q = np.where(special == 1, F32(np.inf), q)
        a = np.where(special == 2, F32(np.inf), a)
        q = np.where(special == 2, F32(np.inf), q)
        a = np.where(special == 3, F32(0), a)
        q = np.where(special == 3, F32(0), q)
        q = np.where(special == 4, F32(0), q)                      # q underflowed, a did not: c = inf
        a = np.where(special == 5, np.sqrt(q.astype(F64) * F64(qs)).astype(F32) * F32(1 + 2.0 ** -22), a)  # cos > 1
        q = np.where(special == 6, F32(1e-45), q)                  # a denormal q
        q = np.where(special == 7, F32(3e38), q)                   # a huge client: c tiny
    if seed % 10 == 7:
        qs = F32(0)
    if seed % 10 == 8:
        qs = F32(np.inf)
    if seed % 10 == 9:
        qs = F32(np.nan)
    return a.astype(F32), q.astype(F32), qs
