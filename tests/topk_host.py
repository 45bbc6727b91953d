"""The host build of the top-k select rules (tests/topk_select_host.cpp over
fedjax_amd/csrc/fjsparse_dev.h), shared by tests/test_topk_ref.py and tests/test_topk_cases.py:
how it is compiled (under the address and undefined-behaviour sanitizers where the toolchain
has them) and how cases go in and results come out."""
import os
import shutil
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compiler():
    for name in ("c++", "g++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    return shutil.which("clang++", path="/opt/rocm/llvm/bin")


def build_host_program(cxx, directory, source=None):
    """Compile the stand-alone host program into `directory`; returns the executable's path."""
    exe = os.path.join(str(directory), "topk_select_host")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "fedjax_amd", "csrc"), source or os.path.join(ROOT, "tests", "topk_select_host.cpp"),
           "-o", exe]
    if subprocess.run(cmd, capture_output=True).returncode != 0:  # a toolchain without the sanitizer runtimes
        cmd = [c for c in cmd if "sanitize" not in c]
        subprocess.run(cmd, check=True, capture_output=True)
    return exe


def run_host(exe, cases, tmp_path):
    """cases: (row float32 or uint32 [P], c). Returns per case (T, sent, trace[6]): the trace is
    (digit, rank left inside the picked bin) per level."""
    blob = [struct.pack("<i", len(cases))]
    for row, c in cases:
        b = np.ascontiguousarray(row).view(np.uint32).ravel()
        blob += [struct.pack("<2i", b.size, c), b.tobytes()]
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(b"".join(blob))
    done = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    out = np.frombuffer(dst.read_bytes(), dtype=np.uint32).reshape(len(cases), 8)
    return [(int(r[0]), int(r[1].view(np.int32)), r[2:].tolist()) for r in out]
