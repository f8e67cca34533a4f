"""The dual-use LDS image of a key tile's high fp16 plane (csrc/kv_share_layout.hpp), no GPU: tests/abi_cpp/kv_share_layout_host.cpp as a
program of its own under the host sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kv_share_layout_under_sanitizers(tmp_path):
    """Built with the host compiler and -fsanitize=address,undefined.  The program writes a 32-key x 128-channel tile of distinct values
    through off(), emulates the row reads of S = K Q'^T and the transposed reads of O^T += V^T P^T lane for lane, and holds every lane
    of every fragment to the fragment-major K and V images; off() must be a bijection on the 8 KiB, every address aligned and equal to
    one of two bases plus the kernel's immediate, and neither kind of read may touch a bank twice within a lane group.  A transposed
    read that is addressed wrongly returns wrong data without a fault on the device: this is the guard against it."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "kv_share_layout_host")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "abi_cpp", "kv_share_layout_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    got = run.stdout.splitlines()
    assert run.returncode == 0 and got and got[-1] == "kv_share_layout_host: ok", (run.stdout[-2000:] + run.stderr[-2000:])
    assert got[-2] == "row reads: 8, extra LDS cycles 0; transposed reads: 16, extra LDS cycles 0"
