"""The host plan of an encoder forward and the knob table (csrc/encoder_plan.hpp), no GPU: tests/abi_cpp/encoder_plan_host.cpp as a
program of its own under the host sanitizers, its table of plans held to tests/golden/encoder_plan_table.txt."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_encoder_plan_and_knob_table_under_sanitizers(tmp_path):
    """Built with the host compiler and -fsanitize=address,undefined.  The program prints one line per plan - 9 batch shapes x 3
    depths x {uniform, two ragged batches} x {default knobs, every knob moved alone, every optional weight image missing alone, the
    dense drop-in} - with every EncoderPlan field; the fixture holds the lines the plan printed before it moved into the header, so
    any later change of a launch decision shows here as a changed line.  The program itself checks the plan's invariants and the
    knob table (accepted and rejected values, defaults, the unknown-knob error) against values written out in it."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "encoder_plan_host")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "abi_cpp", "encoder_plan_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    got = run.stdout.splitlines()
    assert run.returncode == 0 and got and got[-1] == "encoder_plan_host: ok", (run.stdout[-2000:] + run.stderr[-2000:])
    with open(os.path.join(ROOT, "tests", "golden", "encoder_plan_table.txt")) as fh:
        want = [ln for ln in fh.read().splitlines() if not ln.startswith("#")]
    assert len(want) > 4000
    changed = [(w, g) for w, g in zip(want, got[:-1]) if w != g]
    assert not changed, "plans that differ from the fixture (want, got), first of %d: %r" % (len(changed), changed[0])
    assert len(got) - 1 == len(want)
