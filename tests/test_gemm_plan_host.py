"""The launch decision of gmf_gemm_f32 (csrc/gemm_plan.hpp), no GPU: tests/abi_cpp/gemm_plan_host.cpp as a program of its own under
the host sanitizers, over the case table that tests/test_gpu_gemm_forms.py runs on the device (tests/golden/gemm_forms_table.txt).
The program checks every plan's invariants; this test asserts from the plans it prints that the table reaches every form."""
import collections
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "gemm_forms_table.txt")

INSTANTIATIONS = ([f"lds<{t},{tile}>" for t in ("NN", "NT", "TN", "TT") for tile in ("128x128", "64x128", "64x64")] +
                  [f"f32<{t},{tile}>" for t in ("NN", "NT", "TN", "TT") for tile in ("128x128", "64x128")])


def read_table():
    """[{column: int}] in file order; the last comment line names the columns."""
    with open(TABLE) as fh:
        lines = fh.read().splitlines()
    cols = [ln for ln in lines if ln.startswith("#")][-1][1:].split()
    return [dict(zip(cols, map(int, ln.split()))) for ln in lines if ln and not ln.startswith("#")]


def test_gemm_plan_table_reaches_every_form_under_sanitizers(tmp_path):
    """Built with the host compiler and -fsanitize=address,undefined.  One printed line per table case with the GemmPlan fields, the
    contraction length of the first and the last split, the direct kernel's loader choice, and whether the case alone (batch 1)
    takes the same plan.  Asserted: all 12 k_gemm_lds and 8 k_gemm_f32 instantiations, each with and without split-K; every reduce
    group count; k_gemm_lds splits of 1 .. 7 k-steps and a ragged one; k_gemm_f32 with an odd and an even number of full steps, each
    with and without a ragged last step, and both loaders of each k-contiguous operand in every instantiation that has one; the
    flagged rounding, determinism and NaN cases are the ones the GPU test needs.  A grid of 300 000 geometries in the program
    finds no form unreachable."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gemm_plan_host")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "abi_cpp", "gemm_plan_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe, TABLE], capture_output=True, text=True)
    got = run.stdout.splitlines()
    assert run.returncode == 0 and got and got[-1] == "gemm_plan_host: ok", (run.stdout[-2000:] + run.stderr[-2000:])
    table = read_table()
    plans = []
    for ln in got:
        if ln.startswith("case "):
            t = ln.split()
            plans.append({k: (v if k == "form" else int(v)) for k, v in zip(t[0::2], t[1::2])})
    assert len(plans) == len(table) and [p["case"] for p in plans] == list(range(len(table)))
    assert not [ln for ln in got if ln.startswith("unreached")], got[-8:]

    count = collections.Counter(p["form"] for p in plans)
    groups = collections.Counter(p["groups"] for p in plans if p["groups"])
    lens = {fam: [n for p in plans if p["lds"] == (fam == "lds") for n in (p["len_first"], p["len_last"])] for fam in ("lds", "f32")}
    lds_steps = sorted({(n + 15) // 16 for n in lens["lds"]})
    reached = ("forms reached (cases): " + ", ".join(f"{f} {n}" for f, n in sorted(count.items())) +
               f"; reduce groups (cases): {dict(sorted(groups.items()))}; k_gemm_lds k-steps per split: {lds_steps}")
    print(reached)

    for inst in INSTANTIATIONS:
        assert count[inst] > 0 and count[inst + "+splitk"] > 0, f"{inst} missing with or without split-K; {reached}"
    assert len(count) == 40, reached
    assert set(groups) == {1, 2, 4, 8, 16}, reached
    assert set(range(1, 8)) <= set(lds_steps) and any(n % 16 for n in lens["lds"]), reached
    assert {n % 16 for n in lens["lds"]} >= {0, 4, 8, 12} and {n % 16 for n in lens["f32"]} >= {0, 1, 15}, reached
    full_ragged = {((n // 16) % 2, n % 16 != 0) for n in lens["f32"] if n >= 16}
    assert full_ragged == {(0, False), (0, True), (1, False), (1, True)}, (full_ragged, reached)
    for inst in INSTANTIATIONS[12:]:
        mine = [p for p in plans if p["form"].startswith(inst)]
        if inst[4] == "N":      # A's contraction index is contiguous: both loaders
            assert {p["vecA"] for p in mine} == {0, 1}, (inst, reached)
        if inst[5] == "T":
            assert {p["vecB"] for p in mine} == {0, 1}, (inst, reached)
    assert {p["vecA"] for p in plans if not p["lds"]} == {0, 1} and {p["vecB"] for p in plans if not p["lds"]} == {0, 1}

    # the flagged cases: rounding = the longest K of each instantiation; determinism = every group count, batched, same plan alone;
    # NaN = one per kernel family without and one with split-K, at least two rows
    for inst in INSTANTIATIONS:
        mine = [p for p in plans if p["form"].replace("+splitk", "") == inst]
        longest = max(table[p["case"]]["K"] for p in mine)
        assert any(p["flags"] & 1 and table[p["case"]]["K"] == longest for p in mine), f"{inst}: no rounding case at K = {longest}"
    det = [p for p in plans if p["flags"] & 2]
    assert {p["groups"] for p in det} >= {1, 2, 4, 8, 16}, sorted({p["groups"] for p in det})
    assert all(p["alone_same"] and table[p["case"]]["batch"] > 1 for p in det)
    nan = [p for p in plans if p["flags"] & 4]
    assert {(p["lds"], p["ksplits"] > 1) for p in nan} == {(0, False), (0, True), (1, False), (1, True)}
    assert all(table[p["case"]]["M"] > 1 for p in nan)
