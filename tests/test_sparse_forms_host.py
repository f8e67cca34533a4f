"""The launch decisions of the sparse engine (csrc/sparse_conv_plan.hpp), no GPU: tests/abi_cpp/sparse_plan_host.cpp as a program of
its own under the host sanitizers, over the case table that tests/test_gpu_sparse_forms.py runs on the device
(tests/golden/sparse_forms_table.txt).  The levels and maps of every case come from tests/sparse_reference.py; the program prints
each launch's plan and checks its invariants; this test asserts, class by class and by name, that the table reaches every edge of
the kernels' branches.  The table reader, the coordinate sets and the per-case geometry are shared with the GPU test."""
import collections
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import sparse_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "sparse_forms_table.txt")

KERNELS = ["conv", "dgrad", "wgrad", "narrow", "narrow_wgrad", "head", "bnm"]
SETS = ["line-1", "line-64", "line-65", "line-130", "cube12", "cube10-k7", "ragged-d3", "d6-300", "line-16200"]
ROUNDING, NONFINITE, POISON, REPEAT = 1, 2, 4, 8

_LINE_MAPS = [(3, 0, 0), (3, 1, 0), (3, 0, 1)]
# name -> (levels, the plan's maps)
SET_PLANS = {**{n: (2, _LINE_MAPS) for n in SETS if n.startswith("line-")},
             "cube12": (4, [(3, 0, 0), (3, 1, 0), (3, 0, 1), (3, 3, 2), (3, 2, 3), (1, 1, 0), (1, 0, 1)]),
             "cube10-k7": (1, [(7, 0, 0)]),
             "ragged-d3": (2, [(3, 0, 0), (3, 1, 0), (3, 0, 1), (3, 1, 1)]),
             "d6-300": (1, [(3, 0, 0)])}


def read_table():
    """[{column: int}] in file order; the last comment line names the columns."""
    with open(TABLE) as fh:
        lines = fh.read().splitlines()
    cols = [ln for ln in lines if ln.startswith("#")][-1][1:].split()
    return [dict(zip(cols, map(int, ln.split()))) for ln in lines if ln and not ln.startswith("#")]


def case_id(i, c):
    m = "id" if c["k"] == 0 else f"k{c['k']}.{c['out']}{c['in']}"
    return (f"{i}-{KERNELS[c['kernel']]}-{SETS[c['set']]}-{m}-{c['ca']}+{c['cb']}x{c['cout']}" + (f"h{c['hid']}" if c["hid"] else "") +
            (f"-s{c['nsplit']}" if c["nsplit"] else ""))


def random_coords(M, D, span, batches, seed):
    """M unique rows (batch, c_1 .. c_D), coordinates in [-span, span), ragged batch sizes, shuffled."""
    rng = np.random.default_rng(seed)
    rows = set()
    while len(rows) < M:
        b = int(rng.choice(batches, p=np.linspace(1, 2, len(batches)) / np.linspace(1, 2, len(batches)).sum()))
        rows.add((b,) + tuple(int(v) for v in rng.integers(-span, span, D)))
    out = np.array(sorted(rows), dtype=np.int64)
    return out[rng.permutation(M)]


def _cube(n, seed):
    ax = np.arange(n)
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    rows = np.concatenate([np.zeros((len(g), 1), np.int64), g], 1)
    return rows[np.random.default_rng(seed).permutation(len(rows))]


@functools.lru_cache(maxsize=None)
def coord_set(name):
    """int64 [M, 1 + D] rows of a named set, generated: no files."""
    if name.startswith("line-"):
        n = int(name[5:])
        return np.stack([np.zeros(n, np.int64), np.arange(n, dtype=np.int64)], 1)
    return {"cube12": lambda: _cube(12, 21), "cube10-k7": lambda: _cube(10, 22),
            "ragged-d3": lambda: random_coords(700, 3, 7, [0, 1, 2], 11),           # the set of tests/test_gpu_sparse.py
            "d6-300": lambda: random_coords(300, 6, 3, [0, 1], 23)}[name]()


@functools.lru_cache(maxsize=None)
def set_levels(name):
    return R.build_levels(coord_set(name), SET_PLANS[name][0])


@functools.lru_cache(maxsize=None)
def set_map(name, kmap):
    """(row_ptr, pairs) of map (k, out, in) of a set, from the float64 reference's map builder"""
    return R.map_between(set_levels(name), *kmap)


def layer_nsplit(K, cin, cout):
    """gmf_amd.sparse.layer_nsplit, restated (the GPU test asserts the two agree)"""
    if K == 1:
        return 1
    if K * cin * cout * 4 > (16 << 20):
        return min(K, -(-256 // -(-cout // 64)))
    return min(K, 9)


def geometry(c):
    """What a case's launch is made of: {set, kmap (the case's map or None), lmap (the map the launch walks: the transposed one for
    dgrad), K, cin, cout (of the launch), nsplit, cap, n_out, n_in, cmap}."""
    name = SETS[c["set"]]
    lv = set_levels(name)
    kern = KERNELS[c["kernel"]]
    kmap = None if c["k"] == 0 else (c["k"], c["out"], c["in"])
    D = lv[0].shape[1] - 1
    g = {"set": name, "kern": kern, "kmap": kmap, "cap": len(lv[0]), "n_out": len(lv[c["out"]]), "n_in": len(lv[c["in"]]),
         "K": 1 if kmap is None else c["k"] ** D, "cin": c["ca"] + c["cb"], "cout": c["cout"], "nsplit": c["nsplit"], "lmap": kmap}
    if kmap is not None:
        assert kmap in SET_PLANS[name][1], (name, kmap)
    if kern == "dgrad":                                  # a convolution of dy over the transposed map into the input level
        g.update(cin=c["cout"], cout=c["ca"] + c["cb"], n_out=g["n_in"], n_in=g["n_out"],
                 nsplit=layer_nsplit(g["K"], c["cout"], c["ca"] + c["cb"]))
        if kmap is not None and kmap[1] != kmap[2]:
            g["lmap"] = (kmap[0], kmap[2], kmap[1])
            assert g["lmap"] in SET_PLANS[name][1]
    g["cmap"] = None if g["lmap"] is None else set_map(name, g["lmap"])
    return g


def sum_length(c, g):
    """the number of terms of the longest sum of a case (what decides its rounding error)"""
    kern = g["kern"]
    if kern in ("conv", "dgrad", "narrow"):
        return g["cin"] * (1 if g["cmap"] is None else int(np.diff(g["cmap"][0]).max()))
    if kern in ("wgrad", "narrow_wgrad"):
        return g["n_out"] if g["cmap"] is None else int(np.bincount(g["cmap"][1][:, 0], minlength=g["K"]).max())
    return c["ca"] + c["cb"] + c["hid"] if kern == "head" else g["n_out"]


def _run_host(tmp_path, lines):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "sparse_plan_host")
    build = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "abi_cpp", "sparse_plan_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    geo = tmp_path / "geometry.txt"
    geo.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(geo)], capture_output=True, text=True)
    got = run.stdout.splitlines()
    assert run.returncode == 0 and got and got[-1] == "sparse_plan_host: ok", (run.stdout[-2000:] + run.stderr[-2000:])
    assert len(got) == len(lines) + 1
    return got[:-1]


def _fields(line, *names):
    """'conv groups 2 rows 0 65 130 slices 0 1 2 3' -> {'groups': [2], 'rows': [0, 65, 130], 'slices': [0, 1, 2, 3]}"""
    out, key = {}, None
    for tok in line.split()[1:]:
        if tok in names:
            key = tok
            out[key] = []
        else:
            out[key].append(int(tok))
    return out


def test_sparse_forms_table_reaches_every_edge_under_sanitizers(tmp_path):
    table = read_table()
    geos = [geometry(c) for c in table]
    lines = []
    for c, g in zip(table, geos):
        kern = g["kern"]
        if kern in ("conv", "dgrad"):
            lines.append(f"conv {g['K']} {g['cin']} {g['cout']} {g['nsplit']} {g['cap']} {g['n_out']}")
        elif kern in ("wgrad", "narrow_wgrad"):
            per = [g["n_out"]] if g["cmap"] is None else np.bincount(g["cmap"][1][:, 0], minlength=g["K"]).tolist()
            lines.append(f"wgrad {int(kern == 'narrow_wgrad')} {g['K']} {sum(per)} " + " ".join(map(str, per)))
        elif kern == "narrow":
            lines.append(f"narrow {g['K']} {g['cin']} {g['cout']} {g['cap']}")
        elif kern == "head":
            lines.append(f"head {g['cap']}")
        else:
            lines.append(f"bnm {g['cap']} {g['n_out']}")
    plans = _run_host(tmp_path, lines)

    reached = collections.defaultdict(list)            # class name -> the cases that reach it

    def hit(name, i, cond=True):
        if cond:
            reached[name].append(i)

    for i, (c, g, ln) in enumerate(zip(table, geos, plans)):
        kern, K, cin, cout = g["kern"], g["K"], g["cin"], g["cout"]
        if kern in ("conv", "dgrad"):
            p = _fields(ln, "groups", "rows", "slices")
            gb, sb, ns = np.array(p["rows"]), np.array(p["slices"]), g["nsplit"]
            assert ns >= 1 and len(sb) == ns + 1 and len(gb) == p["groups"][0] + 1
            hit("conv: a row group with no rows", i, bool((np.diff(gb) == 0).any()))
            hit("conv: nsplit == K > 1", i, ns == K and K > 1)
            hit("conv: nsplit does not divide K", i, K % ns != 0)
            for v in (1, 15, 16, 17, 33):
                hit(f"conv: cin = {v}", i, cin == v)
            for v in (1, 3, 63, 64, 65, 130):
                hit(f"conv: cout = {v}", i, cout == v)
            hit("conv: ca / cb seam off a multiple of 16", i, kern == "conv" and c["cb"] > 0 and c["ca"] % 16 != 0)
            hit("conv: identity map with a tile tail", i, g["cmap"] is None and any(n % 64 for n in np.diff(gb)))
            if g["cmap"] is None:
                continue
            row_ptr, pairs = g["cmap"]
            npairs = np.diff(row_ptr)
            o = np.repeat(np.arange(g["n_out"]), npairs)
            d = pairs[:, 0]
            hit("conv: an output row with no pairs", i, bool((npairs == 0).any()))
            nd = np.bincount(d, minlength=K)
            sl = np.searchsorted(sb, np.arange(K), side="right") - 1          # slice of each offset
            full = np.bincount(sl[nd > 0], minlength=ns)
            hit("conv: offsets without pairs inside a slice that has pairs", i, bool(((full > 0) & (full < np.diff(sb))).any()))
            per_row = np.zeros((g["n_out"], ns), dtype=bool)
            per_row[o, sl[d]] = True
            some = per_row.any(1) & ~per_row.all(1)
            hit("conv: a row with pairs in only some slices", i, ns > 1 and bool(some.any()))
            hit("conv: a row whose first slice is empty and a later one is not", i, ns > 1 and bool((some & ~per_row[:, 0]).any()))
            grp = np.searchsorted(gb, o, side="right") - 1
            lens = set(np.bincount(d * len(gb) + grp).tolist())
            for v in (1, 63, 64, 65):
                hit(f"conv: an offset's pair list of {v} in a row group", i, v in lens)
        elif kern in ("wgrad", "narrow_wgrad"):
            p = _fields(ln, "nslots", "P", "chunks", "longest_tiles", "multi_tile", "multi_tile_ragged")
            hit(f"{kern}: P > 64", i, p["P"][0] > 64)
            hit(f"{kern}: a chunk of more than one tile (accumulator carried, loop-top barrier)", i, p["multi_tile"][0] > 0)
            hit(f"{kern}: a multi-tile chunk with a last tile under 64 pairs", i, p["multi_tile_ragged"][0] > 0)
            if g["cmap"] is not None:
                hit(f"{kern}: offsets without pairs", i, bool((np.bincount(g["cmap"][1][:, 0], minlength=K) == 0).any()))
            if kern == "wgrad":
                hit("wgrad: three tiles in a chunk", i, p["longest_tiles"][0] >= 3)
                hit("wgrad: cin tail in a second tile", i, cin > 64 and cin % 64 != 0)
                hit("wgrad: cout tail in a second tile", i, cout > 64 and cout % 64 != 0)
                hit("wgrad: cin and cout below one tile", i, cin < 64 and cout < 64)
                hit("wgrad: full 64 x 64 tile", i, cin == 64 and cout == 64)
                hit("wgrad: two sources, seam off a multiple of 4", i, c["cb"] > 0 and c["ca"] % 4 != 0)
                hit("wgrad: identity map", i, g["cmap"] is None)
            else:
                for L in (16, 32, 64):
                    hit(f"narrow_wgrad: lane groups of {L}", i, (16 if cout <= 16 else 32 if cout <= 32 else 64) == L)
        elif kern == "narrow":
            p = _fields(ln, "lanes", "rows_per_wg", "lds", "grid", "strides")
            L, longest = p["lanes"][0], int(np.diff(g["cmap"][0]).max())
            hit(f"narrow: lane groups of {L} with a row of more than {L} pairs", i, longest > L)
            hit(f"narrow: lane groups of {L}, grid-stride loop", i, p["strides"][0] > 1)
            hit("narrow: W in LDS" if p["lds"][0] else "narrow: W in global memory", i)
            hit("narrow: a row whose last pair group is short", i, bool((np.diff(g["cmap"][0]) % L != 0).any()))
            hit("narrow: an output row with no pairs", i, bool((np.diff(g["cmap"][0])[:g["n_out"]] == 0).any()))
            hit("narrow: fewer valid rows than row slots", i, g["n_out"] < g["cap"])
        elif kern == "head":
            p = _fields(ln, "grid", "strides")
            hit("head: grid-stride loop (more than 4096 rows)", i, p["strides"][0] > 1 and g["cap"] > 4096)
            for w in ((64, 64, 64, 64), (1, 0, 1, 1), (33, 7, 17, 3)):
                hit(f"head: (ca, cb, hid, cout) = {w}", i, (c["ca"], c["cb"], c["hid"], c["cout"]) == w)
            hit("head: fewer valid rows than row slots", i, g["n_out"] < g["cap"])
        else:
            p = _fields(ln, "chunks", "rows")
            nch, C = p["chunks"][0], c["ca"]
            hit("bnm: one chunk", i, nch == 1)
            hit("bnm: a few chunks", i, 1 < nch < 64)
            hit("bnm: 64 chunks", i, nch == 64)
            hit("bnm: valid rows end inside the first chunk", i, nch > 1 and g["n_out"] < p["rows"][1])
            hit("bnm: valid rows end inside a later chunk", i, nch > 1 and p["rows"][1] < g["n_out"] < g["cap"])
            for v in (63, 64, 65):
                hit(f"bnm: C = {v}", i, C == v)
            hit("bnm: C over two column blocks", i, C > 64)

    wanted = (["conv: a row group with no rows", "conv: nsplit == K > 1", "conv: nsplit does not divide K",
               "conv: ca / cb seam off a multiple of 16", "conv: identity map with a tile tail", "conv: an output row with no pairs",
               "conv: offsets without pairs inside a slice that has pairs", "conv: a row with pairs in only some slices",
               "conv: a row whose first slice is empty and a later one is not"] +
              [f"conv: cin = {v}" for v in (1, 15, 16, 17, 33)] + [f"conv: cout = {v}" for v in (1, 3, 63, 64, 65, 130)] +
              [f"conv: an offset's pair list of {v} in a row group" for v in (1, 63, 64, 65)] +
              [f"{k}: {w}" for k in ("wgrad", "narrow_wgrad")
               for w in ("P > 64", "a chunk of more than one tile (accumulator carried, loop-top barrier)",
                         "a multi-tile chunk with a last tile under 64 pairs", "offsets without pairs")] +
              ["wgrad: three tiles in a chunk", "wgrad: cin tail in a second tile", "wgrad: cout tail in a second tile",
               "wgrad: cin and cout below one tile", "wgrad: full 64 x 64 tile", "wgrad: two sources, seam off a multiple of 4",
               "wgrad: identity map"] + [f"narrow_wgrad: lane groups of {L}" for L in (16, 32, 64)] +
              [f"narrow: lane groups of {L} with a row of more than {L} pairs" for L in (16, 32, 64)] +
              [f"narrow: lane groups of {L}, grid-stride loop" for L in (16, 32, 64)] +
              ["narrow: W in LDS", "narrow: W in global memory", "narrow: a row whose last pair group is short",
               "narrow: an output row with no pairs", "narrow: fewer valid rows than row slots",
               "head: grid-stride loop (more than 4096 rows)", "head: fewer valid rows than row slots"] +
              [f"head: (ca, cb, hid, cout) = {w}" for w in ((64, 64, 64, 64), (1, 0, 1, 1), (33, 7, 17, 3))] +
              ["bnm: one chunk", "bnm: a few chunks", "bnm: 64 chunks", "bnm: valid rows end inside the first chunk",
               "bnm: valid rows end inside a later chunk", "bnm: C over two column blocks"] + [f"bnm: C = {v}" for v in (63, 64, 65)])
    print(f"sparse forms table: {len(table)} cases; reached (cases): " + "; ".join(f"{w} [{len(reached[w])}]" for w in wanted))
    missing = [w for w in wanted if not reached[w]]
    assert not missing, f"the table no longer reaches: {missing}"
    # Not in the table: the narrow kernel's grid-stride loop with W in global memory needs more than 4096 x 4 = 16 384 row slots;
    # the loop is the same code in both instantiations (kLdsW only chooses where W is read from) and is reached with W in LDS.

    # the flagged cases are the ones the GPU test needs
    flagged = lambda bit, kern=None: [i for i, (c, g) in enumerate(zip(table, geos))      # noqa: E731
                                      if c["flags"] & bit and (kern is None or g["kern"] == kern)]
    for kern in KERNELS:                                   # rounding: the longest sum of each kernel
        mine = [i for i, g in enumerate(geos) if g["kern"] == kern]
        longest = max(sum_length(table[i], geos[i]) for i in mine)
        assert any(sum_length(table[i], geos[i]) == longest for i in flagged(ROUNDING, kern)), f"{kern}: no rounding case at {longest} terms"
    poison = flagged(POISON, "conv")
    assert poison and all(geos[i]["nsplit"] > 1 for i in poison)
    assert set(poison) & set(reached["conv: nsplit == K > 1"]) and set(poison) & set(reached["conv: a row with pairs in only some slices"])
    assert set(poison) & set(reached["conv: a row whose first slice is empty and a later one is not"])
    assert flagged(POISON, "wgrad") and flagged(POISON, "narrow_wgrad")
    assert set(flagged(POISON, "wgrad")) & set(reached["wgrad: offsets without pairs"])
    nonfinite = {(geos[i]["kern"], "id" if geos[i]["cmap"] is None else ("sliced" if geos[i]["nsplit"] > 1 else "whole")) for i in flagged(NONFINITE, "conv")}
    assert nonfinite >= {("conv", "id"), ("conv", "sliced"), ("conv", "whole")}, nonfinite
    nf_narrow = set(flagged(NONFINITE, "narrow"))
    assert nf_narrow & set(reached["narrow: W in LDS"]) and nf_narrow & set(reached["narrow: W in global memory"])
    assert flagged(NONFINITE, "head") and flagged(NONFINITE, "bnm")
    rep = flagged(REPEAT)
    assert {geos[i]["kern"] for i in rep} >= {"conv", "dgrad", "wgrad", "narrow", "narrow_wgrad"}
    assert any(geos[i]["set"] == "ragged-d3" and geos[i]["nsplit"] > 1 for i in flagged(REPEAT, "conv"))
    # exactness on integers in [-4, 4]: every partial sum is an integer (or, after a scale of 0.5, a half) below 2^24
    for c, g in zip(table, geos):
        assert 16 * g["K"] * max(g["cin"], 1) + 8 < 2 ** 23 and 16 * g["cap"] < 2 ** 23
