"""Writes gmf_amd/csrc/tsdf_mc_table.inc, the kernels' copy of the marching-cubes case table, from its one home
gmf_amd/_mc_table.py.  Run it after changing the table; tests/test_fragments_mesh_host.py fails while the two differ.

    python tools/gen_mc_table.py            # rewrite the file
    python tools/gen_mc_table.py --print    # to stdout"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "gmf_amd", "csrc", "tsdf_mc_table.inc")


def text():
    spec = importlib.util.spec_from_file_location("_mc_table", os.path.join(ROOT, "gmf_amd", "_mc_table.py"))     # (no torch import)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = mod.TRI_TABLE
    assert len(rows) == 256 and all(len(r) == 16 for r in rows)
    head = "// Written by tools/gen_mc_table.py from gmf_amd/_mc_table.py: the 256 x 16 rows of the marching-cubes case table.\n"
    return head + "".join("{" + ", ".join(str(v) for v in r) + "},\n" for r in rows)


if __name__ == "__main__":
    if "--print" in sys.argv[1:]:
        sys.stdout.write(text())
    else:
        with open(OUT, "w") as f:
            f.write(text())
