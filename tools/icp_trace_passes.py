"""Per-pass kernel times of ICP's two searches from a rocprofv3 kernel trace of
    rocprofv3 --kernel-trace --stats -f csv -- python tools/time_solvers.py --icp-shape SHAPE
The per-kernel averages of the stats file mix working launches with those of a finished pair, which return at once.  This reads
the trace (*_kernel_trace.csv), splits it into calls at k_icp_init, keeps the calls of 11 passes (both criteria at 0,
max_iteration = 10: every pass runs) and prints medians over passes 0..9: the search kernel, k_icp_step, the last step (pass
10 stops before the Umeyama update) and, for the grid, the sum of launch_grid_build's four kernels.
A trace of `tools/time_solvers.py --plane-shape SHAPE` also holds point-to-plane calls (k_icp_plane_partials, k_icp_plane_solve
in place of k_icp_step); they get a line of their own.  So do the coloured calls of `--colored-shape SHAPE` (k_icp_color_partials
in the place of k_icp_plane_partials), with the medians of k_knn_search and k_color_gradient over the whole trace beside them.
Usage: python tools/icp_trace_passes.py TRACE.csv [TRACE.csv ...]"""
import csv
import statistics as st
import sys


def passes(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None
    for r in rows:
        n, dur = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "k_icp_init" in n:
            cur = {"nn": [], "step": [], "build": [], "grid": False, "partials": [], "solve": [], "color": []}
            calls.append(cur)
        elif cur is None:
            continue
        elif "k_icp_nn_grid" in n:
            cur["nn"].append(dur)
            cur["grid"] = True
        elif "k_icp_nn" in n:
            cur["nn"].append(dur)
        elif "k_icp_step" in n:
            cur["step"].append(dur)
        elif "k_icp_plane_partials" in n:
            cur["partials"].append(dur)
        elif "k_icp_color_partials" in n:
            cur["color"].append(dur)
        elif "k_icp_plane_solve" in n:
            cur["solve"].append(dur)
        elif "k_grid_count" in n or "k_grid_scatter" in n or "rocprim" in n:
            cur["build"].append(dur)
    for grid in (False, True):
        c11 = [c for c in calls if len(c["nn"]) == 11 and c["grid"] == grid and len(c["step"]) == 11]
        if not c11:
            continue
        nn = [x for c in c11 for x in c["nn"][:10]]
        step = [x for c in c11 for x in c["step"][:10]]
        last = [c["step"][10] for c in c11]
        build = [sum(c["build"]) for c in calls if c["grid"] == grid and c["build"]]
        line = (f"{path}: {'grid ' if grid else 'brute'} {len(c11)} calls; search {st.median(nn):.1f} [{min(nn):.1f}, {max(nn):.1f}] us, "
                f"k_icp_step {st.median(step):.1f} us, last step {st.median(last):.1f} us")
        if build:
            line += f", build kernels {st.median(build):.1f} us (median of {len(build)} calls)"
        print(line)
    for key, what in (("partials", "point-to-plane"), ("color", "coloured")):
        p11 = [c for c in calls if len(c["nn"]) == 11 and len(c[key]) == 11]
        if p11:
            def med(k):
                x = [v for c in p11 for v in c[k][:10]]
                return f"{st.median(x):.1f} [{min(x):.1f}, {max(x):.1f}] us"
            print(f"{path}: {what} {len(p11)} calls; search {med('nn')}, k_icp_{'plane' if key == 'partials' else 'color'}_partials "
                  f"{med(key)}, k_icp_plane_solve {med('solve')}")
    for name in ("k_knn_search", "k_color_gradient"):
        x = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if x:
            print(f"{path}: {name} {len(x)} launches; {st.median(x):.1f} [{min(x):.1f}, {max(x):.1f}] us")


if __name__ == "__main__":
    for p in sys.argv[1:]:
        passes(p)
