"""include/impc_cluster.h against its ctypes mirror (impc.clustering): struct sizes and field offsets
from the C compiler on the header itself, the constants, the defaults and the exported symbols."""
import ctypes as C
import os
import shutil
import subprocess

import impc
from impc import clustering as CL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = (("impc_cluster_params", CL.ClusterParams), ("impc_cluster_in", CL.ClusterIn),
           ("impc_cluster_out", CL.ClusterOut))


def test_cluster_struct_layouts_match_the_header(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "impc_cluster.h"', "int main(void) {"]
    for cname, py in STRUCTS:
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
    lines.append('printf("%d %d %d %d\\n", IMPC_CLUSTER_POINTS, IMPC_CLUSTER_BOXES, IMPC_CLUSTER_EMPTY, IMPC_CLUSTER_NOISE);')
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, py in STRUCTS:
        want.append(C.sizeof(py))
        want += [getattr(py, f).offset for f, _ in py._fields_]
    want += [CL.FLAG_POINTS, CL.FLAG_BOXES, CL.FLAG_EMPTY, CL.NOISE]
    assert got == want


def test_cluster_defaults_are_the_reference_defaults():
    p = CL.cluster_params()
    assert (p.cloud_res, p.region_x, p.region_y, p.ground_height, p.ceiling_height) == (0.2, 5.0, 2.0, 0.3, 2.0)
    assert (p.offset, p.min_speed, p.eps, p.density_thresh) == (2.0, 0.3, 0.5, 0.9)
    assert (p.min_pts, p.tree_level, p.angle_num, p.kmeans_iters) == (15, 3, 20, 10)
    assert p.max_points > 0 and p.max_boxes > 0
    assert CL.cluster_params(**CL.LIVE_PARAMS).region_x == 6.0


def test_cluster_symbols_are_exported_and_bound():
    lib = C.CDLL(impc.LIB_PATH)
    for name in ("impc_cluster_default_params", "impc_cluster_create", "impc_cluster_destroy", "impc_cluster_run_device",
                 "impc_cluster_run"):
        assert hasattr(lib, name) and name in impc.EXPORTED, name
