"""The static-obstacle producer on the host: the scenes of tests/cluster_cases.py hold the outcome
classes they are named for and keep the margins the device comparison is conditioned on (asserted
with the restatement tests/cluster_ref.py alone); the closed form of DBSCAN's visiting order equals
the literal recursion; the serial form over csrc/cluster.hpp (tests/native/cluster_harness.cpp)
equals the restatement bit for bit; and the same harness runs clean as a stand-alone program under
AddressSanitizer and UBSan."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import cluster_cases as cases
import cluster_ref as ref
from impc import OccMap
from impc.clustering import ClusterIn, ClusterOut, ClusterParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "native", "build", "libcluster_harness.so")
OUTPUTS = ("heading", "count", "centroid", "size", "yaw", "flags", "num_points", "num_initial", "cloud", "dbscan_label")
MARGIN = 1e-9


def c_params(pr):
    return ClusterParams(**pr)


def c_map(m):
    return OccMap(origin=(C.c_double * 3)(*m["origin"]), resolution=m["resolution"], dims=(C.c_int32 * 3)(*m["dims"]))


def facts(gname, call, name):
    g = cases.group(gname)
    i = g["names"].index(name)
    return g["facts"][call][i], {k: v[i] for k, v in g["ref"][call].items()}, i


# ---- the scenes are what they are named for (restatement only)
def test_margins_hold_for_every_scene():
    for g in cases.groups():
        for k, fs in enumerate(g["facts"]):
            for n, f in zip(g["names"], fs):
                if f is None:
                    continue
                assert f["margin_a"] > MARGIN and f["margin_b"] > MARGIN, (n, k, f)
                assert f["margin_c"] > MARGIN, (n, k, f)


def test_outcome_classes_are_present():
    f0, s0, i = facts("main", 0, "kept_when_empty")
    f1, s1, _ = facts("main", 1, "kept_when_empty")
    assert f0["points"] > 0 and s0["count"] == 1 and f1["points"] == 0  # an empty cloud after a non-empty one:
    assert s1["count"] == 1 and s1["flags"] == 0  # run() does nothing, the box stays
    np.testing.assert_array_equal(s1["centroid"], s0["centroid"])
    assert s1["heading"] != s0["heading"]  # (angle_ is updated before the scan)

    f, s, _ = facts("main", 1, "no_core")
    assert f["points"] > 0 and f["core"] == 0 and s["count"] == 0 and s["flags"] == 0

    f, s, _ = facts("main", 1, "dense_box")  # kept unsplit; angle 0 wins the tie against angle 10 (pi / 2)
    assert f["splits"] == 0 and s["count"] == 1 and s["yaw"][0] == 0.0
    n = s["num_points"]
    pts = [tuple(p) for p in s["cloud"][:n][s["dbscan_label"][:n] == 0]]
    cen = ref.centre(pts)
    box = []
    for angle in (0.0, math.pi * 10.0 / 20.0):
        q = np.array([ref.rotate(math.cos(angle), math.sin(angle), p, cen) for p in pts])
        box.append(np.sort(np.round(q.max(0) - q.min(0), 9)[:2]))
    np.testing.assert_array_equal(box[0], box[1])  # the same box up to rounding: the strict > decides

    f, s, _ = facts("main", 1, "yawed_slab")
    assert f["depth"] == 3 and s["num_initial"] == 1 and s["count"] >= 4

    f, s, _ = facts("dbscan", 1, "contested_border")
    assert f["contested"] >= 1 and s["num_initial"] == 2
    f, s, _ = facts("dbscan", 1, "preceding_border")
    assert f["preceding"] >= 1

    assert facts("main", 1, "big_cloud")[0]["points"] > 256
    assert 0 < facts("main", 1, "small_cloud")[0]["points"] <= 64

    f, s, _ = facts("quarter", 1, "upper_face")
    assert f["upper_face"] > 0 and s["count"] >= 1
    g = cases.group("quarter")
    assert g["pr"]["cloud_res"] == 0.25
    n = s["num_points"]
    d = np.sqrt(((s["cloud"][:n, None] - s["cloud"][None, :n]) ** 2).sum(-1))
    assert (d == g["pr"]["eps"]).any()  # lattice distances of exactly eps

    g = cases.group("main")
    i = g["names"].index("heading_held")
    v = g["calls"][1]["cur_vel"][i]
    assert np.linalg.norm(v) < g["pr"]["min_speed"]
    assert g["ref"][1]["heading"][i] == g["ref"][0]["heading"][i] == 0.3 != math.atan2(v[1], v[0])
    i = g["names"].index("first_at_rest")
    assert not g["calls"][0]["cur_vel"][i].any() and g["calls"][0]["first"][i]
    st = ref.new_state(cases.I, g["pr"])
    st["heading"][:] = 1.25  # whatever angle_ held before, the first call replaces it by atan2(0, 0)
    ref.run(g["pr"], g["map"], g["map_max"], g["occ"], g["calls"][0]["cur_pos"], g["calls"][0]["cur_vel"], st,
            first=g["calls"][0]["first"])
    assert st["heading"][i] == 0.0
    i = g["names"].index("inactive")
    assert g["facts"][1][i] is None and not g["calls"][1]["active"][i]
    for k in ref.new_state(1, g["pr"]):
        np.testing.assert_array_equal(g["ref"][1][k][i], g["ref"][0][k][i])

    for name, flag in (("too_many_points", ref.FLAG_POINTS), ("too_many_boxes", ref.FLAG_BOXES),
                       ("too_many_initial", ref.FLAG_BOXES)):
        f, s, i = facts("caps", 1, name)
        s0 = facts("caps", 0, name)[1]
        assert s["flags"] == flag and s0["flags"] == 0 and s0["count"] == 1, name
        assert s["count"] == 1  # the previous box and count stay
        np.testing.assert_array_equal(s["centroid"], s0["centroid"])
    assert facts("caps", 1, "too_many_boxes")[0]["depth"] >= 1  # the tree outgrew max_boxes, not DBSCAN
    assert facts("caps", 1, "too_many_initial")[1]["num_initial"] == 3


def test_an_empty_two_means_child_is_flagged():
    """IMPC_CLUSTER_EMPTY.  Two distinct seeds keep a member each in every round (the member of a label
    that lies farthest along m1 - m0 is strictly closer to its own mean), so a child comes out empty
    only where a seed does not exist: the split of a one-point cluster.  Its density is 1, so it takes
    a density_thresh above 1; no 2-means distance is compared in that split (for the lone point margin
    c stays infinite; the pair's is that of its own, proper split one level up)."""
    for name, level in (("empty_child", 1), ("empty_child_later", 2)):
        for call in range(2):
            f, s, i = facts("lonely", call, name)
            assert s["flags"] == ref.FLAG_EMPTY and f["depth"] == level
            assert f["margin_c"] == math.inf or level == 2
            assert s["count"] == 1 and s["yaw"][0] == -0.125  # the state the group began with
    f, s, _ = facts("lonely", 1, "e0")
    assert f["points"] == 0 and s["flags"] == 0 and s["count"] == 1
    assert ref.kmeans(ref.params(), [(0.2, 0.4, 0.6)])[0] is None


# ---- DBSCAN: the closed form is the recursion
def test_dbscan_closed_form_equals_the_visiting_order_on_the_cases():
    for g in cases.groups():
        for st in g["ref"]:
            for i in range(cases.I):
                n = int(st["num_points"][i])
                if 0 < n <= g["pr"]["max_points"]:
                    cloud = [tuple(p) for p in st["cloud"][i, :n]]
                    assert ref.dbscan_literal(cloud, g["pr"]["eps"], g["pr"]["min_pts"]) == \
                        ref.dbscan_closed(cloud, g["pr"]["eps"], g["pr"]["min_pts"])


def test_dbscan_closed_form_equals_the_visiting_order_on_random_clouds():
    """200 small random lattice clouds, dense and sparse bands alternating along y (the cloud order is
    x-major, so clusters apart in y start before the points between them): clouds with several
    clusters, contested border points and ones that precede their cluster all occur."""
    rng = np.random.default_rng(1405)
    contested = preceding = multi = 0
    for _ in range(200):
        dims = (int(rng.integers(3, 7)), int(rng.integers(8, 15)), int(rng.integers(2, 5)))
        dens = np.repeat(rng.choice([0.95, 0.15], dims[1] // 2 + 1), 2)[:dims[1]]
        keep = rng.random(dims) < dens[None, :, None]
        cloud = [(0.2 * a, 0.2 * b, 0.2 * c) for a, b, c in np.argwhere(keep)]
        min_pts = int(rng.integers(5, 14))
        lit, clo = ref.dbscan_literal(cloud, 0.5, min_pts), ref.dbscan_closed(cloud, 0.5, min_pts)
        assert lit == clo
        a, b = ref.border_facts(cloud, 0.5, min_pts)
        contested, preceding, multi = contested + a, preceding + b, multi + (clo[1] > 1)
    assert contested > 5 and preceding > 20 and multi > 20


# ---- the harness (csrc/cluster.hpp compiled for the host) against the restatement
def _harness():
    lib = C.CDLL(HARNESS)
    lib.cluster_serial.restype = C.c_int
    lib.cluster_serial.argtypes = [C.POINTER(ClusterParams), C.c_int64, C.POINTER(ClusterIn), C.POINTER(ClusterOut),
                                   C.c_int]
    return lib


def harness_run(lib, g, state, call, threads=1):
    keep = {k: np.ascontiguousarray(v) for k, v in call.items()}
    occ = np.ascontiguousarray(g["occ"])
    i = ClusterIn(active=keep["active"].ctypes.data, first=keep["first"].ctypes.data,
                  cur_pos=keep["cur_pos"].ctypes.data, cur_vel=keep["cur_vel"].ctypes.data, occ_inflated=occ.ctypes.data)
    i.map = c_map(g["map"])
    i.map_max[:] = g["map_max"]
    o = ClusterOut(**{k: state[k].ctypes.data for k in OUTPUTS})
    assert lib.cluster_serial(C.byref(c_params(g["pr"])), cases.I, C.byref(i), C.byref(o), threads) == 0


@pytest.mark.parametrize("gname", list(cases.BUILDERS))
def test_harness_equals_the_restatement_bit_for_bit(gname):
    lib, g = _harness(), cases.group(gname)
    state = cases.initial_state(g)
    for k, call in enumerate(g["calls"]):
        harness_run(lib, g, state, call, threads=1 + 2 * k)
        for key in OUTPUTS:
            np.testing.assert_array_equal(state[key].view(np.uint8), g["ref"][k][key].view(np.uint8),
                                          err_msg=f"{gname} call {k} {key}")


def dump_cases(path):
    """the dump cluster_harness.cpp's main reads"""
    with open(path, "wb") as f:
        gs = cases.groups()
        f.write(struct.pack("q", len(gs)))
        for g in gs:
            f.write(bytes(c_params(g["pr"])))
            f.write(struct.pack("q", cases.I))
            f.write(bytes(c_map(g["map"])))
            f.write(struct.pack("3d", *g["map_max"]))
            f.write(np.ascontiguousarray(g["occ"]).tobytes())
            f.write(struct.pack("q", len(g["calls"])))
            for call in g["calls"]:
                for key, dt in (("active", np.int8), ("first", np.int8), ("cur_pos", np.float64), ("cur_vel", np.float64)):
                    f.write(np.ascontiguousarray(call[key], dt).tobytes())


def test_harness_runs_clean_under_the_sanitizers(tmp_path):
    """The harness with its own main, built with -fsanitize=address,undefined as a stand-alone
    program, over every case (nothing is loaded into Python under a sanitizer)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, dump = str(tmp_path / "cluster_check"), str(tmp_path / "cases.bin")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DCLUSTER_HARNESS_MAIN", "-Wno-unknown-pragmas",
                    os.path.join(ROOT, "tests", "native", "cluster_harness.cpp"), "-o", exe, "-lpthread"], check=True)
    dump_cases(dump)
    r = subprocess.run([exe, dump], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    assert r.stdout.startswith("cases %d checksum" % len(cases.BUILDERS)), r.stdout
