"""Seeded scenes for the tests of include/impc_cluster.h.  A GROUP is one cluster object's worth of
work: parameters, one inflated occupancy map, I = 13 instances and two chained calls (so that the
cases that keep state see real state).  Every instance lives in its own 4 m cell of the map and has a
name that says which outcome it is there for; tests/test_cluster_host.py asserts those outcomes and
the three margins with the restatement (tests/cluster_ref.py) alone.

Every map but "quarter" puts its voxel centres on the multiples of 0.1 (origin -8.05), so the 0.2
lattice samples voxel interiors.  The "quarter" map has dyadic voxels (0.125 from -8), so the
0.25 lattice is exact: lattice distances of exactly eps = 0.5 occur and x = 8.0 = map_max is hit.
"""
import functools
import math

import numpy as np

import cluster_ref as ref

I = 13
CELLS = [(-6.0 + 4.0 * (k % 4), -6.0 + 4.0 * (k // 4)) for k in range(16)]


def _map(origin, res, dims):
    """a grid from (origin, origin, origin + 8): the map, its upper corner, the empty inflated grid"""
    m = dict(origin=[origin, origin, origin + 8.0], resolution=res, dims=list(dims))
    return m, [m["origin"][k] + dims[k] * res for k in range(3)], np.zeros(dims, np.uint8)


def _fill(m, occ, pred):
    """occupy every voxel whose centre satisfies pred(x, y, z) (vectorised over the grid)."""
    ax = [m["origin"][k] + (np.arange(m["dims"][k]) + 0.5) * m["resolution"] for k in range(3)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    occ[pred(x, y, z)] = 1


def _block(m, occ, lo, hi):
    e = 1e-6
    _fill(m, occ, lambda x, y, z: (x > lo[0] - e) & (x < hi[0] + e) & (y > lo[1] - e) & (y < hi[1] + e) &
          (z > lo[2] - e) & (z < hi[2] + e))


def _slab(m, occ, c, yaw, half_len, half_wid):
    t, n = (math.cos(yaw), math.sin(yaw)), (-math.sin(yaw), math.cos(yaw))
    _fill(m, occ, lambda x, y, z: (np.abs((x - c[0]) * t[0] + (y - c[1]) * t[1]) <= half_len) &
          (np.abs((x - c[0]) * n[0] + (y - c[1]) * n[1]) <= half_wid))


def _pose(cell, k=0, dx=None, dy=None, yaw=None, speed=1.0):
    """a pose in general position (no lattice plane through the region's corners or its origin)"""
    dx = -1.0 + 0.013 * (k + 1) if dx is None else dx
    dy = 0.017 * (k + 1) - 0.11 if dy is None else dy
    yaw = 0.02 * (k - 6) + 0.005 if yaw is None else yaw
    return (cell[0] + dx, cell[1] + dy, 1.0), (speed * math.cos(yaw), speed * math.sin(yaw), 0.0)


def _calls(names, poses1, poses2, first=(), inactive2=()):
    """two calls over the named instances: poses1 / poses2 map a name to (pos, vel)."""
    calls = []
    for poses, k in ((poses1, 0), (poses2, 1)):
        pos = np.array([poses[n][0] for n in names])
        vel = np.array([poses[n][1] for n in names])
        active = np.array([0 if (k == 1 and n in inactive2) else 1 for n in names], np.int8)
        fst = np.array([1 if (k == 0 and n in first) else 0 for n in names], np.int8)
        calls.append(dict(cur_pos=pos, cur_vel=vel, active=active, first=fst))
    return calls


SMALL = dict(region_x=2.0, region_y=1.5, ground_height=0.3, ceiling_height=1.5, offset=1.0)
Z = (0.0, 2.3)
SLAB = dict(yaw=71.0, half_len=1.27, half_wid=0.11, ox=0.05, oy=0.19)  # chosen for its 2-means margin


def _blocker(m, occ, cell):
    def blk(n, x0, x1, y0, y1, z=Z):
        c = cell[n]
        _block(m, occ, (c[0] + x0, c[1] + y0, z[0]), (c[0] + x1, c[1] + y1, z[1]))
    return blk


def _main(slab=None):
    slab = slab or SLAB
    m, map_max, occ = _map(-8.05, 0.1, (160, 160, 24))
    names = ["kept_when_empty", "no_core", "dense_box", "yawed_slab", "two_pillars", "wide_box", "big_cloud",
             "small_cloud", "heading_held", "first_at_rest", "inactive", "tall_box", "far_box"]
    cell = dict(zip(names, CELLS))
    blk = _blocker(m, occ, cell)
    blk("kept_when_empty", 0.0, 0.8, -0.4, 0.4)
    blk("no_core", 0.4, 0.4, 0.0, 0.0)  # one column: 7 points, none of them core
    blk("dense_box", 0.0, 0.8, -0.4, 0.4)
    c = cell["yawed_slab"]
    _slab(m, occ, (c[0] + slab["ox"], c[1] + slab["oy"]), math.radians(slab["yaw"]), slab["half_len"],
          slab["half_wid"])
    blk("two_pillars", 0.0, 0.8, -1.2, -0.4)
    blk("two_pillars", 0.0, 0.8, 0.4, 1.2)
    blk("wide_box", 0.2, 0.8, -1.0, 1.0)
    blk("big_cloud", -0.2, 1.0, -1.0, 1.0)
    blk("small_cloud", 0.2, 0.6, -0.2, 0.2)
    blk("heading_held", 0.0, 0.8, -0.4, 0.4)
    blk("first_at_rest", 0.0, 0.8, -0.4, 0.4)
    blk("inactive", 0.0, 0.8, -0.4, 0.4)
    blk("tall_box", 0.2, 1.0, -0.2, 0.6)
    blk("far_box", 1.0, 1.6, -0.6, 0.2)
    p1 = {n: _pose(cell[n], k) for k, n in enumerate(names)}
    p2 = {n: _pose(cell[n], k + 3) for k, n in enumerate(names)}
    p1["first_at_rest"] = _pose(cell["first_at_rest"], 9, speed=0.0)  # first: heading = atan2(0, 0) = 0 is taken
    p2["first_at_rest"] = _pose(cell["first_at_rest"], 4, speed=0.0)  # not first: held
    p1["heading_held"] = _pose(cell["heading_held"], 8, yaw=0.3)
    p2["heading_held"] = _pose(cell["heading_held"], 5, yaw=2.0, speed=0.2)  # below min_speed: 0.3 is held
    p2["kept_when_empty"] = _pose(cell["kept_when_empty"], 0, dx=-1.3, yaw=math.pi - 0.02)  # turned away
    p2["inactive"] = _pose(cell["inactive"], 2, yaw=1.0)
    pr = ref.params(**SMALL, max_points=1024, max_boxes=12)
    return dict(pr=pr, map=m, map_max=map_max, occ=occ, names=names,
                calls=_calls(names, p1, p2, first=("first_at_rest",), inactive2=("inactive",)))


def _dbscan():
    """tree_level 0: the boxes are those of the DBSCAN clusters themselves"""
    m, map_max, occ = _map(-8.05, 0.1, (160, 160, 24))
    names = ["contested_border", "preceding_border"] + ["d%d" % k for k in range(I - 2)]
    cell = dict(zip(names, CELLS))
    blk = _blocker(m, occ, cell)
    # two blocks 0.8 apart in y and one point midway just past their far edge: not core (three
    # neighbours in each block), adjacent to core points of both, after both starts
    blk("contested_border", 0.0, 0.8, -1.2, -0.6)
    blk("contested_border", 0.0, 0.8, 0.2, 0.8)
    blk("contested_border", 1.0, 1.0, -0.2, -0.2, (0.9, 0.9))
    # a block with a spike towards the vehicle: the tip precedes every core point of the block
    blk("preceding_border", 0.2, 1.0, -0.4, 0.4)
    blk("preceding_border", -0.2, 0.0, 0.0, 0.0, (0.9, 0.9))
    for k, n in enumerate(names[2:]):
        blk(n, 0.0, 0.6 + 0.2 * (k % 3), -0.4, 0.2 + 0.2 * (k % 2))
        blk(n, 0.2, 0.2, 0.8, 0.8, (0.5, 0.9 + 0.2 * (k % 3)))  # a short column beside it
    p1 = {n: _pose(cell[n], k) for k, n in enumerate(names)}
    p2 = {n: _pose(cell[n], 12 - k) for k, n in enumerate(names)}
    pr = ref.params(**SMALL, tree_level=0, max_points=1024, max_boxes=12)
    return dict(pr=pr, map=m, map_max=map_max, occ=occ, names=names, calls=_calls(names, p1, p2))


def _quarter():
    m, map_max, occ = _map(-8.0, 0.125, (128, 128, 16))
    names = ["upper_face", "eps_exact"] + ["q%d" % k for k in range(I - 2)]
    cell = dict(zip(names, [CELLS[3], CELLS[0]] + CELLS[4:4 + I - 2]))
    for k, n in enumerate(names[1:]):
        c = cell[n]
        _block(m, occ, (c[0], c[1] - 0.5, 0.0), (c[0] + 0.75 + 0.25 * (k % 3), c[1] + 0.25 * (k % 4), 2.0))
    # upper_face: the vehicle looks at the map's x = 8.0 face: the lattice sheet x = 8.0 is in the map
    # (closed box) and its voxel index is past the grid, i.e. occupied
    _block(m, occ, (7.25, cell["upper_face"][1] - 0.5, 0.0), (7.9, cell["upper_face"][1] + 0.5, 2.0))
    p1 = {n: _pose(cell[n], k) for k, n in enumerate(names)}
    p2 = {n: _pose(cell[n], k + 4) for k, n in enumerate(names)}
    p1["upper_face"] = _pose((7.3, cell["upper_face"][1]), 1)
    p2["upper_face"] = _pose((7.1, cell["upper_face"][1]), 3)
    pr = ref.params(**dict(SMALL, cloud_res=0.25, ground_height=0.25), tree_level=0, max_points=1024, max_boxes=12)
    return dict(pr=pr, map=m, map_max=map_max, occ=occ, names=names, calls=_calls(names, p1, p2))


def _caps(slab=None):
    """small capacities: 200 points, 2 boxes"""
    slab = slab or SLAB
    m, map_max, occ = _map(-8.05, 0.1, (160, 160, 24))
    names = ["too_many_points", "too_many_boxes", "too_many_initial"] + ["c%d" % k for k in range(I - 3)]
    cell = dict(zip(names, CELLS))
    blk = _blocker(m, occ, cell)
    blk("too_many_points", 0.0, 1.0, -1.0, 1.0)
    c = cell["too_many_boxes"]  # the main group's slab: 8 boxes
    _slab(m, occ, (c[0] + slab["ox"], c[1] + slab["oy"]), math.radians(slab["yaw"]), slab["half_len"],
          slab["half_wid"])
    for dy in (-1.2, -0.2, 0.8):  # three separate DBSCAN clusters
        blk("too_many_initial", 0.2, 0.6, dy, dy + 0.4)
    for n in names[3:]:
        blk(n, 0.2, 0.8, -0.2, 0.4)
    p2 = {n: _pose(cell[n], k) for k, n in enumerate(names)}
    p2["too_many_boxes"] = _pose(cell["too_many_boxes"], 3)  # the pose that sees the slab in "main"
    # the first call shows every instance the last filler's block: boxes to keep
    p1 = {n: _pose(cell[names[-1]], k) for k, n in enumerate(names)}
    pr = ref.params(**SMALL, max_points=200, max_boxes=2)
    return dict(pr=pr, map=m, map_max=map_max, occ=occ, names=names, calls=_calls(names, p1, p2))


def _lonely():
    """density_thresh 1.5 splits every cluster, min_pts 0 makes every point core and eps 0.3 joins
    lattice neighbours only: a cluster is split down to single points, and a single point has no
    2-means seed -- the reference's undefined case (an uninitialised fpoint, then points[0] of the
    empty child).  The state starts with one box per instance, which every flagged instance keeps."""
    m, map_max, occ = _map(-8.05, 0.1, (160, 160, 24))
    names = ["empty_child", "empty_child_later"] + ["e%d" % k for k in range(I - 2)]
    cell = dict(zip(names, CELLS))
    blk = _blocker(m, occ, cell)
    blk("empty_child", 0.4, 0.4, 0.0, 0.0, (0.9, 0.9))  # one point: split at level 0
    blk("empty_child_later", 0.4, 0.6, 0.2, 0.2, (0.9, 0.9))  # two points: one each, split at level 1
    p1 = {n: _pose(cell[n], k) for k, n in enumerate(names)}  # (the other instances see nothing)
    p2 = {n: _pose(cell[n], k + 2) for k, n in enumerate(names)}
    pr = ref.params(**SMALL, density_thresh=1.5, min_pts=0, eps=0.3, max_points=64, max_boxes=4)
    init = dict(count=np.ones(I, np.int32), centroid=np.full((I, 4, 3), 0.25), size=np.full((I, 4, 3), 0.5),
                yaw=np.full((I, 4), -0.125))
    return dict(pr=pr, map=m, map_max=map_max, occ=occ, names=names, calls=_calls(names, p1, p2), init=init)


def three_boxes(instances):
    """every instance sees the same three separate blocks from a pose of its own: three boxes each,
    for a replan with num_static = 3 (one call)"""
    m, map_max, occ = _map(-8.05, 0.1, (160, 160, 24))
    cell = CELLS[5]
    for dy in (-1.2, -0.2, 0.8):
        _block(m, occ, (cell[0] + 0.2, cell[1] + dy, Z[0]), (cell[0] + 0.6, cell[1] + dy + 0.4, Z[1]))
    names = ["v%d" % k for k in range(instances)]
    poses = {n: _pose(cell, k % 7, dx=-1.0 + 0.011 * (k + 1)) for k, n in enumerate(names)}
    pr = ref.params(**SMALL, max_points=512, max_boxes=3)
    return dict(pr=pr, map=m, map_max=map_max, occ=occ, names=names, calls=_calls(names, poses, poses)[:1])


BUILDERS = dict(main=_main, dbscan=_dbscan, quarter=_quarter, caps=_caps, lonely=_lonely)


def initial_state(g):
    """the state before the first call: zeros, or what the group sets"""
    state = ref.new_state(I, g["pr"])
    for k, v in g.get("init", {}).items():
        state[k][...] = v
    return state


@functools.lru_cache(maxsize=None)
def group(name):
    """The group with the restatement's result after each call: g["ref"][k] is the state after call
    k (copies), g["facts"][k] the per-instance facts of call k."""
    g = BUILDERS[name]()
    state = initial_state(g)
    g["ref"], g["facts"] = [], []
    for call in g["calls"]:
        facts = ref.run(g["pr"], g["map"], g["map_max"], g["occ"], call["cur_pos"], call["cur_vel"], state,
                        active=call["active"], first=call["first"])
        g["facts"].append(facts)
        g["ref"].append({k: v.copy() for k, v in state.items()})
    return g


def groups():
    return [group(n) for n in BUILDERS]


if __name__ == "__main__":  # a look at what each scene gives
    for gname in BUILDERS:
        g = group(gname)
        for k in range(2):
            for i, n in enumerate(g["names"]):
                f, s = g["facts"][k][i], g["ref"][k]
                if f is None:
                    print(gname, k, n, "inactive")
                    continue
                print(gname, k, n, "pts", f["points"], "init", s["num_initial"][i], "count", s["count"][i], "flags",
                      s["flags"][i], "depth", f["depth"], "head %.3f" % s["heading"][i],
                      "margins %.2e %.2e %.2e" % (f["margin_a"], f["margin_b"], f["margin_c"]),
                      "yaw", np.round(s["yaw"][i, :s["count"][i]], 3).tolist())
