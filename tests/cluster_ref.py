"""A plain-Python restatement of the reference's static-obstacle producer, for the tests of
include/impc_cluster.h: mpcPlanner::staticObstacleClusteringCB (trajectory_planner mpcPlanner.cpp:
200-247), obstacleClustering (clustering/obstacleClustering.cpp, .h), DBSCAN (clustering/DBSCAN.h) and
KMeans (clustering/Kmeans.cpp).  Python floats are IEEE doubles and every expression below is written
in the reference's order of operations, so the host harness (tests/native/cluster_harness.cpp) must
agree bit for bit.  Eigen sums three terms as t0 + (t1 + t2) (Redux.h's unroller halves the range).

run() also reports the three margins the device comparison is conditioned on:
  a  the distance of every floor / ceil argument of the region from an integer
  b  min |(p - pOrigin) . face| over the scanned lattice
  c  min |d0 - d1| over every point, round and split of 2-means
"""
import math

import numpy as np

FLAG_POINTS, FLAG_BOXES, FLAG_EMPTY = 1, 2, 4
NOISE, NOT_CLASSIFIED = -2, -1  # DBSCAN.h:17-18

DEFAULTS = dict(cloud_res=0.2, region_x=5.0, region_y=2.0, ground_height=0.3, ceiling_height=2.0, offset=2.0,
                min_speed=0.3, eps=0.5, density_thresh=0.9, min_pts=15, tree_level=3, angle_num=20, kmeans_iters=10,
                max_points=4096, max_boxes=16)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def norm3(a, b, c):
    return math.sqrt(a * a + (b * b + c * c))


def region(pr, pos, vel, first, heading):
    """mpcPlanner.cpp:209-228.  Returns (heading, face, pOrigin, xStart, xEnd, yStart, yEnd, margin a)."""
    angle = math.atan2(vel[1], vel[0])  # :209
    if norm3(vel[0], vel[1], vel[2]) >= pr["min_speed"] or first:  # :210
        heading = angle
    c, s = math.cos(heading), math.sin(heading)
    face, side = (c, s, 0.0), (-s, c, 0.0)  # :213-215
    reach = pr["region_x"] + pr["offset"]
    org = [pos[k] - pr["offset"] * face[k] for k in range(3)]  # :216
    p1 = [org[k] + pr["region_y"] * side[k] for k in range(3)]  # :220-223
    p2 = [org[k] - pr["region_y"] * side[k] for k in range(3)]
    p3 = [p1[k] + reach * face[k] for k in range(3)]
    p4 = [p2[k] + reach * face[k] for k in range(3)]
    res = pr["cloud_res"]
    args = [min(p1[0], p2[0], p3[0], p4[0]) / res, max(p1[0], p2[0], p3[0], p4[0]) / res,
            min(p1[1], p2[1], p3[1], p4[1]) / res, max(p1[1], p2[1], p3[1], p4[1]) / res]
    x0, x1 = math.floor(args[0]) * res, math.ceil(args[1]) * res  # :225-228
    y0, y1 = math.floor(args[2]) * res, math.ceil(args[3]) * res
    margin = min(abs(a - round(a)) for a in args)
    return heading, face, org, x0, x1, y0, y1, margin


def axis(start, end, step):
    """for (v = start; v <= end; v += step): the running sums (:230-232)."""
    out, v = [], start
    while v <= end:
        out.append(v)
        v += step
    return out


def in_map(m, map_max, p):  # occupancyMap.h:479-488
    return all(m["origin"][k] <= p[k] <= map_max[k] for k in range(3))


def inflated_occupied(m, occ, p):  # occupancyMap.h:257-269, :490-505
    idx = [math.floor((p[k] - m["origin"][k]) / m["resolution"]) for k in range(3)]
    if any(idx[k] < 0 or idx[k] >= m["dims"][k] for k in range(3)):
        return True
    return bool(occ[idx[0], idx[1], idx[2]])


def scan(pr, reg, m, map_max, occ):
    """:230-241: the cloud in loop order (x outer, y, z inner) and margin b."""
    _, face, org, x0, x1, y0, y1, _ = reg
    res = pr["cloud_res"]
    zs = axis(pr["ground_height"], pr["ceiling_height"], res)
    cloud, margin = [], math.inf
    for x in axis(x0, x1, res):
        for y in axis(y0, y1, res):
            for z in zs:
                d = (x - org[0]) * face[0] + ((y - org[1]) * face[1] + (z - org[2]) * face[2])  # :234
                margin = min(margin, abs(d))
                if d >= 0 and in_map(m, map_max, (x, y, z)) and inflated_occupied(m, occ, (x, y, z)):
                    cloud.append((x, y, z))
    return cloud, margin


def adjacency(cloud, eps):
    """checkNearPoints (DBSCAN.h:87-97): adj[i] ascending, getDis (:31-33) <= eps, i itself excluded."""
    a = np.asarray(cloud, dtype=np.float64).reshape(-1, 3)
    dx, dy, dz = (a[:, None, k] - a[None, :, k] for k in range(3))
    near = np.sqrt(dx * dx + dy * dy + dz * dz) <= eps
    np.fill_diagonal(near, False)
    return [np.flatnonzero(r).tolist() for r in near]


def dbscan_literal(cloud, eps, min_pts):
    """DBSCAN::run (DBSCAN.h:56-85) in its own visiting order (dfs with an explicit stack of the
    adjacency iterators).  Returns (label per point, clusters)."""
    adj = adjacency(cloud, eps)
    n = len(cloud)
    cluster = [NOT_CLASSIFIED] * n
    core = [len(adj[i]) >= min_pts for i in range(n)]
    idx = -1
    for i in range(n):
        if cluster[i] != NOT_CLASSIFIED:
            continue
        if not core[i]:
            cluster[i] = NOISE
            continue
        idx += 1
        cluster[i] = idx  # dfs(i, idx)
        stack = [iter(adj[i])]
        while stack:
            nxt = next(stack[-1], None)
            if nxt is None:
                stack.pop()
            elif cluster[nxt] == NOT_CLASSIFIED:
                cluster[nxt] = idx
                if core[nxt]:
                    stack.append(iter(adj[nxt]))
    return cluster, idx + 1


def dbscan_closed(cloud, eps, min_pts):
    """The same result without the visiting order: clusters are the components of the core points
    over core-core adjacency, numbered by ascending smallest core index (their start); a point that is
    not core joins the cluster with the smallest start among those with a core point adjacent to it
    and a start below its own index, and is noise otherwise."""
    adj = adjacency(cloud, eps)
    n = len(cloud)
    core = [len(adj[i]) >= min_pts for i in range(n)]
    start, starts = [-1] * n, []
    for i in range(n):
        if not core[i] or start[i] >= 0:
            continue
        starts.append(i)
        start[i], todo = i, [i]
        while todo:
            u = todo.pop()
            for q in adj[u]:
                if core[q] and start[q] < 0:
                    start[q] = i
                    todo.append(q)
    for b in range(n):
        if not core[b]:
            cand = [start[q] for q in adj[b] if core[q] and start[q] < b]
            start[b] = min(cand) if cand else -1
    rank = {s: k for k, s in enumerate(starts)}
    return [rank[s] if s >= 0 else NOISE for s in start], len(starts)


def border_facts(cloud, eps, min_pts):
    """(contested, preceding): the points that are not core and are adjacent to core points of two
    or more clusters that started before them; those adjacent to a core point but noise because every
    such cluster started after them."""
    labels, _ = dbscan_closed(cloud, eps, min_pts)
    adj = adjacency(cloud, eps)
    core = [len(a) >= min_pts for a in adj]
    first = {}
    for i, lab in enumerate(labels):
        if core[i]:
            first.setdefault(lab, i)
    contested = preceding = 0
    for b in range(len(cloud)):
        if core[b]:
            continue
        near = {labels[q] for q in adj[b] if core[q]}
        if len({c for c in near if first[c] < b}) >= 2:
            contested += 1
            assert labels[b] == min(c for c in near if first[c] < b)
        if near and labels[b] == NOISE:
            preceding += 1
    return contested, preceding


def centre(points):
    """(clusterMin + clusterMax) / 2.0 (obstacleClustering.cpp:96-124, :192-218)."""
    lo, hi = list(points[0]), list(points[0])
    for p in points:
        for k in range(3):
            if p[k] < lo[k]:
                lo[k] = p[k]
            elif p[k] > hi[k]:
                hi[k] = p[k]
    return [(lo[k] + hi[k]) / 2.0 for k in range(3)]


def rotate(c, s, p, cen):
    """rot * (p - centroid) + centroid (:238-243); a zero comes out as +0."""
    d0, d1, d2 = p[0] - cen[0], p[1] - cen[1], p[2] - cen[2]
    ms = -s
    return ((c * d0 + (ms * d1 + 0.0 * d2)) + cen[0] + 0.0, (s * d0 + (c * d1 + 0.0 * d2)) + cen[1] + 0.0,
            (0.0 * d0 + (0.0 * d1 + 1.0 * d2)) + cen[2] + 0.0)


def orientation(pr, points):
    """getOrientation (:230-279): (maxDensity, rotated min, rotated max, angle) of the first best angle."""
    cen, res = centre(points), pr["cloud_res"]
    best, out = 0.0, ([0.0] * 3, [0.0] * 3, 0.0)
    for i in range(pr["angle_num"]):
        angle = math.pi * float(i) / float(pr["angle_num"])  # :236
        c, s = math.cos(angle), math.sin(angle)
        lo, hi = list(points[0]), list(points[0])  # :239-240: the UNROTATED points[0]
        for p in points:
            q = rotate(c, s, p, cen)
            for k in range(3):
                if q[k] < lo[k]:
                    lo[k] = q[k]
                elif q[k] > hi[k]:
                    hi[k] = q[k]
        ln, wn, hn = ((hi[k] - lo[k]) / res + 1 for k in range(3))  # :268-270
        density = float(len(points)) / (ln * wn * hn)
        if density > best:  # :273
            best, out = density, (lo, hi, angle)
    return (best,) + out


def classify(p, c0, c1):
    """KMeans::Classify (Kmeans.cpp:40-59) over two centroids: (label, |d0 - d1|)."""
    a = b = 0.0
    for k in range(3):
        a += (p[k] - c0[k]) * (p[k] - c0[k])
    for k in range(3):
        b += (p[k] - c1[k]) * (p[k] - c1[k])
    d0, d1 = math.sqrt(a), math.sqrt(b)
    return (1 if d0 > d1 else 0), abs(d0 - d1)


def kmeans(pr, points):
    """runKmeans (:129-189) and KMeans::Cluster (Kmeans.cpp:61-100): (children, margin c); children is
    None when a seed does not exist."""
    cen = centre(points)

    def farthest(src):
        best, out = 0.0, None
        for p in points:
            d = norm3(p[0] - src[0], p[1] - src[1], p[2] - src[2])
            if d > best:
                best, out = d, p
        return out

    f = farthest(cen)
    ff = farthest(f) if f is not None else None
    if ff is None:
        return None, math.inf
    c0, c1, margin = list(f), list(ff), math.inf
    for _ in range(pr["kmeans_iters"]):
        mean, cnt = [[0.0] * 3, [0.0] * 3], [0, 0]
        labels = []
        for p in points:
            lab, gap = classify(p, c0, c1)
            labels.append(lab)
            margin = min(margin, gap)
        for j in range(2):  # (label by label, in index order: Kmeans.cpp:72-87)
            for p, lab in zip(points, labels):
                if lab == j:
                    for k in range(3):
                        mean[j][k] += p[k]
                    cnt[j] += 1
            if cnt[j]:
                mean[j] = [v / cnt[j] for v in mean[j]]
        c0, c1 = mean
    kids = ([], [])
    for p in points:
        lab, gap = classify(p, c0, c1)
        margin = min(margin, gap)
        kids[lab].append(p)
    return kids, margin


def cluster_cloud(pr, cloud):
    """obstacleClustering::run on a non-empty cloud of at most max_points points.  Returns a dict:
    flags, boxes (None with a flag) as (centroid, size, yaw) per leaf, labels, num_initial, margin c,
    depth (the deepest level at which a node was split, 0 = none)."""
    labels, ninit = dbscan_closed(cloud, pr["eps"], pr["min_pts"])
    out = dict(flags=0, boxes=None, labels=labels, num_initial=ninit, margin_c=math.inf, depth=0, splits=0)
    if ninit > pr["max_boxes"]:
        out["flags"] = FLAG_BOXES
        return out
    seq = [[p for p, lab in zip(cloud, labels) if lab == k] for k in range(ninit)]
    done = [False] * ninit
    for level in range(pr["tree_level"]):
        nseq, ndone, empty = [], [], False
        for pts, fin in zip(seq, done):
            if fin or orientation(pr, pts)[0] >= pr["density_thresh"]:
                nseq.append(pts)
                ndone.append(True)
                continue
            kids, gap = kmeans(pr, pts)
            out["margin_c"] = min(out["margin_c"], gap)
            out["depth"], out["splits"] = level + 1, out["splits"] + 1
            if kids is None or not kids[0] or not kids[1]:
                empty = True
                continue
            nseq += [kids[0], kids[1]]
            ndone += [False, False]
        if empty or len(nseq) > pr["max_boxes"]:
            out["flags"] = FLAG_EMPTY if empty else FLAG_BOXES
            return out
        seq, done = nseq, ndone
    boxes = []
    for pts in seq:
        _, lo, hi, angle = orientation(pr, pts)
        # bboxVertex (obstacleClustering.h:50-52) read by getStaticObstacles (:309-311)
        boxes.append(([(hi[k] + lo[k]) / 2.0 for k in range(3)], [hi[k] - lo[k] for k in range(3)], -angle))
    out["boxes"] = boxes
    return out


def new_state(I, pr):
    P, S = pr["max_points"], pr["max_boxes"]
    return dict(heading=np.zeros(I), count=np.zeros(I, np.int32), centroid=np.zeros((I, S, 3)),
                size=np.zeros((I, S, 3)), yaw=np.zeros((I, S)), flags=np.zeros(I, np.int32),
                num_points=np.zeros(I, np.int32), num_initial=np.zeros(I, np.int32), cloud=np.zeros((I, P, 3)),
                dbscan_label=np.zeros((I, P), np.int32))


def run(pr, m, map_max, occ, cur_pos, cur_vel, state, active=None, first=None):
    """One call of impc_cluster_run over every instance: `state` (new_state) is updated in place.
    Returns per instance a dict of margins and outcome facts (None for an inactive instance)."""
    facts = []
    P = pr["max_points"]
    for i in range(len(cur_pos)):
        if active is not None and not active[i]:
            facts.append(None)
            continue
        reg = region(pr, cur_pos[i], cur_vel[i], bool(first[i]) if first is not None else False,
                     float(state["heading"][i]))
        state["heading"][i] = reg[0]
        cloud, mb = scan(pr, reg, m, map_max, occ)
        f = dict(margin_a=reg[7], margin_b=mb, margin_c=math.inf, points=len(cloud), depth=0, splits=0, core=0,
                 contested=0, preceding=0, upper_face=0)
        facts.append(f)
        state["num_points"][i] = len(cloud)
        if not cloud or len(cloud) > P:
            state["flags"][i] = FLAG_POINTS if cloud else 0
            continue
        r = cluster_cloud(pr, cloud)
        f.update(margin_c=r["margin_c"], depth=r["depth"], splits=r["splits"])
        f["contested"], f["preceding"] = border_facts(cloud, pr["eps"], pr["min_pts"])
        f["core"] = sum(len(a) >= pr["min_pts"] for a in adjacency(cloud, pr["eps"]))
        f["upper_face"] = sum(any(p[k] == map_max[k] for k in range(3)) for p in cloud)
        state["cloud"][i, :len(cloud)] = cloud
        state["dbscan_label"][i, :len(cloud)] = r["labels"]
        state["num_initial"][i] = r["num_initial"]
        state["flags"][i] = r["flags"]
        if r["flags"]:
            continue
        state["count"][i] = len(r["boxes"])
        for k, (cen, size, yaw) in enumerate(r["boxes"]):
            state["centroid"][i, k], state["size"][i, k], state["yaw"][i, k] = cen, size, yaw
    return facts
