"""The three-teams-per-CU instance's iteration loop (mpc_wave.hpp WaveQP DENSE): the projection bounds,
q and the second products tier's geometry are per-pass copies, the rows' rho / 1/rho come from an LDS
table and one general entry's addresses are unpacked in the loop.  None of that may change a bit: every
case runs the same QPs at IMPC_TEAMS_PER_CU=3 and =2 (the two-per-CU instance keeps the plain forms),
asserts that three per CU was really taken, that x, y and every info field are byte-identical, and
helpers.compare against the oracle for every QP.

The dense instance exists for N = 20, two general-row slots and the two-tier layout: intent_config
buckets with K = 8 and K = 9, 48-64 QPs per case.

Cases: every class of bound through the clamp (box rows binding / l = u, general rows of both slots
two-sided and one-sided each way, built around the oracle's solution of the unmodified QP so that they
stay feasible); bounds updated on a persistent workspace from device memory; a grouped launch whose
workgroups change batch, in FIFO and longest-first order (the per-pass tier geometry follows the
pattern tables); a refactorisation between passes (the rho table is rewritten)."""
import functools

import numpy as np
import pytest

import impc
from helpers import compare, oracle, take
from impc import scenarios
from oracle import osqp_oracle as ora

pytestmark = pytest.mark.gpu

ENV = "IMPC_TEAMS_PER_CU"
NL = 256      # lanes per team: general row g sits in slot g // NL
SEED = 8212   # every rewritten QP of _classes() is solved by the oracle with this seed (asserted)
INF = 1e30    # OSQP_INFTY


@functools.lru_cache(maxsize=None)
def _buckets():
    # 24 instances x 8 hypotheses: 144 QPs with K = 8, 48 with K = 9
    return scenarios.intent_config(N=20, K=8, instances=24, hyps=8, seed=SEED)


def _settings(**kw):
    return impc.default_settings(verbose=0, **kw)


def _rows(pat):
    """(box rows, general rows in slot order) as mpc_structure.cpp assigns them: a variable's box row
    is its first single-entry row, every other row is general, in row order."""
    n, m = pat["n"], pat["m"]
    Ap, Ai = np.asarray(pat["Ap"]), np.asarray(pat["Ai"])
    col = np.repeat(np.arange(n), np.diff(Ap))
    cnt = np.bincount(Ai, minlength=m)
    first = np.full(m, -1)
    first[Ai[::-1]] = col[::-1]
    is_box, seen = np.zeros(m, bool), set()
    for i in range(m):
        if cnt[i] == 1 and int(first[i]) not in seen:
            seen.add(int(first[i]))
            is_box[i] = True
    assert len(seen) == n
    return np.flatnonzero(is_box), np.flatnonzero(~is_box)


def _ax(pat, Ax, x):
    n, m = pat["n"], pat["m"]
    Ap, Ai = np.asarray(pat["Ap"]), np.asarray(pat["Ai"])
    col = np.repeat(np.arange(n), np.diff(Ap))
    z = np.zeros((x.shape[0], m))
    for b in range(x.shape[0]):
        np.add.at(z[b], Ai, Ax[b] * x[b, col])
    return z


@functools.lru_cache(maxsize=None)
def _classes(K):
    """The K bucket with l, u rewritten around the oracle's solution z = A x of the unmodified QPs
    (x stays feasible).  Per QP, rows drawn at random from each group:
      box rows      u = z (binding, finite both sides) / l = z (binding) / l = u = z
      general rows  of slot 0 and of slot 1: two-sided finite [z - 0.5, z + 0.5], lower only
                    [z - 0.25, inf), upper only (-inf, z + 0.25], l = u = z kept where it was
    Returns (cfg, counts of each class per slot)."""
    nq = 64 if K == 8 else 48
    cfg = take(_buckets()[K], nq)
    pat, v = cfg["pattern"], cfg["values"]
    s = _settings()
    x0, _, i0 = oracle(cfg, s)
    assert np.isin(i0["status_val"], (1, 2)).all(), i0["status_val"]
    # (the solution meets its bounds to the solver's tolerance only: clipped, so that no rewritten
    # row ends with l > u)
    z = np.clip(_ax(pat, v["Ax"], x0), v["l"], v["u"])
    box, gen = _rows(pat)
    slot = np.arange(gen.size) // NL
    assert slot.max() == 1  # two general-row slots in use
    l, u = v["l"].copy(), v["u"].copy()
    rng = np.random.default_rng(SEED + K)
    seen = {k: 0 for k in ("box_u", "box_l", "box_eq", "g0_two", "g1_two", "g0_lo", "g1_lo", "g0_up", "g1_up")}
    for b in range(nq):
        fin = box[(l[b, box] > -INF * 1e-4) & (u[b, box] < INF * 1e-4) & (u[b, box] - l[b, box] > 1e-3)]
        pick = rng.choice(fin, 9, replace=False)
        u[b, pick[:3]] = z[b, pick[:3]]
        l[b, pick[3:6]] = z[b, pick[3:6]]
        l[b, pick[6:]] = u[b, pick[6:]] = z[b, pick[6:]]
        seen["box_u"] += 3
        seen["box_l"] += 3
        seen["box_eq"] += 3
        for sl in (0, 1):
            rows = gen[slot == sl]
            ineq = rows[u[b, rows] - l[b, rows] > 1e-3]  # the obstacle rows (the dynamics stay l = u)
            pick = rng.choice(ineq, 6, replace=False)
            two, lo, up = pick[:2], pick[2:4], pick[4:]
            l[b, two], u[b, two] = z[b, two] - 0.5, z[b, two] + 0.5
            l[b, lo], u[b, lo] = z[b, lo] - 0.25, INF
            l[b, up], u[b, up] = -INF, z[b, up] + 0.25
            seen[f"g{sl}_two"] += 2
            seen[f"g{sl}_lo"] += 2
            seen[f"g{sl}_up"] += 2
    assert all(c > 0 for c in seen.values()), seen
    assert ((l <= z) & (z <= u)).all()  # every rewritten row still contains the unmodified solution
    out = dict(cfg, values=dict(v, l=l, u=u))
    return out, seen


@functools.lru_cache(maxsize=None)
def _classes_ref(K, **kw):
    cfg, _ = _classes(K)
    ref = oracle(cfg, _settings(**kw))
    assert np.isin(ref[2]["status_val"], (1,)).all(), ref[2]["status_val"]  # every QP solved
    return ref


def _batch(ctx, cfg, settings):
    pat, v = cfg["pattern"], cfg["values"]
    b = impc.Batch(ctx, pat["n"], pat["m"], pat["Pp"], pat["Pi"], pat["Ap"], pat["Ai"], v["q"].shape[0])
    b.set_kernel(impc.KERNEL_STRUCTURED)
    b.set_settings(settings)
    b.set_values(v["Px"], v["q"], v["Ax"], v["l"], v["u"])
    if cfg.get("x_ws") is not None:
        b.warm_start(cfg["x_ws"], None)
    return b


def _solve(ctx, cfgs, settings, order=None):
    """One launch over cfgs (grouped when several); ([(x, y, info)], [teams per CU])."""
    batches = []
    try:
        for cfg in cfgs:
            batches.append(_batch(ctx, cfg, settings))
            if order is not None:
                batches[-1].set_queue_order(order)
        if len(batches) > 1:
            impc.solve_group(batches)
        else:
            batches[0].solve()
        return [b.get() for b in batches], [b.stats()["teams_per_cu"] for b in batches]
    finally:
        for b in batches:
            b.close()


def _same_bits(r2, r3):
    for (x2, y2, i2), (x3, y3, i3) in zip(r2, r3):
        assert x2.tobytes() == x3.tobytes() and y2.tobytes() == y3.tobytes()
        assert i2.tobytes() == i3.tobytes()  # every info field


def _both(ctx, monkeypatch, cfgs, settings, order=None):
    monkeypatch.setenv(ENV, "2")
    r2, t2 = _solve(ctx, cfgs, settings, order)
    monkeypatch.setenv(ENV, "3")
    r3, t3 = _solve(ctx, cfgs, settings, order)
    assert all(t == 2 for t in t2), t2
    assert all(t == 3 for t in t3), t3  # the dense instance was really taken
    _same_bits(r2, r3)
    return r3


@pytest.mark.parametrize("K", [8, 9])
def test_every_class_of_bound_reaches_the_clamp(ctx, monkeypatch, K):
    cfg, _ = _classes(K)
    r3 = _both(ctx, monkeypatch, [cfg], _settings())
    compare(r3[0], _classes_ref(K))


@pytest.mark.parametrize("K", [8, 9])
def test_refactorisation_between_passes(ctx, monkeypatch, K):
    kw = dict(adaptive_rho_interval=25, adaptive_rho_tolerance=1.0001)
    cfg, _ = _classes(K)
    ref = _classes_ref(K, **kw)
    assert (ref[2]["rho_updates"] >= 1).all()  # every QP refactors (and rewrites the rho table)
    r3 = _both(ctx, monkeypatch, [cfg], _settings(**kw))
    compare(r3[0], ref)
    assert np.array_equal(r3[0][2]["rho_updates"], ref[2]["rho_updates"])


def _tightened(cfg):
    """Finite two-sided box bounds pulled in by 10 % of their width, one-sided general rows raised."""
    v = cfg["values"]
    l, u = v["l"].copy(), v["u"].copy()
    fin = (l > -INF * 1e-4) & (u < INF * 1e-4) & (u - l > 1e-3)
    w = u - l
    l[fin] += 0.1 * w[fin]
    u[fin] -= 0.1 * w[fin]
    return l, u


def _persistent_sequence(ctx, cfg, settings, l2, u2):
    b = _batch(ctx, cfg, settings)
    keep = []
    try:
        b.set_persistent(True)
        b.solve()
        first = b.get()
        keep = [impc.DeviceArray(ctx, np.ascontiguousarray(a)) for a in (l2, u2)]
        b.update_bounds_device(keep[0].ptr, keep[1].ptr)
        b.solve()
        return first, b.get(), b.stats()["teams_per_cu"]
    finally:
        for k in keep:
            k.free()
        b.close()


@pytest.mark.parametrize("K", [8, 9])
def test_bounds_updated_on_a_persistent_workspace(ctx, monkeypatch, K):
    cfg = take(_buckets()[K], 48)
    s = _settings()
    l2, u2 = _tightened(cfg)
    monkeypatch.setenv(ENV, "2")
    a2, b2, t2 = _persistent_sequence(ctx, cfg, s, l2, u2)
    monkeypatch.setenv(ENV, "3")
    a3, b3, t3 = _persistent_sequence(ctx, cfg, s, l2, u2)
    assert t2 == 2 and t3 == 3, (t2, t3)
    _same_bits([a2, b2], [a3, b3])
    # the oracle's osqp_setup -> [warm start] -> solve -> osqp_update_bounds -> solve, per QP
    pat, v = cfg["pattern"], cfg["values"]
    os_ = ora.settings_from(s)
    nq = v["q"].shape[0]
    xo, yo = np.empty((nq, pat["n"])), np.empty((nq, pat["m"]))
    io = np.empty(nq, dtype=impc.INFO_DTYPE)
    for i in range(nq):
        w = ora.Workspace(pat, v["Px"][i], v["q"][i], v["Ax"][i], v["l"][i], v["u"][i], os_)
        if cfg.get("x_ws") is not None:
            w.warm_start(cfg["x_ws"][i], np.zeros(pat["m"]))
        w.solve()
        w.update_bounds(l2[i], u2[i])
        xo[i], yo[i], info = w.solve()
        for f in io.dtype.names:
            io[f][i] = info[f]
        w.close()
    compare(b3, (xo, yo, io))


@pytest.mark.parametrize("order", [impc.QUEUE_FIFO, impc.QUEUE_LONGEST_FIRST], ids=["fifo", "longest-first"])
def test_grouped_launch_changes_batch(ctx, monkeypatch, order):
    """40 K = 8 and 24 K = 9 QPs in one solve_group: a workgroup that crosses from one batch to the
    other reloads the pattern tables, and the second tier's row length and addresses with them."""
    bks = _buckets()
    cfgs = [take(bks[8], 40), take(bks[9], 24)]
    s = _settings()
    grouped = _both(ctx, monkeypatch, cfgs, s, order)
    monkeypatch.setenv(ENV, "3")
    for cfg, res in zip(cfgs, grouped):
        alone, t = _solve(ctx, [cfg], s, order)
        assert t == [3], t
        _same_bits(alone, [res])
        compare(res, oracle(cfg, s))
