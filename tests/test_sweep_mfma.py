"""The default-horizon stage recursions on the four-block FP64 matrix instruction (mpc_wave.hpp
sweep_mfma: every instance with a compile-time horizon W = 19) against the oracle, with the project's
rule (helpers.compare: identical status and iteration count, x, y and obj within 1e-5):

* the grouped K = 8 / K = 9 launch on the two-tier instance, built for two and for three teams per CU,
* the one-tier instance (K = 3) and the three general-row slots (K = 19),
* a runtime horizon (N = 10), whose sweeps stay on the lane grid but read the same stored -F,
* a refactorisation between passes (F is rewritten), and
* the exits around the sweeps: the infeasible and max-iter golden vectors and max_iter = 1."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import impc
from helpers import compare, oracle, take
from impc import scenarios

pytestmark = pytest.mark.gpu

ENV = "IMPC_TEAMS_PER_CU"
NQ = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _buckets(N, K, instances, seed):
    return scenarios.intent_config(N=N, K=K, instances=instances, hyps=8, seed=seed)


@functools.lru_cache(maxsize=None)
def _bucket(N, K, seed):
    """NQ QPs with K obstacle trajectories (six of an instance's eight hypotheses carry K)."""
    return take(_buckets(N, K, (NQ + 5) // 6, seed)[K], NQ)


def _solve(ctx, cfgs, settings):
    batches = []
    try:
        for cfg in cfgs:
            pat, v = cfg["pattern"], cfg["values"]
            b = impc.Batch(ctx, pat["n"], pat["m"], pat["Pp"], pat["Pi"], pat["Ap"], pat["Ai"], v["q"].shape[0])
            batches.append(b)
            b.set_kernel(impc.KERNEL_STRUCTURED)
            b.set_settings(settings)
            b.set_values(v["Px"], v["q"], v["Ax"], v["l"], v["u"])
            if cfg.get("x_ws") is not None:
                b.warm_start(cfg["x_ws"], None)
        if len(batches) > 1:
            impc.solve_group(batches)
        else:
            batches[0].solve()
        return [b.get() for b in batches], [b.stats() for b in batches]
    finally:
        for b in batches:
            b.close()


@functools.lru_cache(maxsize=None)
def _grouped():
    bks = _buckets(20, 8, 16, 9100)  # 96 QPs with K = 8 and 32 with K = 9: 128 in one grouped launch
    cfgs = [bks[8], bks[9]]
    assert sum(c["values"]["q"].shape[0] for c in cfgs) == 128
    return cfgs, [oracle(c, impc.default_settings(verbose=0)) for c in cfgs]


@pytest.mark.parametrize("teams", [2, 3])
def test_grouped_k8_k9_two_tier(ctx, monkeypatch, teams):
    monkeypatch.setenv(ENV, str(teams))
    cfgs, refs = _grouped()
    res, st = _solve(ctx, cfgs, impc.default_settings(verbose=0))
    assert all(s["kernel"] == impc.KERNEL_STRUCTURED and s["teams_per_cu"] == teams for s in st), st
    for r, ref in zip(res, refs):
        compare(r, ref)


@pytest.mark.parametrize("N,K,seed", [(20, 3, 9103), (20, 19, 9119), (10, 8, 9110)],
                         ids=["K3-one-tier", "K19-three-row-slots", "N10-runtime-W-lane-grid"])
def test_other_instances(ctx, N, K, seed):
    cfg = _bucket(N, K, seed)
    s = impc.default_settings(verbose=0)
    res, st = _solve(ctx, [cfg], s)
    assert st[0]["kernel"] == impc.KERNEL_STRUCTURED, st
    if K == 19:
        assert st[0]["row_slots"] == 3, st
    compare(res[0], oracle(cfg, s))


def test_refactorisation_rewrites_f(ctx):
    cfg = _bucket(20, 8, 9101)
    s = impc.default_settings(verbose=0, adaptive_rho_interval=25, adaptive_rho_tolerance=1.0001)
    res, _ = _solve(ctx, [cfg], s)
    ref = oracle(cfg, s)
    assert (ref[2]["rho_updates"] >= 1).all()
    compare(res[0], ref)
    assert np.array_equal(res[0][2]["rho_updates"], ref[2]["rho_updates"])


def test_ends_on_first_iteration(ctx):
    cfg = _bucket(20, 8, 9101)
    s = impc.default_settings(verbose=0, max_iter=1)
    res, _ = _solve(ctx, [cfg], s)
    ref = oracle(cfg, s)
    assert (ref[2]["iter"] == 1).all()
    compare(res[0], ref)


def _golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    pat = dict(n=int(z["n"]), m=int(z["m"]), Pp=z["Pp"], Pi=z["Pi"], Ap=z["Ap"], Ai=z["Ai"])
    s = impc.Settings()
    for (f, t), v in zip(impc.Settings._fields_, z["settings"]):
        setattr(s, f, float(v) if t is C.c_double else int(v))
    info = np.zeros(z["iter"].shape[0], dtype=impc.INFO_DTYPE)
    info["iter"], info["status_val"], info["obj_val"] = z["iter"], z["status_val"], z["obj_val"]
    info["rho_updates"] = z["rho_updates"]
    cfg = dict(pattern=pat, values={k: z[k] for k in ("Px", "q", "Ax", "l", "u")},
               x_ws=z["x_ws"] if z["x_ws"].size else None)
    return cfg, s, (z["x"], z["y"], info)


@pytest.mark.parametrize("name", ["G6_infeasible", "G7_max_iter"])
def test_golden_exits(ctx, name):
    cfg, s, ref = _golden(name)
    res, _ = _solve(ctx, [cfg], s)
    compare(res[0], ref)
