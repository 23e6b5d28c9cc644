"""The compile-time stage sweeps of the default horizon (mpc_wave.hpp sweep_mfma, W = 19: N = 20) at the
smallest launches that reach them: seeded intent_config buckets of 12 QPs, K = 8 with K = 9 in one
grouped launch (the two-tier, two-slot instance, forced to three and to two teams per CU as
test_teams_per_cu.py does) and K = 3 alone (the one-tier instance, two per CU under either value).

A sweep keeps step m's result in one lane per element and stores the 19 steps after the last one, reads
(F, c) some steps ahead of their use, and writes the slots no step owns to discard slots.  What can go
wrong there shows as a stage stored to the wrong slot, a step lost, or a read of F that a
refactorisation has since rewritten:

* max_iter = 1 isolates one linear solve: a stage in the wrong slot cannot hide behind convergence;
* default settings: the full solve;
* the two forced occupancies give the same bits;
* a short adaptive_rho_interval refactors mid-solve, so the reads ahead see a rewritten F;
* tests/golden/sweep_step_parent.npz holds x, y, iterations and status of the same 36 QPs as the
  library computed them before the sweep's instructions were reordered (tools/sweep_step_golden.py
  wrote it on an MI355X): byte equality, the seconds-long stand-in for comparing the benchmark's dumped
  outputs."""
import functools
import os

import numpy as np
import pytest

import impc
from helpers import compare, oracle, take
from impc import scenarios

pytestmark = pytest.mark.gpu

ENV = "IMPC_TEAMS_PER_CU"
NQ = 12
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_step_parent.npz")
CASES = ("k8k9", "k3")


@functools.lru_cache(maxsize=None)
def cases():
    """name -> the configs of one launch (a grouped launch when there are two)."""
    bks = scenarios.intent_config(N=20, K=8, instances=6, hyps=8, seed=1108)   # 36 QPs with K = 8, 12 with K = 9
    one = scenarios.intent_config(N=20, K=3, instances=2, hyps=8, seed=1103)   # 12 QPs with K = 3
    return {"k8k9": (take(bks[8], NQ), take(bks[9], NQ)), "k3": (take(one[3], NQ),)}


def solve(ctx, cfgs, settings):
    """One (grouped) launch over cfgs: ([(x, y, info)], [stats])."""
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


def golden_arrays(name, res):
    """The arrays the golden file keeps of launch `name`."""
    out = {}
    for k, (x, y, info) in enumerate(res):
        out.update({f"{name}_{k}_x": x, f"{name}_{k}_y": y, f"{name}_{k}_iter": info["iter"],
                    f"{name}_{k}_status": info["status_val"]})
    return out


@functools.lru_cache(maxsize=None)
def _ref(name, kw):
    s = impc.default_settings(verbose=0, **dict(kw))
    return tuple(oracle(cfg, s) for cfg in cases()[name])


def _run(ctx, monkeypatch, name, per_cu, **kw):
    monkeypatch.setenv(ENV, str(per_cu))
    cfgs = cases()[name]
    assert all(c["values"]["q"].shape[0] == NQ for c in cfgs)
    res, st = solve(ctx, cfgs, impc.default_settings(verbose=0, **kw))
    want = per_cu if name == "k8k9" else 2  # the one-tier instance is built for two per CU only
    assert all(s["kernel"] == impc.KERNEL_STRUCTURED and s["teams_per_cu"] == want for s in st), st
    return res


def _parity(ctx, monkeypatch, name, per_cu, **kw):
    res = _run(ctx, monkeypatch, name, per_cu, **kw)
    ref = _ref(name, tuple(sorted(kw.items())))
    for r, o in zip(res, ref):
        compare(r, o)
    return res, ref


@pytest.mark.parametrize("per_cu", [3, 2])
@pytest.mark.parametrize("name", CASES)
def test_one_iteration(ctx, monkeypatch, name, per_cu):
    res, ref = _parity(ctx, monkeypatch, name, per_cu, max_iter=1)
    assert all((o[2]["iter"] == 1).all() for o in ref)


@pytest.mark.parametrize("per_cu", [3, 2])
@pytest.mark.parametrize("name", CASES)
def test_default_settings(ctx, monkeypatch, name, per_cu):
    _parity(ctx, monkeypatch, name, per_cu)


@pytest.mark.parametrize("kw", [dict(max_iter=1), dict()], ids=["one-iteration", "default"])
@pytest.mark.parametrize("name", CASES)
def test_two_and_three_per_cu_same_bits(ctx, monkeypatch, name, kw):
    r3 = _run(ctx, monkeypatch, name, 3, **kw)
    r2 = _run(ctx, monkeypatch, name, 2, **kw)
    for (x2, y2, i2), (x3, y3, i3) in zip(r2, r3):
        assert x2.tobytes() == x3.tobytes() and y2.tobytes() == y3.tobytes()
        assert i2.tobytes() == i3.tobytes()  # every info field


@pytest.mark.parametrize("per_cu", [3, 2])
@pytest.mark.parametrize("name", CASES)
def test_refactorisation_mid_solve(ctx, monkeypatch, name, per_cu):
    res, ref = _parity(ctx, monkeypatch, name, per_cu, adaptive_rho_interval=10, adaptive_rho_tolerance=1.0001)
    for r, o in zip(res, ref):
        assert (o[2]["rho_updates"] >= 1).all()  # every QP refactors, and goes on iterating after it
        assert (o[2]["iter"] > 10).all()
        assert np.array_equal(r[2]["rho_updates"], o[2]["rho_updates"])


@pytest.mark.parametrize("per_cu", [3, 2])
@pytest.mark.parametrize("name", CASES)
def test_unchanged_results(ctx, monkeypatch, name, per_cu):
    res = _run(ctx, monkeypatch, name, per_cu)
    with np.load(GOLDEN, allow_pickle=False) as z:
        for key, a in golden_arrays(name, res).items():
            g = z[key]
            assert a.dtype == g.dtype and a.shape == g.shape, key
            assert a.tobytes() == g.tobytes(), key
