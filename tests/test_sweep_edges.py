"""What the default horizon's stage sweeps (mpc_wave.hpp sweep_pro / sweep_run, W = 19) do around their 19
steps: the sweeping wavefront forms its lane maps and store addresses and issues its first F reads in front
of the barrier that releases the sweep, and stores each capture register behind the last step that writes
it.  The seeded launches of test_sweep_step.py (12 + 12 QPs of N = 20, K = 8 with K = 9 grouped, forced to
three and to two teams per CU, and the 12-QP K = 3 one-tier case), at the places where that can go wrong:

* max_iter = 2 and 3: the prologue of iteration t + 1 is formed while iteration t's LDS is live;
* max_iter = 26 with the default check interval: a check at 25, then one more iteration across the pass
  boundary (begin_pass);
* a grouped launch of the N = 20, K = 8 batch with an N = 12 batch of the same kernel class: the
  runtime-horizon instance takes the unrolled sweep for the N = 20 batch and the lane grid for the other;
* a persistent workspace resumed after update_bounds_device: the resume refactors, so the first F reads
  follow a rewritten F.

Parity against the oracle (helpers.compare) and identical bytes at three and two teams per CU."""
import functools

import numpy as np
import pytest

import impc
from helpers import compare, oracle, take
from impc import scenarios
from oracle import osqp_oracle as ora
from test_sweep_step import CASES, ENV, NQ, _parity, _run, cases, solve

pytestmark = pytest.mark.gpu


def _same_bits(ra, rb):
    for (xa, ya, ia), (xb, yb, ib) in zip(ra, rb):
        assert xa.tobytes() == xb.tobytes() and ya.tobytes() == yb.tobytes()
        assert ia.tobytes() == ib.tobytes()  # every info field


@pytest.mark.parametrize("max_iter", [2, 3, 26])
@pytest.mark.parametrize("name", CASES)
def test_few_iterations_and_pass_boundary(ctx, monkeypatch, name, max_iter):
    r3, ref = _parity(ctx, monkeypatch, name, 3, max_iter=max_iter)
    assert all((o[2]["iter"] == max_iter).all() for o in ref)  # none of these QPs is solved that early
    r2, _ = _parity(ctx, monkeypatch, name, 2, max_iter=max_iter)
    _same_bits(r3, r2)


@functools.lru_cache(maxsize=None)
def _short():
    """12 QPs of N = 12, K = 8: another horizon in the kernel class of the N = 20, K = 8 batch."""
    return take(scenarios.intent_config(N=12, K=8, instances=6, hyps=8, seed=1212)[8], NQ)


def test_mixed_horizon_group(ctx, monkeypatch):
    monkeypatch.setenv(ENV, "2")
    s = impc.default_settings(verbose=0)
    long_, short = cases()["k8k9"][0], _short()
    alone, st_a = solve(ctx, (long_,), s)
    mixed, st_m = solve(ctx, (long_, short), s)
    # one launch for both (same team shape and row slots), so its horizon is a runtime value
    assert all(st_m[0][k] == st_m[1][k] for k in ("team_lanes", "var_slots", "row_slots")), st_m
    _same_bits(alone, mixed[:1])
    compare(mixed[1], oracle(short, s))


@pytest.mark.parametrize("per_cu", [3, 2])
def test_persistent_resume_after_bounds_update(ctx, monkeypatch, per_cu):
    monkeypatch.setenv(ENV, str(per_cu))
    cfg = cases()["k8k9"][0]
    s = impc.default_settings(verbose=0)
    pat, v = cfg["pattern"], cfg["values"]
    b = impc.Batch(ctx, pat["n"], pat["m"], pat["Pp"], pat["Pi"], pat["Ap"], pat["Ai"], NQ)
    keep = []
    try:
        b.set_kernel(impc.KERNEL_STRUCTURED)
        b.set_settings(s)
        b.set_values(v["Px"], v["q"], v["Ax"], v["l"], v["u"])
        if cfg.get("x_ws") is not None:
            b.warm_start(cfg["x_ws"], None)
        b.set_persistent(True)
        b.solve()
        r1 = b.get()
        keep = [impc.DeviceArray(ctx, np.ascontiguousarray(v[k])) for k in ("l", "u")]
        b.update_bounds_device(keep[0].ptr, keep[1].ptr)
        b.solve()
        r2 = b.get()
    finally:
        for d in keep:
            d.free()
        b.close()
    os_ = ora.settings_from(s)
    for i in range(NQ):
        w = ora.Workspace(pat, v["Px"][i], v["q"][i], v["Ax"][i], v["l"][i], v["u"][i], os_)
        if cfg.get("x_ws") is not None:
            w.warm_start(cfg["x_ws"][i], np.zeros(pat["m"]))
        refs = [w.solve()]
        w.update_bounds(v["l"][i], v["u"][i])
        refs.append(w.solve())
        w.close()
        for r, ref in zip((r1, r2), refs):
            compare((r[0][i:i + 1], r[1][i:i + 1], r[2][i:i + 1]),
                    (ref[0][None], ref[1][None], np.array([ref[2]], dtype=ref[2].dtype)))
