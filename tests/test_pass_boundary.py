"""The structured kernel's pass boundary (mpc_wave.hpp solve(): the termination check, the rho
estimate / update and the products rewrite between two passes of the ADMM iteration loop) on the
one-variable-per-lane team shape, against the oracle: identical status and iteration count, x / y /
objective within 1e-5 relative (helpers.compare).

Every check goes through the team reduction (GpuTeam::reduce: 17 maxima and 2 sums combined across
the wavefronts in one lane per value), whose results decide status and iteration count.

The cases are the smallest that reach each path of the boundary: the compile-time-horizon instance
(N = 20; K = 0 and K = 8), its two-tier products instance (K = 20) and the runtime-horizon instance
(N = 5); a solve that ends one iteration before, on and one after a check (max_iter 24 / 25 / 26: the
post-loop update_info, the in-loop one, and a pass of one iteration) and on the second check (50); rho-only
boundaries (adaptive_rho_interval != check_termination); a forced rho update with its
refactorisation; a per-QP time limit that never binds (the time-limit form of the passes); a resumed
persistent workspace.  8-12 QPs each, the oracle's results computed once per case."""
import functools

import numpy as np
import pytest

import impc
from helpers import compare, gpu, oracle
from impc import scenarios
from oracle import osqp_oracle as ora

pytestmark = pytest.mark.gpu

B = 8
BASE = dict(verbose=0, adaptive_rho_interval=25)


@functools.lru_cache(maxsize=None)
def _cfg(N, K, seed):
    return scenarios.static_config(N=N, K=K, batch=B, identical=False, seed=seed)


@functools.lru_cache(maxsize=None)
def _ref(N, K, seed, items):
    return oracle(_cfg(N, K, seed), impc.default_settings(**dict(items)))


def _settings(**kw):
    items = tuple(sorted({**BASE, **kw}.items()))
    return impc.default_settings(**dict(items)), items


def _check(ctx, N, K, seed, **kw):
    s, items = _settings(**kw)
    ref = _ref(N, K, seed, items)
    assert np.isin(ref[2]["status_val"], (1, 2, -2)).all(), ref[2]["status_val"]  # the oracle has a solution
    res = gpu(ctx, _cfg(N, K, seed), s, impc.KERNEL_STRUCTURED)
    compare(res, ref)
    return res, ref


@pytest.mark.parametrize("N,K,seed", [(20, 0, 7100), (20, 8, 7101), (20, 20, 7102), (5, 2, 7103)],
                         ids=["N20-K0", "N20-K8", "N20-K20-two-tier", "N5-K2-runtime-W"])
def test_instances(ctx, N, K, seed):
    res, ref = _check(ctx, N, K, seed)
    assert (ref[2]["iter"] >= 25).all()  # every QP passes at least one check


@pytest.mark.parametrize("max_iter", [24, 25, 26, 50])
def test_solve_ends_around_a_check(ctx, max_iter):
    res, ref = _check(ctx, 20, 8, 7101, max_iter=max_iter)
    assert (ref[2]["iter"] == max_iter).all()  # none of these QPs is solved that early


def test_rho_only_boundaries(ctx):
    # rho estimates at 10, 20, 30, ... between the checks at 25, 50, ...; both at once at 50, 100, ...
    _check(ctx, 20, 8, 7101, adaptive_rho_interval=10)


def test_forced_rho_update_and_refactorisation(ctx):
    # a first rho far from the estimate: every QP updates rho (and refactors) at its first boundary
    res, ref = _check(ctx, 20, 8, 7101, rho=1e-3)
    assert (ref[2]["rho_updates"] >= 1).all()
    assert np.array_equal(res[2]["rho_updates"], ref[2]["rho_updates"])


def test_time_limit_that_never_binds(ctx):
    cfg = _cfg(20, 8, 7101)
    s, items = _settings()
    pat, v = cfg["pattern"], cfg["values"]
    b = impc.Batch(ctx, pat["n"], pat["m"], pat["Pp"], pat["Pi"], pat["Ap"], pat["Ai"], B)
    try:
        b.set_kernel(impc.KERNEL_STRUCTURED)
        b.set_settings(s)
        b.set_values(v["Px"], v["q"], v["Ax"], v["l"], v["u"])
        b.set_time_limits(np.full(B, 100.0))
        b.solve()
        res = b.get()
    finally:
        b.close()
    compare(res, _ref(20, 8, 7101, items))


def test_persistent_resume(ctx):
    cfg = _cfg(20, 8, 7101)
    s, _ = _settings()
    pat, v = cfg["pattern"], cfg["values"]
    q2 = v["q"] * (1 + 0.05 * np.random.default_rng(7).standard_normal(v["q"].shape))
    b = impc.Batch(ctx, pat["n"], pat["m"], pat["Pp"], pat["Pi"], pat["Ap"], pat["Ai"], B)
    try:
        b.set_kernel(impc.KERNEL_STRUCTURED)
        b.set_settings(s)
        b.set_values(v["Px"], v["q"], v["Ax"], v["l"], v["u"])
        b.set_persistent(True)
        b.solve()
        r1 = b.get()
        b.update_lin_cost(q2)
        b.solve()
        r2 = b.get()
    finally:
        b.close()
    os_ = ora.settings_from(s)
    for i in range(B):
        w = ora.Workspace(pat, v["Px"][i], v["q"][i], v["Ax"][i], v["l"][i], v["u"][i], os_)
        refs = [w.solve()]
        w.update_lin_cost(q2[i])
        refs.append(w.solve())
        w.close()
        for r, ref in zip((r1, r2), refs):
            assert ref[2]["status_val"] in (1, 2)
            compare((r[0][i:i + 1], r[1][i:i + 1], r[2][i:i + 1]),
                    (ref[0][None], ref[1][None], np.array([ref[2]], dtype=ref[2].dtype)))
