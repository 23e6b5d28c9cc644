"""The entry points that put values into a batch, host against device: impc_batch_set_values,
_warm_start, _update_lin_cost, _update_bounds and _update_matrices each have a _device twin that
takes the same numbers from device memory.  Two batches of one size are fed the same numbers, one
through the host calls and one through the twins, and every solve along the way must agree bit for
bit: x, y and every field of the info records.  Then the state rules the two share: which calls
end a persistent workspace's resumability, and which error a bad call gets first.

Four N = 20, K = 2 QPs per batch, except the case just over the pinned-staging limit, where the
host calls leave their staged arm (a few hundred QPs, the four tiled)."""
import numpy as np
import pytest

import impc
from helpers import HAS_SOLUTION
from impc import scenarios

pytestmark = pytest.mark.gpu

# include/impc_qp.h
DATA_VALIDATION_ERROR, WORKSPACE_NOT_INIT_ERROR, UNSUPPORTED = 1, 7, 102

KERNELS = pytest.mark.parametrize("kernel", [impc.KERNEL_GENERIC, impc.KERNEL_STRUCTURED],
                                  ids=["generic", "structured"])
DUALS = pytest.mark.parametrize("duals", [True, False], ids=["x-y", "x-only"])


@pytest.fixture(scope="module")
def case():
    """The four QPs and the values the updates replace theirs with (read-only)."""
    cfg = scenarios.static_config(N=20, K=2, batch=4, identical=False, seed=1701)
    pat, v = cfg["pattern"], cfg["values"]
    rng = np.random.default_rng(17)
    c = dict(pat=pat, v={k: np.ascontiguousarray(a, dtype=np.float64) for k, a in v.items()})
    c["q2"] = v["q"] * (1 + 0.05 * rng.standard_normal(v["q"].shape))
    c["q5"] = v["q"] * (1 + 0.3 * rng.standard_normal(v["q"].shape))
    l3, u3 = v["l"].copy(), v["u"].copy()
    fin = np.isfinite(l3) & np.isfinite(u3) & (u3 - l3 > 1e-3)
    l3[fin] -= 0.05
    u3[fin] += 0.05
    c["l3"], c["u3"] = l3, u3
    c["P3"] = v["Px"] * (1.0 + 0.5 * rng.uniform(size=v["Px"].shape))
    c["A3"] = v["Ax"] * (1.0 + 0.02 * rng.standard_normal(v["Ax"].shape))
    c["xw"] = 0.1 * rng.standard_normal(v["q"].shape)
    c["yw"] = 0.01 * rng.standard_normal(v["l"].shape)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    for a in c["v"].values():
        a.setflags(write=False)
    return c


class Feed:
    """One batch, fed through the host entry points (dev = False) or through their _device twins
    from device copies of the same arrays (dev = True)."""

    def __init__(self, ctx, pat, B, dev, kernel=impc.KERNEL_AUTO):
        self.ctx, self.dev, self.keep = ctx, dev, []
        self.b = impc.Batch(ctx, pat["n"], pat["m"], pat["Pp"], pat["Pi"], pat["Ap"], pat["Ai"], B)
        self.b.set_kernel(kernel)
        self.b.set_settings(impc.default_settings(verbose=0, adaptive_rho_interval=25))

    def ptr(self, a):
        if a is None:
            return None
        self.keep.append(impc.DeviceArray(self.ctx, np.ascontiguousarray(a, dtype=np.float64)))
        return self.keep[-1].ptr

    def set_values(self, Px, q, Ax, l, u):
        if self.dev:
            self.b.set_values_device(*[self.ptr(a) for a in (Px, q, Ax, l, u)])
        else:
            self.b.set_values(Px, q, Ax, l, u)

    def warm_start(self, x, y):
        if self.dev:
            self.b.warm_start_device(self.ptr(x), self.ptr(y))
        else:
            self.b.warm_start(x, y)

    def update_lin_cost(self, q):
        if self.dev:
            self.b.update_lin_cost_device(self.ptr(q))
        else:
            self.b.update_lin_cost(q)

    def update_bounds(self, l, u):
        if self.dev:
            self.b.update_bounds_device(self.ptr(l), self.ptr(u))
        else:
            self.b.update_bounds(l, u)

    def update_matrices(self, Px, Ax):
        if self.dev:
            self.b.update_matrices_device(self.ptr(Px), self.ptr(Ax))
        else:
            self.b.update_matrices(Px, Ax)

    def solve(self):
        self.b.solve()
        return self.b.get()

    def close(self):
        self.b.close()
        for d in self.keep:
            d.free()


def both(ctx, pat, B, kernel, script):
    """script(feed) -> the list of its solves' results; run on a host-fed and on a device-fed batch,
    the two lists bit for bit equal.  Returns the host-fed one."""
    runs = []
    for dev in (False, True):
        f = Feed(ctx, pat, B, dev, kernel)
        try:
            assert f.b.stats()["kernel"] == kernel
            runs.append(script(f))
        finally:
            f.close()
    assert len(runs[0]) == len(runs[1]) > 0
    for step, ((xh, yh, ih), (xd, yd, idv)) in enumerate(zip(*runs)):
        print(f"solve {step}: status {ih['status_val'].tolist()[:8]} iter {ih['iter'].tolist()[:8]}")
        np.testing.assert_array_equal(xh.view(np.uint64), xd.view(np.uint64), err_msg=f"x, solve {step}")
        np.testing.assert_array_equal(yh.view(np.uint64), yd.view(np.uint64), err_msg=f"y, solve {step}")
        for name in ih.dtype.names:
            assert ih[name].tobytes() == idv[name].tobytes(), (step, name, ih[name], idv[name])
    # the comparison is of solves, not of two batches that both failed to start
    assert np.isin(runs[0][0][2]["status_val"], HAS_SOLUTION).all(), runs[0][0][2]["status_val"]
    return runs[0]


def base(c):
    v = c["v"]
    return v["Px"], v["q"], v["Ax"], v["l"], v["u"]


def test_generic_updates(ctx, case):
    """Set-up generic workspace: q, then the bounds, replaced in place (interleave + k_update_*)."""
    def script(f):
        f.set_values(*base(case))
        out = [f.solve()]
        f.update_lin_cost(case["q2"])
        out.append(f.solve())
        f.update_bounds(case["l3"], case["u3"])
        out.append(f.solve())
        return out
    r = both(ctx, case["pat"], 4, impc.KERNEL_GENERIC, script)
    assert not np.array_equal(r[0][0], r[1][0]) and not np.array_equal(r[1][0], r[2][0])  # the updates arrived


@DUALS
def test_generic_warm_start_in_place(ctx, case, duals):
    """After a solve the generic workspace takes a warm start in place (k_warm_start), with duals or
    with y = 0."""
    def script(f):
        f.set_values(*base(case))
        out = [f.solve()]
        f.update_lin_cost(case["q2"])
        f.warm_start(out[0][0] * 1.01, out[0][1] * 0.99 if duals else None)
        out.append(f.solve())
        return out
    both(ctx, case["pat"], 4, impc.KERNEL_GENERIC, script)


@pytest.mark.parametrize("which", ["A", "P", "PA", "shared-A", "shared-P"])
def test_structured_matrix_updates(ctx, case, which):
    """Persistent structured workspace: new A and / or P values, then a q update after them (the
    q_after / d_qsnap path), then new bounds.  shared-*: the batch's values came from
    impc_batch_set_values_shared, so the update first expands them into the per-QP arrays."""
    v = case["v"]
    new = which.split("-")[-1]
    P3 = case["P3"] if "P" in new else None
    A3 = case["A3"] if "A" in new else None
    split = impc.shared_split(v["Px"], v["Ax"])
    assert split is not None and split[2].size > 0

    def script(f):
        if which.startswith("shared"):
            f.b.set_values_shared(split[0], split[1], split[2], split[3], v["q"], v["l"], v["u"])
        else:
            f.set_values(*base(case))
        f.b.set_persistent(True)
        out = [f.solve()]
        f.update_matrices(P3, A3)
        f.update_lin_cost(case["q5"])
        out.append(f.solve())
        f.update_bounds(case["l3"], case["u3"])
        out.append(f.solve())
        return out
    r = both(ctx, case["pat"], 4, impc.KERNEL_STRUCTURED, script)
    assert not np.array_equal(r[0][0], r[1][0]) and not np.array_equal(r[1][0], r[2][0])


@KERNELS
@DUALS
def test_first_values_and_warm_start(ctx, case, kernel, duals):
    """Before the first solve: the host calls stage four QPs in pinned memory, the twins copy."""
    def script(f):
        f.set_values(*base(case))
        f.warm_start(case["xw"], case["yw"] if duals else None)
        return [f.solve()]
    both(ctx, case["pat"], 4, kernel, script)


def over_staging_limit(pat):
    """The smallest batch whose inputs, warm start and results no longer fit the 8 MiB of pinned
    staging (impc_qp.hip stage_len: per QP the five input arrays, x and y twice, one info record)."""
    n, m = pat["n"], pat["m"]
    nnzP, nnzA = int(pat["Pp"][-1]), int(pat["Ap"][-1])
    per_qp = (nnzP + n + nnzA + 2 * m) + 2 * (n + m) + impc.INFO_DTYPE.itemsize // 8
    return (8 << 20) // 8 // per_qp + 1


@KERNELS
def test_values_and_warm_start_over_the_staging_limit(ctx, case, kernel):
    """A batch one QP past the staging limit: impc_batch_set_values and _warm_start upload each
    array on its own here, the arm four QPs never reach."""
    B = over_staging_limit(case["pat"])
    assert 100 < B < 1000, B
    tile = lambda a: np.ascontiguousarray(np.tile(a, (B // 4 + 1, 1))[:B])  # noqa: E731
    vals = [tile(a) for a in base(case)]
    xw, yw = tile(case["xw"]), tile(case["yw"])

    def script(f):
        f.set_values(*vals)
        f.warm_start(xw, yw)
        return [f.solve()]
    r = both(ctx, case["pat"], B, kernel, script)
    assert np.array_equal(r[0][0][:4], r[0][0][4:8])  # tiled in, tiled out


def persistent_solved(ctx, case):
    f = Feed(ctx, case["pat"], 4, False, impc.KERNEL_STRUCTURED)
    f.set_values(*base(case))
    f.b.set_persistent(True)
    f.solve()
    return f


@pytest.mark.parametrize("how", ["set_values", "set_values_device", "set_settings", "set_active", "set_persistent"])
def test_calls_that_end_resumability(ctx, case, how):
    """After any of these the persistent workspace no longer matches the batch: an update is refused
    until a solve has set it up again."""
    f = persistent_solved(ctx, case)
    try:
        f.update_lin_cost(case["q2"])  # resumable now
        if how == "set_values":
            f.b.set_values(*base(case))
        elif how == "set_values_device":
            f.b.set_values_device(*[f.ptr(a) for a in base(case)])
        elif how == "set_settings":
            f.b.set_settings(impc.default_settings(verbose=0, adaptive_rho_interval=25, rho=0.2))
        elif how == "set_active":
            f.b.set_active(3)
        else:
            f.b.set_persistent(True)
        with pytest.raises(impc.ImpcError) as e:
            f.update_lin_cost(case["q2"])
        assert e.value.code == WORKSPACE_NOT_INIT_ERROR
        f.solve()
        f.update_lin_cost(case["q2"])
        f.update_bounds(case["l3"], case["u3"])
    finally:
        f.close()


def crossed(case):
    """The lower bounds with l > u at (QP 2, row 5)."""
    l = case["v"]["l"].copy()
    assert np.isfinite(case["v"]["u"][2, 5])
    l[2, 5] = case["v"]["u"][2, 5] + 1.0
    return l


def test_first_error_of_a_bad_call(ctx, case):
    v = case["v"]
    f = Feed(ctx, case["pat"], 4, False, impc.KERNEL_STRUCTURED)
    try:
        f.set_values(*base(case))
        f.solve()
        with pytest.raises(impc.ImpcError) as e:  # structured, not persistent
            f.update_lin_cost(case["q2"])
        assert e.value.code == WORKSPACE_NOT_INIT_ERROR and "impc_batch_set_persistent" in str(e.value)
        with pytest.raises(impc.ImpcError) as e:  # crossed bounds with the values
            f.b.set_values(v["Px"], v["q"], v["Ax"], crossed(case), v["u"])
        assert e.value.code == DATA_VALIDATION_ERROR
        assert "lower bound greater than upper bound (QP 2, row 5)" in str(e.value)
    finally:
        f.close()
    g = Feed(ctx, case["pat"], 4, False, impc.KERNEL_GENERIC)
    try:
        g.set_values(*base(case))
        with pytest.raises(impc.ImpcError) as e:  # generic, before setup; the crossed bounds are not looked at yet
            g.update_bounds(crossed(case), v["u"])
        assert e.value.code == WORKSPACE_NOT_INIT_ERROR and "setup has not run" in str(e.value)
        with pytest.raises(impc.ImpcError) as e:
            g.update_matrices(None, case["A3"])
        assert e.value.code == UNSUPPORTED
    finally:
        g.close()


@KERNELS
def test_crossed_bounds_in_an_update(ctx, case, kernel):
    f = Feed(ctx, case["pat"], 4, False, kernel)
    try:
        f.set_values(*base(case))
        if kernel == impc.KERNEL_STRUCTURED:
            f.b.set_persistent(True)
        f.solve()
        with pytest.raises(impc.ImpcError) as e:
            f.update_bounds(crossed(case), case["v"]["u"])
        assert e.value.code == DATA_VALIDATION_ERROR and "lower bound greater than upper bound" in str(e.value)
    finally:
        f.close()


@KERNELS
def test_crossed_bounds_in_an_update_name_qp_and_row(ctx, case, kernel):
    """impc_batch_update_bounds reports where l > u, as impc_batch_set_values does."""
    f = Feed(ctx, case["pat"], 4, False, kernel)
    try:
        f.set_values(*base(case))
        if kernel == impc.KERNEL_STRUCTURED:
            f.b.set_persistent(True)
        f.solve()
        with pytest.raises(impc.ImpcError) as e:
            f.update_bounds(crossed(case), case["v"]["u"])
        assert e.value.code == DATA_VALIDATION_ERROR
        assert "lower bound greater than upper bound (QP 2, row 5)" in str(e.value)
    finally:
        f.close()
