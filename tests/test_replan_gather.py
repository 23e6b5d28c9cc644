"""Each replan's per-instance records (impc_replan_record, include/impc_replan.h): the layout, the
host restatement impc.distributed.pack_replan_records, the device pack (impc_replan_pack_device,
k_pack_records) against it byte for byte, the in-place RCCL all-gather (impc_replan_gather) on a
world of one, and the device replan on a split of the instances against the whole batch.

The GPU tests use the scenario of tests/test_replan_branches.py (I = 24, K = 3, N = 20, one replan
from set_state(prev, first): all three branches), without an issue cut-off and without a solver
time limit, so nothing depends on the clock."""
import ctypes as C
import os
import struct
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

import impc
from impc import distributed as D
from impc.replan import (FANOUT, SINGLE_CURRENT, SINGLE_FIRST, DeviceReplan, ReplanRecord, record_dtype,
                         solve_traj_ok)

INVALID_ARGUMENT = 101
OFFSETS = dict(rank=0, inst=4, branch=8, valid=9, first_time=10, has_plan=11, best_cand=12, num_obs=16, ob_idx=20,
               status=24, iter=28, obj=32, score=40, pri_res=48, dua_res=56)
HEADER = "<iibbbbiiiiidddd"  # the header's fields in offset order (no padding: 64 bytes)


# ------------------------------------------------------------------------------------- layout
def test_record_layout():
    assert C.sizeof(ReplanRecord) == 64 == struct.calcsize(HEADER)
    for f, off in OFFSETS.items():
        assert getattr(ReplanRecord, f).offset == off, f
    for P in (0, 1, 20):
        dt = record_dtype(P)
        assert dt.itemsize == 64 + 64 * P
        for f, off in OFFSETS.items():
            assert dt.fields[f][1] == off, (P, f)
        assert dt.fields["plan_states"][1] == 64 and dt["plan_states"].shape == (P, 8)
        assert dt["plan_states"].base == np.float64
    assert [dt[f] for f in ("rank", "branch", "obj")] == [np.int32, np.int8, np.float64]


# ------------------------------------------------------------------------------- known answer
def _info(rows):
    a = np.zeros(len(rows), impc.INFO_DTYPE)
    for j, (it, st, obj, pri, dua) in enumerate(rows):
        a[j]["iter"], a[j]["status_val"], a[j]["obj_val"], a[j]["pri_res"], a[j]["dua_res"] = it, st, obj, pri, dua
        a[j]["rho_updates"], a[j]["rho_estimate"] = 7, 0.25  # not part of a record
    return a


def test_pack_known_answer():
    """Four hand-written instances -- a fan-out with a selection, a fan-out without one, a first
    plan, a current-obstacle solve with a failed status -- read back with struct at the stated
    offsets, zero padding rows included."""
    N, P, n = 4, 3, 13 * 4 - 5
    plan_x = np.arange(4 * n, dtype=np.float64).reshape(4, n) + 0.5
    va = dict(branch=np.array([FANOUT, FANOUT, SINGLE_FIRST, SINGLE_CURRENT], np.int8),
              valid=np.array([1, 0, 1, 0], np.int8), first_time=np.array([0, 0, 0, 0], np.int8),
              prev_count=np.array([N, N, N, N], np.int32), best_cand=np.array([2, -1, -1, -1], np.int32),
              num_obs=np.array([2, 1, 0, 3], np.int32), ob_idx=np.array([1, 0, -1, -1], np.int32),
              # instance 0: candidate 2 sits in slot 4 (a two-intent candidate): shape 2 + 1, row 5
              cand_slot=np.array([[0, 1, 4, 2, 3, 5], [0, 1, 2, 3, 4, 5], [-1] * 6, [-1] * 6], np.int32),
              slot_row=np.array([[0, 1, 2, 3, 5, 6], [0, 1, 2, 3, 0, 1], [1, -1, -1, -1, -1, -1],
                                 [2, -1, -1, -1, -1, -1]], np.int32),
              shape=np.array([2, 1, 0, 3], np.int32), plan_x=plan_x)
    infos = {0: _info([(1, 1, 1.0, 0.1, 0.2), (25, 1, -3.5, 1e-4, 2e-4)]),
             3: _info([(0, 0, 0, 0, 0)] * 2 + [(4000, -3, float("inf"), 0.75, 1.5)] + [(0, 0, 0, 0, 0)] * 2 +
                      [(50, 2, 12.25, 3e-3, 4e-3)])}
    weighted = np.full((4, 6), np.nan)
    weighted[0, 2] = 2.625
    rec = D.pack_replan_records(5, 100, P, 6, va, infos, weighted)
    assert rec.dtype == record_dtype(P) and rec.shape == (6,)
    raw = rec.tobytes()
    size = 64 + 64 * P
    assert len(raw) == 6 * size
    want = [(5, 100, FANOUT, 1, 0, 1, 2, 2, 1, 2, 50, 12.25, 2.625, 3e-3, 4e-3),
            (5, 101, FANOUT, 0, 0, 1, -1, 1, 0, 0, 0, 0.0, 0.0, 0.0, 0.0),
            (5, 102, SINGLE_FIRST, 1, 0, 1, -1, 0, -1, 1, 25, -3.5, 0.0, 1e-4, 2e-4),
            (5, 103, SINGLE_CURRENT, 0, 0, 1, -1, 3, -1, -3, 4000, float("inf"), 0.0, 0.75, 1.5)]
    for i, w in enumerate(want):
        assert struct.unpack_from(HEADER, raw, i * size) == w, i
        for f, off in OFFSETS.items():  # each field alone at its stated offset
            code = "<i" if f in ("rank", "inst", "best_cand", "num_obs", "ob_idx", "status", "iter") else \
                "<b" if f in ("branch", "valid", "first_time", "has_plan") else "<d"
            assert struct.unpack_from(code, raw, i * size + off)[0] == w[list(OFFSETS).index(f)], (i, f)
        assert struct.unpack_from(f"<{8 * P}d", raw, i * size + 64) == tuple(plan_x[i, : 8 * P]), i
    assert raw[4 * size:] == bytes(2 * size)  # the padding rows
    # plan_states [I][N][8] instead of plan_x; P = 0: headers only
    va2 = dict(va, plan_states=plan_x[:, : 8 * N].reshape(4, N, 8))
    del va2["plan_x"]
    assert D.pack_replan_records(5, 100, P, 6, va2, infos, weighted).tobytes() == raw
    r0 = D.pack_replan_records(5, 100, 0, 4, va, infos, weighted)
    assert r0.tobytes() == b"".join(raw[i * size: i * size + 64] for i in range(4))
    with pytest.raises(ValueError):
        D.pack_replan_records(5, 100, P, 3, va, infos, weighted)
    with pytest.raises(ValueError):
        D.pack_replan_records(5, 2 ** 31 - 3, P, 6, va, infos, weighted)


# ------------------------------------------------------------------------------ two gloo ranks
WORLD, SPLIT = 2, (0, 2, 6)  # an uneven split: 2 and 4 of 6 instances


def _ref_replan(idx):
    """One makePlanWithPred of the instances `idx` of a fixed 6-instance mixed-branch scenario on
    the restatement (oracle/replan_ref.py), as the host arrays of pack_replan_records: view_arrays,
    shape_infos (each shape's rows in the order the instances produce them) and weighted."""
    from impc import scenarios
    from oracle import replan_ref as ref
    from oracle import select_ref
    Iall, K, N = 6, 3, 20
    inst = next(iter(scenarios.intent_config(N=N, K=K, instances=Iall, hyps=6, seed=6060).values()))["instances"]
    _, pd = impc.mpc_params(horizon=N)
    s = impc.default_settings(verbose=0)
    pred_size = np.broadcast_to(inst["size"], inst["pred"].shape).copy()
    cur_size = np.broadcast_to(inst["size"], (Iall, K, 3)).copy()
    ar = np.arange(Iall)
    first, has_pred, cur_count = ar % 3 == 0, ar % 4 != 0, np.where(ar % 2 == 0, K, 0)
    n, I = 13 * N - 5, len(idx)
    va = dict(branch=np.zeros(I, np.int8), valid=np.zeros(I, np.int8), first_time=np.zeros(I, np.int8),
              prev_count=np.zeros(I, np.int32), best_cand=np.full(I, -1, np.int32), num_obs=np.zeros(I, np.int32),
              ob_idx=np.full(I, -1, np.int32), cand_slot=np.full((I, 6), -1, np.int32),
              slot_row=np.full((I, 6), -1, np.int32), shape=np.zeros(I, np.int32), plan_x=np.zeros((I, n)))
    weighted = np.full((I, 6), np.nan)
    infos = {}

    def add(k, info):
        infos.setdefault(k, []).append(info)
        return len(infos[k]) - 1

    for j, i in enumerate(idx):
        ft = int(first[i])
        px = np.concatenate([inst["prev"][i].reshape(-1), np.zeros(n - 8 * N)])
        pos, vel, xref, pred = inst["pos"][i], inst["vel"][i], inst["xref"][i], inst["pred"][i]
        dyn_cur = pred[:, 0, 0, :]
        br = ref.branch(ft, bool(has_pred[i]), int(cur_count[i]))
        plan = None
        if br == ref.FANOUT:
            fo, qps = ref.fanout_qps(pd, ft, px, pos, vel, xref, dyn_cur, pred, pred_size[i], inst["prob_all"][i])
            sols = [ref.solve(p, v, w, s) for p, v, w in qps]
            ns = npair = 0
            for c, t in enumerate(fo["types"]):  # single-intent candidates fill slots 0..3, two-intent 4..5
                if t < 4:
                    slot, ns = ns, ns + 1
                else:
                    slot, npair = 4 + npair, npair + 1
                va["cand_slot"][j, c] = slot
                va["slot_row"][j, slot] = add(K + (1 if slot >= 4 else 0), sols[c][2])
            states = [[list(x[8 * k: 8 * k + 8]) for k in range(N)] for x, _, _ in sols]
            best, bpos, _, w = select_ref.select_instance(
                states, [ref.solve_traj_ok(sol[2]) for sol in sols], ref._states(px, N), ft, [list(r) for r in xref],
                [], [c[0] for c in fo["cands"]], [c[1] for c in fo["cands"]], inst["prob_all"][i][fo["ob_idx"]],
                pd["dynamic_safety_dist"], pd["static_safety_dist"])
            va["best_cand"][j], va["num_obs"][j], va["ob_idx"][j], va["shape"][j] = best, K, fo["ob_idx"], K
            if best >= 0:
                weighted[j, best] = w[bpos]
                plan = sols[best][0]
        else:
            cur = br == ref.SINGLE_CURRENT
            ci = int(cur_count[i]) if cur else 0
            p, v, w = ref.single_qp(pd, ft, px, pos, vel, xref, dyn_cur[:ci] if cur else None,
                                    cur_size[i][:ci] if cur else None)
            x, _, info = ref.solve(p, v, w, s)
            va["num_obs"][j] = va["shape"][j] = ci
            va["slot_row"][j, 0] = add(ci, info)
            if ref.solve_traj_ok(info):
                plan = x
        va["branch"][j], va["valid"][j] = br, plan is not None
        va["first_time"][j] = 0 if plan is not None else ft
        va["prev_count"][j] = N if (plan is not None or not ft) else 0
        va["plan_x"][j] = plan if plan is not None else px
    return va, {k: np.array(v) for k, v in infos.items()}, weighted


def _gloo_worker(rank, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(WORLD))
    try:
        import sys
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path[:0] = [here, os.path.dirname(here)]
        r, lr, w = D.env()
        dist = D.init("gloo", lr)
        counts = [SPLIT[k + 1] - SPLIT[k] for k in range(w)]
        lo, hi = SPLIT[r], SPLIT[r + 1]
        P = 20
        rec = D.pack_replan_records(r, lo, P, hi - lo, *_ref_replan(range(lo, hi)))
        # the exchange moves bytes: records as uint8 rows, viewed as the dtype again after unpad
        rows = np.frombuffer(rec.tobytes(), np.uint8).reshape(hi - lo, rec.dtype.itemsize)
        allrows = D.gather_costs(dist, rows, counts)
        dist.barrier()
        dist.destroy_process_group()
        q.put((r, allrows, counts))
    except Exception:  # surface the failure in the parent
        import traceback
        q.put((rank, traceback.format_exc(), None))


def test_two_rank_gloo_records_match_whole_batch():
    """The restatement's records over two gloo ranks holding 2 and 4 of 6 instances: both ranks end
    with identical bytes, equal to the whole batch packed in one process in every field but rank."""
    from test_distributed import _free_port
    mctx = mp.get_context("spawn")
    q = mctx.Queue()
    port = _free_port()
    procs = [mctx.Process(target=_gloo_worker, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    whole = D.pack_replan_records(0, 0, 20, 6, *_ref_replan(range(6)))
    out = {}
    for _ in range(WORLD):
        r, rows, counts = q.get(timeout=600)
        assert counts is not None, rows
        out[r] = rows
        assert counts == [2, 4]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert out[0].tobytes() == out[1].tobytes()
    got = np.frombuffer(out[0].tobytes(), record_dtype(20))
    assert got.shape == (6,)
    np.testing.assert_array_equal(got["rank"], [0, 0, 1, 1, 1, 1])
    np.testing.assert_array_equal(got["inst"], np.arange(6))
    same = got.copy()
    same["rank"] = 0
    assert same.tobytes() == whole.tobytes()
    assert set(got["branch"]) == {FANOUT, SINGLE_FIRST, SINGLE_CURRENT}
    assert (got["best_cand"][got["branch"] == FANOUT] >= 0).any() and (got["score"] != 0).any()


# ------------------------------------------------------------------------------------------ GPU
I, K, N = 24, 3, 20


def _inputs(lo=0, hi=I):
    """The scenario of test_replan_branches.test_mixed_branches_three_chained_replans, instances
    [lo, hi): everything run() takes, and prev / first for set_state."""
    from test_replan_branches import _scenario
    p, pd, inst, pred_size = _scenario()
    idx = np.arange(I)
    full = dict(pos=inst["pos"], vel=inst["vel"], xref=inst["xref"], pred=inst["pred"], pred_size=pred_size,
                prob=inst["prob_all"], prev=inst["prev"], first=(idx % 4 == 0).astype(np.int8),
                has_pred=[idx % 3 != 1, idx % 5 != 2], cur_count=np.where(idx % 2 == 0, K, 0),
                cur_size=np.broadcast_to(inst["size"], (I, K, 3)).copy())
    d = {k: (v[lo:hi].copy() if not isinstance(v, list) else [h[lo:hi] for h in v]) for k, v in full.items()}
    return p, pd, d


def _run(rp, d, step, pos, vel, pred, **kw):
    return rp.run(pos, vel, d["xref"], dyn_cur=pred[:, :, 0, 0, :], pred_pos=pred, pred_size=d["pred_size"],
                  prob=d["prob"], has_pred=d["has_pred"][step], cur_size=d["cur_size"], cur_count=d["cur_count"], **kw)


def _pack(ctx, rp, rank, inst_base, P, max_inst):
    """pack_device into a fresh buffer prefilled with ones (so that unwritten bytes show); the
    records on the host"""
    dt = record_dtype(P)
    buf = impc.DeviceArray(ctx, np.full(max_inst * dt.itemsize, 0xFF, np.uint8))
    try:
        rp.pack_device(rank, inst_base, P, max_inst, buf.ptr)
        return np.frombuffer(buf.get().tobytes(), dt)
    finally:
        buf.free()


@pytest.fixture(scope="module")
def replanned(ctx):
    """One replan of the 24 instances (no cut-off, no time limit) and its host arrays."""
    p, pd, d = _inputs()
    s = impc.default_settings(verbose=0)
    rp = DeviceReplan(ctx, p, pd, I, K, d["pred"].shape[3], s, issue_cutoff_s=0.0)
    rp.set_state(d["prev"], d["first"])
    out = _run(rp, d, 0, d["pos"], d["vel"], d["pred"])
    yield rp, rp.record_arrays(out), d
    rp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [0, 1, 7, 20])
def test_pack_device_matches_restatement(ctx, replanned, P):
    """8 P = 0, 8, 56, 160 words of plan per record: below, around and not a multiple of the 64
    lanes that copy them.  Byte for byte; rows 24..28 zero."""
    rp, arrays, _ = replanned
    got = _pack(ctx, rp, 3, 1000, P, 29)
    want = D.pack_replan_records(3, 1000, P, 29, *arrays)
    assert got.tobytes() == want.tobytes()
    assert got[24:].tobytes() == bytes(5 * (64 + 64 * P))
    assert set(got["branch"][:24]) == {FANOUT, SINGLE_FIRST, SINGLE_CURRENT}
    assert (got["rank"][:24] == 3).all() and (got["inst"][:24] == 1000 + np.arange(24)).all()
    fan = got["branch"][:24] == FANOUT
    assert (got["best_cand"][:24][fan] >= 0).any() and (got["score"][:24][fan] != 0).any()
    assert (got["iter"][:24][~fan] > 0).all() and (got["status"][:24][~fan] != 0).all()


@pytest.mark.gpu
def test_pack_device_single_instance(ctx):
    p, pd, d = _inputs(0, 1)
    rp = DeviceReplan(ctx, p, pd, 1, K, d["pred"].shape[3], impc.default_settings(verbose=0), issue_cutoff_s=0.0)
    try:
        rp.set_state(d["prev"], d["first"])
        out = _run(rp, d, 0, d["pos"], d["vel"], d["pred"])
        got = _pack(ctx, rp, 0, 0, 20, 1)
        assert got.tobytes() == D.pack_replan_records(0, 0, 20, 1, *rp.record_arrays(out)).tobytes()
        assert got["branch"][0] == SINGLE_FIRST and got["valid"][0] == 1 and got["has_plan"][0] == 1
    finally:
        rp.close()


@pytest.mark.gpu
def test_no_selection_keeps_previous_plan(ctx):
    """Past the issue cut-off (0.15 s; the replan starts 1 s late) no candidate is issued: every
    fan-out record has no selection, zero QP fields and the previous plan's states."""
    p, pd, d = _inputs()
    rp = DeviceReplan(ctx, p, pd, I, K, d["pred"].shape[3], impc.default_settings(verbose=0))
    try:
        rp.set_state(d["prev"], d["first"])
        out = _run(rp, d, 0, d["pos"], d["vel"], d["pred"], t_start=time.perf_counter() - 1.0)
        assert not out["issued"]
        got = _pack(ctx, rp, 0, 0, N, I)
        assert got.tobytes() == D.pack_replan_records(0, 0, N, I, *rp.record_arrays(out)).tobytes()
        fan = got["branch"] == FANOUT
        assert fan.sum() >= 8
        f = got[fan]
        assert (f["valid"] == 0).all() and (f["best_cand"] == -1).all() and (f["has_plan"] == 1).all()
        for k in ("status", "iter", "obj", "score", "pri_res", "dua_res"):
            assert f[k].tobytes() == bytes(f[k].nbytes), k
        assert f["plan_states"].tobytes() == np.ascontiguousarray(d["prev"][fan], np.float64).tobytes()
        assert (got["iter"][~fan] > 0).all()  # the single solves have no cut-off
    finally:
        rp.close()


@pytest.mark.gpu
def test_world_one_rccl_gather(ctx, replanned):
    """impc_replan_gather on a communicator of one rank: the in-place all-gather leaves exactly
    pack_device's bytes for rank 0."""
    rp, _, _ = replanned
    P, mx = 20, I + 5
    dt = record_dtype(P)
    comm = D.make_comm(None, ctx)
    recv = impc.DeviceArray(ctx, np.full(mx * dt.itemsize, 0xFF, np.uint8))
    try:
        rp.gather_records(comm, 1000, P, mx, recv.ptr)
        ctx.synchronize()
        got = recv.get().tobytes()
        assert got == _pack(ctx, rp, 0, 1000, P, mx).tobytes()
        recv.set(np.full(mx * dt.itemsize, 0xFF, np.uint8))
        comm.gather_replan_records(rp, 1000, P, mx, recv.ptr)  # the communicator's pass-through
        assert recv.get().tobytes() == got
    finally:
        recv.free()
        comm.close()


@pytest.mark.gpu
def test_split_replan_equals_whole_batch(ctx):
    """impc_replan_run on the instance ranges [0, 9) and [9, 24) against the whole batch over two
    chained replans: the halves pack into one buffer where an all-gather would place their blocks,
    and unpad gives the whole object's records in every field but rank, bit for bit (a QP's
    arithmetic depends neither on its row nor on its batch's size).  The whole object is checked
    against oracle/replan_ref.py by test_replan_branches._check_replan."""
    from test_replan_branches import _check_replan
    bounds, mx, P = (0, 9, 24), 15, N
    s = impc.default_settings(verbose=0)
    dt = record_dtype(P)
    p, pd, dw = _inputs()
    parts = [_inputs(bounds[r], bounds[r + 1])[2] for r in range(2)]
    L = dw["pred"].shape[3]
    objs = [DeviceReplan(ctx, p, pd, hi - lo, K, L, s, issue_cutoff_s=0.0) for lo, hi in ((0, I), (0, 9), (9, 24))]
    recv = impc.DeviceArray(ctx, (2 * mx * dt.itemsize,), np.uint8)
    try:
        data = [dw] + parts
        state = []
        for rp, d in zip(objs, data):
            rp.set_state(d["prev"], d["first"])
            state.append([d["pos"].copy(), d["vel"].copy(), d["pred"].copy()])
        seen = set()
        for step in range(2):
            before = objs[0].plans()
            outs = [_run(rp, d, step, *st) for rp, d, st in zip(objs, data, state)]
            pos, vel, pred = state[0]
            expect, expect_first = _check_replan(outs[0], before, pos, vel, dw["xref"], pred[:, :, 0, 0, :], pred,
                                                 dw["pred_size"], dw["prob"], dw["has_pred"][step], dw["cur_size"],
                                                 dw["cur_count"], pd, s)
            plan_x, ft, _, valid = objs[0].plans()
            np.testing.assert_array_equal(plan_x, expect)
            np.testing.assert_array_equal(ft, expect_first)
            whole = _pack(ctx, objs[0], 0, 0, P, I)
            np.testing.assert_array_equal(whole["branch"], outs[0]["branch"])
            np.testing.assert_array_equal(whole["best_cand"], outs[0]["best_cand"])
            np.testing.assert_array_equal(whole["valid"], valid)
            ok = [outs[0]["best_cand"][i] >= 0 if outs[0]["branch"][i] == FANOUT else
                  bool(solve_traj_ok(outs[0]["shapes"][outs[0]["single_rows"][i][0]]["info"][outs[0]["single_rows"][i][1]]))
                  for i in range(I)]
            np.testing.assert_array_equal(valid == 1, ok)  # validTraj as the restatement decides it
            recv.set(np.full(2 * mx * dt.itemsize, 0xFF, np.uint8))
            for r in range(2):
                objs[1 + r].pack_device(r, bounds[r], P, mx, recv.ptr + r * mx * dt.itemsize)
            got = D.unpad(np.frombuffer(recv.get().tobytes(), dt), [9, 15])
            np.testing.assert_array_equal(got["rank"], [0] * 9 + [1] * 15)
            for f in dt.names:
                if f != "rank":  # integers equal, doubles bit-equal
                    assert got[f].tobytes() == whole[f].tobytes(), (step, f)
            seen.update(int(b) for b in whole["branch"])
            for rp, st in zip(objs, state):  # next replan: x0 = the plan's next state, predictions one step on
                px, _, _, v = rp.plans()
                st[0] = np.where(v[:, None] == 1, px[:, 8:11], st[0])
                st[1] = np.where(v[:, None] == 1, px[:, 11:14], st[1])
                st[2] = np.concatenate([st[2][:, :, :, 1:], st[2][:, :, :, -1:]], axis=3)
        assert seen == {FANOUT, SINGLE_FIRST, SINGLE_CURRENT}
    finally:
        recv.free()
        for rp in objs:
            rp.close()


@pytest.mark.gpu
def test_argument_errors_leave_the_object_usable(ctx, replanned):
    rp, arrays, d = replanned
    P, dt = 5, record_dtype(5)
    lib, _P = impc.lib, C.c_void_p
    buf = impc.DeviceArray(ctx, ((I + 1) * dt.itemsize,), np.uint8)
    fresh = DeviceReplan(ctx, *_inputs()[:2], I, K, d["pred"].shape[3], impc.default_settings(verbose=0))
    other = impc.Context(0)
    comm, foreign = D.make_comm(None, ctx), D.make_comm(None, other)
    try:
        def pack(h, rank, base, steps, mx, out):
            return lib.impc_replan_pack_device(h, rank, base, steps, mx, _P(out))

        def gather(h, c, base, steps, mx, out):
            return lib.impc_replan_gather(h, c, base, steps, mx, _P(out))

        bad = [pack(None, 0, 0, P, I, buf.ptr), pack(rp.h, 0, 0, P, I, None), pack(rp.h, 0, 0, -1, I, buf.ptr),
               pack(rp.h, 0, 0, N + 1, I, buf.ptr), pack(rp.h, 0, 0, P, I - 1, buf.ptr),
               pack(rp.h, 0, -1, P, I, buf.ptr), pack(rp.h, 0, 2 ** 31 - I + 1, P, I, buf.ptr),
               pack(fresh.h, 0, 0, P, I, buf.ptr),
               gather(None, comm.h, 0, P, I, buf.ptr), gather(rp.h, None, 0, P, I, buf.ptr),
               gather(rp.h, comm.h, 0, P, I, None), gather(rp.h, comm.h, 0, N + 1, I, buf.ptr),
               gather(rp.h, comm.h, 0, P, I - 1, buf.ptr), gather(rp.h, comm.h, -1, P, I, buf.ptr),
               gather(fresh.h, comm.h, 0, P, I, buf.ptr), gather(rp.h, foreign.h, 0, P, I, buf.ptr)]
        assert bad == [INVALID_ARGUMENT] * len(bad)
        assert impc.lib.impc_last_error().decode()
        with pytest.raises(impc.ImpcError) as e:
            rp.pack_device(0, 0, N + 1, I, buf.ptr)
        assert e.value.code == INVALID_ARGUMENT and "plan_steps" in str(e.value)
        # the largest instance ids still pack; the object is as usable as before
        base = 2 ** 31 - I
        rp.pack_device(1, base, P, I + 1, buf.ptr)
        got = np.frombuffer(buf.get().tobytes(), dt)
        assert got.tobytes() == D.pack_replan_records(1, base, P, I + 1, *arrays).tobytes()
        assert got["inst"][I - 1] == 2 ** 31 - 1
        rp.gather_records(comm, 0, P, I + 1, buf.ptr)
        assert buf.get().tobytes() == D.pack_replan_records(0, 0, P, I + 1, *arrays).tobytes()
    finally:
        comm.close()
        foreign.close()
        other.close()
        fresh.close()
        buf.free()
