// replan_run.hip -- the whole batched makePlanWithPred behind one C-ABI call (include/impc_replan.h,
// impc_replan_*), part of libimpc_qp.so.
//
// Reference: trajectory_planner/include/trajectory_planner/mpcPlanner.cpp:571-661 (makePlanWithPred),
// called per planning instance by mpcNavigation.cpp:316-322.  Per instance it takes one of three
// branches (:593-606) -- the intent fan-out with six candidate solves and a selection, or ONE
// solveTraj (first plan, or no predictions) -- and commits the plan it gets into the planner state.
// Every instance may track a different number of obstacles (predPos.size(), :343-373).  Here every
// instance of a batch goes through one call, and the call never waits for the device:
//
//   k_plan_rows   the branch of every instance and the rows of every QP shape (shape k = the QPs
//                 with k dynamic-obstacle rows per stage; with per-instance static counts bound,
//                 the pair (k, s_i)), by a scan over the instances, one workgroup per tile of
//                 shapes; the device clock at the start of the replan
//   k_pick        one thread per instance: findClosestObstacle + getIntentComb's candidate order
//   k_prep        one wavefront per row: the warm start, the time limit and the obstacle sources
//                 (which prediction / current obstacle each obstacle row linearises)
//   build         impc_lib::build_rows per shape: the device builder straight from the per-instance
//                 inputs, written in place into the shape's solver batch
//   k_issue       the issue cut-off (:613) on the device clock; each shape's solve count
//   solve         ONE impc_batch_solve_group over every shape, each batch's QP count read from
//                 device memory by the solver itself
//   k_cand        the candidates' validity (solveProblem NoError), solution pointers, obstacle sets
//   selection     impc_select_best_device over every instance (non-fan-out instances: no candidate)
//   k_commit      every plan into the planner state
//   k_commit_ref   the reference of every committed plan (ref_, plan_exec.hpp)
//
// No x, y, QP value or count leaves the device, and nothing on the host waits for it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/impc_exec.h"
#include "../../include/impc_fanout.h"
#include "../../include/impc_mpc.h"
#include "../../include/impc_qp.h"
#include "../../include/impc_replan.h"
#include "../../include/impc_select.h"
#include "lib_internal.hpp"
#include "plan_exec.hpp"

namespace impc_rp {

constexpr int kPlanLanes = 512;
constexpr int kPlanTile = 14;  // shapes per workgroup of the row scan: (2 * 14 + 3) * 520 int32 = 63 KB of LDS
constexpr int kMaxObstacles = 30;
constexpr int FORWARD = 0, LEFT = 1, RIGHT = 2, STOP = 3;  // dynamicPredictor's intent enum

// Shape k's rows in the flat row arrays: shape 0 holds the single solves without dynamic
// obstacles (<= I rows); shapes 1..K at most four rows per instance (the four single-intent
// candidates of an instance with K_i = k, or the two two-intent candidates of one with K_i + 1 =
// k, or one current-obstacle single solve with c_i = k); shape K + 1 the two-intent candidates of
// the instances with K_i = K (<= 2 I rows); shape K + 2, present with static obstacles only, the
// first plans (<= I rows; without static obstacles they are shape 0's).
__host__ __device__ inline int64_t shape_base(int64_t I, int K, int k) {
    return k == 0 ? 0 : k <= K + 1 ? I + 4 * I * (int64_t)(k - 1) : I * (4 * (int64_t)K + 3);
}
__host__ __device__ inline int64_t shape_cap(int64_t I, int K, int k) {
    return k == 0 ? I : k <= K ? 4 * I : k == K + 1 ? 2 * I : I;
}
__host__ __device__ inline int shape_of(int64_t I, int K, int64_t f) {
    if (f < I) return 0;
    if (f >= I * (4 * (int64_t)K + 3)) return K + 2;
    const int64_t k = 1 + (f - I) / (4 * I);
    return (int)(k < K + 1 ? k : K + 1);
}
// the dynamic-obstacle rows per stage of shape k's QPs
__host__ __device__ inline int shape_dyn(int K, int k) { return k <= K + 1 ? k : 0; }

// With per-instance static counts bound (impc_replan_bind_static_count) a shape is the pair (k
// dynamic rows, s static rows).  Ids 0 .. K + 2 are the shapes above (s = S_st; K + 2: none); the
// pair (k, s < S_st), k in 0 .. K + 1, has id K + 3 + s (K + 2) + k and shape k's capacity, its rows
// after the I (4 K + 4) rows of ids 0 .. K + 2: block s of I (4 K + 3) rows laid out as ids 0 .. K + 1.
__host__ __device__ inline int shape_id(int K, int nst, int k, int s) {
    return s >= nst ? k : K + 3 + s * (K + 2) + k;
}
__host__ __device__ inline int64_t xshape_base(int64_t I, int K, int id) {
    if (id <= K + 2) return shape_base(I, K, id);
    const int e = id - (K + 3);
    return I * (4 * (int64_t)K + 4) + (int64_t)(e / (K + 2)) * I * (4 * (int64_t)K + 3) + shape_base(I, K, e % (K + 2));
}
__host__ __device__ inline int64_t xshape_cap(int64_t I, int K, int id) {
    return shape_cap(I, K, id <= K + 2 ? id : (id - (K + 3)) % (K + 2));
}
__host__ __device__ inline int xshape_of(int64_t I, int K, int64_t f) {
    const int64_t r0 = I * (4 * (int64_t)K + 4), blk = I * (4 * (int64_t)K + 3);
    if (f < r0) return shape_of(I, K, f);
    const int64_t g = f - r0;
    return K + 3 + (int)(g / blk) * (K + 2) + shape_of(I, K, g % blk);
}
__host__ __device__ inline int xshape_dyn(int K, int id) {
    return id <= K + 2 ? shape_dyn(K, id) : (id - (K + 3)) % (K + 2);
}
// the static-obstacle rows per stage of shape id's QPs
__host__ __device__ inline int xshape_stat(int K, int nst, int id) {
    return id <= K + 1 ? nst : id == K + 2 ? 0 : (id - (K + 3)) / (K + 2);
}

// per-shape device pointers, fixed when the replan object is created
struct ShapeDev {
    double *xws, *tlim;       // the batch's warm-start input [cap][n] and time limits [cap]
    const double *x;          // the batch's primal solutions [cap][n]
    const impc_info *info;    // [cap]
    int64_t *osrc;            // obstacle sources [cap][k] (build_rows)
};

// The branch of one instance (:593-606), its predicted-obstacle count K_i and current count c_i.
struct Decide {
    const int8_t *first_time, *has_pred;
    const int32_t *num_pred, *cur_count;
    int32_t K, cur_all;
    __device__ void operator()(int64_t i, int &br, int &ki, int &ci) const {
        const bool ft = first_time[i] != 0;
        ki = num_pred ? min(max(num_pred[i], 0), K) : K;
        const bool hp = (has_pred ? has_pred[i] != 0 : true) && ki > 0;  // obPredPos_.size() != 0
        ci = cur_count ? min(max(cur_count[i], 0), K) : (cur_all ? K : 0);
        br = (!ft && hp) ? IMPC_REPLAN_FANOUT : (!ft && ci > 0) ? IMPC_REPLAN_SINGLE_CURRENT : IMPC_REPLAN_SINGLE_FIRST;
    }
};

struct PlanArgs {
    int64_t I;
    int32_t K, T, tile, nst, first_shape;  // T shapes in tiles of `tile`; first_shape: the first plans'
                                           // shape (K + 2 with static obstacles, else 0)
    Decide decide;
    const int32_t *scount;      // [I] bound static counts, or null: nst for every instance
    int8_t *branch;
    int32_t *num_obs, *shp, *slot_row, *best, *scnt;
    int32_t *row_inst;
    int8_t *row_code;
    int64_t *cnt;               // [T] single solves per shape, [T .. 2T) rows per shape, [2T .. 2T+3) branches
    unsigned long long *clk;    // [0] the device clock at the start of the replan
};

// The shapes of one instance: its single solve's (a first plan's QP has no obstacle rows -- static
// and dynamic obstacles cleared, :593-602 --, any other has the current obstacles' c_i (0 with
// SINGLE_FIRST) and the instance's s_i statics), or its candidates' two (K_i and K_i + 1 dynamic rows).
struct InstShapes {
    int br, ki, ci, si, id0, id1;  // id0: the single solve's / the single-intent candidates' shape
    bool first;
};
__device__ inline InstShapes inst_shapes(const PlanArgs &a, int64_t i) {
    InstShapes r;
    a.decide(i, r.br, r.ki, r.ci);
    r.si = a.scount ? min(max(a.scount[i], 0), a.nst) : a.nst;
    r.first = a.decide.first_time[i] != 0;
    if (r.br == IMPC_REPLAN_FANOUT) {
        r.id0 = shape_id(a.K, a.nst, r.ki, r.si);
        r.id1 = shape_id(a.K, a.nst, r.ki + 1, r.si);
    } else {
        r.id0 = r.br == IMPC_REPLAN_SINGLE_CURRENT ? shape_id(a.K, a.nst, r.ci, r.si)
                : r.first                          ? a.first_shape
                                                   : shape_id(a.K, a.nst, 0, r.si);
        r.id1 = -1;
    }
    return r;
}

// One workgroup of kPlanLanes lanes per tile of `tile` consecutive shape ids (one tile holds every
// shape of an object without bound static counts up to K = 11, so the LDS is bounded whatever the
// shape count: with counts bound the (K + 2)(S_st + 1) + 1 shapes spread over more workgroups, each
// deciding every instance again and keeping only its own shapes' rows).  Lane t owns a contiguous
// range of instances.  Counters [R = 2 tile + 3][kPlanLanes] in LDS (rows 0..tile-1: single solves
// of the tile's shapes, tile..2 tile-1: their candidate rows, the last three: instances per branch),
// an exclusive scan over the lanes (a wavefront scan of 64 lanes, then the wavefront totals), and a
// second pass that writes each instance's rows in ascending order: every shape holds its single
// solves first, then its candidates.  An instance's per-instance outputs are written by the
// workgroup of its shape id0, slots 4 and 5 of a fan-out instance by that of id1.
__global__ __launch_bounds__(kPlanLanes) void k_plan_rows(PlanArgs a) {
    extern __shared__ int32_t cl[];  // [R][kPlanLanes], then wave totals [R][kPlanLanes / 64]
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, NW = kPlanLanes / 64;
    const int S = a.tile, R = 2 * S + 3, T = a.T;
    const int s0 = (int)blockIdx.x * S, s1 = min(T, s0 + S);  // this workgroup's shape ids
    int32_t *wt = cl + R * kPlanLanes;
    if (t == 0 && blockIdx.x == 0) a.clk[0] = wall_clock64();
    const int64_t per = (a.I + kPlanLanes - 1) / kPlanLanes;
    const int64_t i0 = min(a.I, (int64_t)t * per), i1 = min(a.I, i0 + per);
    const auto mine = [&](int id) { return id >= s0 && id < s1; };
    for (int r = 0; r < R; r++) cl[r * kPlanLanes + t] = 0;
    for (int64_t i = i0; i < i1; i++) {
        const InstShapes d = inst_shapes(a, i);
        cl[(2 * S + d.br) * kPlanLanes + t]++;
        if (d.br == IMPC_REPLAN_FANOUT) {
            if (mine(d.id0)) cl[(S + d.id0 - s0) * kPlanLanes + t] += 4;
            if (mine(d.id1)) cl[(S + d.id1 - s0) * kPlanLanes + t] += 2;
        } else if (mine(d.id0)) {
            cl[(d.id0 - s0) * kPlanLanes + t]++;
        }
    }
    for (int r = 0; r < R; r++) {  // exclusive scan inside each wavefront
        const int v = cl[r * kPlanLanes + t];
        int x = v;
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        cl[r * kPlanLanes + t] = x - v;
        if (lane == 63) wt[r * NW + w] = x;
    }
    __syncthreads();
    for (int r = 0; r < R; r++) {
        int add = 0;
        for (int ww = 0; ww < w; ww++) add += wt[r * NW + ww];
        cl[r * kPlanLanes + t] += add;
    }
    auto total = [&](int r) {
        int64_t s = 0;
        for (int ww = 0; ww < NW; ww++) s += wt[r * NW + ww];
        return s;
    };
    for (int64_t i = i0; i < i1; i++) {
        const InstShapes d = inst_shapes(a, i);
        int32_t *sr = a.slot_row + 6 * i;
        if (mine(d.id0)) {
            a.branch[i] = (int8_t)d.br;
            a.best[i] = -1;
            a.shp[i] = d.id0;
            a.scnt[i] = (d.br == IMPC_REPLAN_SINGLE_FIRST && d.first) ? 0 : d.si;
            a.num_obs[i] = d.br == IMPC_REPLAN_FANOUT ? d.ki : d.br == IMPC_REPLAN_SINGLE_FIRST ? 0 : d.ci;
        }
        if (d.br == IMPC_REPLAN_FANOUT) {
            for (int s = 0; s < 6; s++) {
                const int id = s < 4 ? d.id0 : d.id1;
                if (!mine(id)) continue;
                const int64_t r = total(id - s0) + cl[(S + id - s0) * kPlanLanes + t]++;
                const int64_t f = xshape_base(a.I, a.K, id) + r;
                a.row_inst[f] = (int32_t)i;
                a.row_code[f] = (int8_t)s;
                sr[s] = (int32_t)r;
            }
        } else if (mine(d.id0)) {
            const int64_t r = cl[(d.id0 - s0) * kPlanLanes + t]++;
            const int64_t f = xshape_base(a.I, a.K, d.id0) + r;
            a.row_inst[f] = (int32_t)i;
            a.row_code[f] =
                (int8_t)(d.br == IMPC_REPLAN_SINGLE_FIRST ? IMPC_REPLAN_ROW_FIRST : IMPC_REPLAN_ROW_CURRENT);
            sr[0] = (int32_t)r;
            for (int s = 1; s < 6; s++) sr[s] = -1;
        }
    }
    if (t == 0) {
        for (int id = s0; id < s1; id++) {
            a.cnt[id] = total(id - s0);
            a.cnt[T + id] = total(id - s0) + total(S + id - s0);
        }
        if (blockIdx.x == 0)
            for (int b = 0; b < 3; b++) a.cnt[2 * T + b] = total(2 * S + b);
    }
}

__device__ inline double norm3(double a, double b, double c) {
#pragma clang fp contract(off)
    return sqrt((a * a + b * b) + c * c);
}

// maxCoeff (:762): the first most probable intent of one obstacle's [4] probabilities
__device__ inline int max_intent(const double *p) {
    int m = 0;
    for (int q = 1; q < 4; q++)
        if (p[q] > p[m]) m = q;
    return m;
}

struct PickArgs {
    int64_t I;
    int32_t K, N;
    const int8_t *branch;
    const int32_t *num_obs;
    const double *pos, *plan_states, *dyn_cur, *prob;
    const int32_t *prev_count;
    int32_t *ob, *ctype, *cslot, *slot_type;
    double *cprob;
};

// findClosestObstacle (:663-708, over the instance's K_i obstacles; a fan-out instance is never on
// its first plan) and getIntentComb's order (:719-756: std::sort of (weight, index) pairs, taken
// from the back); single-solve instances get -1.  As impc_intent_fanout_device (fanout.hip), with
// the obstacle count per instance.
__global__ __launch_bounds__(64) void k_pick(PickArgs a) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.I) return;
    int32_t *ct = a.ctype + 6 * i, *cs = a.cslot + 6 * i, *sty = a.slot_type + 6 * i;
    if (a.branch[i] != IMPC_REPLAN_FANOUT) {
        a.ob[i] = -1;
        for (int c = 0; c < 6; c++) ct[c] = cs[c] = sty[c] = -1;
        return;
    }
    const int K = a.K, Ki = a.num_obs[i];
    const double *cp = a.pos + 3 * i, *dc = a.dyn_cur + i * K * 3;
    int ob = -1;
    double minD = INFINITY;
    const int pc = a.prev_count[i];
    if (pc < 2) {  // distance to the current position (:676-686)
        for (int k = 0; k < Ki; k++) {
            const double d = norm3(cp[0] - dc[3 * k], cp[1] - dc[3 * k + 1], cp[2] - dc[3 * k + 2]);
            if (d < minD) {
                minD = d;
                ob = k;
            }
        }
    } else {  // direction-weighted, every term at states[0] / states[1] as written (:687-706)
        const double *s = a.plan_states + i * (int64_t)a.N * 8, *ns = s + 8;
        const double traj = atan2(ns[1] - s[1], ns[0] - s[0]);
        for (int k = 0; k < Ki; k++) {
            const double obs = atan2(dc[3 * k + 1] - s[1], dc[3 * k] - s[0]);
            const double d = norm3(s[0] - dc[3 * k], s[1] - dc[3 * k + 1], s[2] - dc[3 * k + 2]);
            double dist = 0.0;
            for (int j = 0; j < pc / 3; j++) {
                const double w = exp((double)-j);
                dist += w * d * (3.0 - cos(traj - obs));
                if (dist > minD) break;
            }
            if (dist < minD) {
                minD = dist;
                ob = k;
            }
        }
    }
    if (ob < 0) ob = 0;  // only with NaN inputs (the reference would index -1)
    a.ob[i] = ob;
    const double *pr = a.prob + (i * K + ob) * 4;
    const double w[6] = {pr[STOP], pr[LEFT], pr[RIGHT], pr[FORWARD], pr[LEFT] < pr[FORWARD] ? pr[FORWARD] : pr[LEFT],
                         pr[RIGHT] < pr[FORWARD] ? pr[FORWARD] : pr[RIGHT]};
    int type_at[6];
    for (int t = 0; t < 6; t++) {
        int pos = 0;
        for (int u = 0; u < 6; u++)
            if (w[t] < w[u] || (!(w[u] < w[t]) && t < u)) pos++;
        type_at[pos] = t;
    }
    int ns_ = 0, np_ = 0;
    for (int c = 0; c < 6; c++) {
        const int t = type_at[c];
        const int s = t < 4 ? ns_++ : 4 + np_++;
        ct[c] = t;
        cs[c] = s;
        sty[s] = t;
    }
    for (int q = 0; q < 4; q++) a.cprob[4 * i + q] = pr[q];
}

// Obstacle o of slot s's candidate (getIntentComb :731-768): the closest obstacle's intents
// first, then every other obstacle in index order at its most probable intent.
__device__ inline void cand_obstacle(int ob, int t, bool pair, int o, const double *prob_i, int &k, int &intent) {
    const int nfirst = pair ? 2 : 1;
    if (o < nfirst) {
        k = ob;
        constexpr int single_intent[4] = {STOP, LEFT, RIGHT, FORWARD};
        intent = t < 4 ? single_intent[t] : (o == 0 ? (t == 4 ? LEFT : RIGHT) : FORWARD);
    } else {
        const int q = o - nfirst;
        k = q < ob ? q : q + 1;
        intent = max_intent(prob_i + 4 * k);
    }
}

struct PrepArgs {
    int64_t I, n, total;
    int32_t K, L, T;
    const int64_t *cnt;
    const ShapeDev *sh;
    const int32_t *row_inst, *ob, *slot_type;
    const int8_t *row_code, *first_time;
    const double *plan_x, *prob;
    double cand_limit;
};

// One wavefront per row (grid-stride over every shape's capacity; rows past a shape's count are
// skipped): the warm start (solveTraj :485-509: the plan, or zeros on a first plan -- row I of
// plan_x), the row's time limit (candidates: timeLimit; single solves: none, :442-444) and the
// sources of its obstacle rows for the builder.
__global__ __launch_bounds__(64) void k_prep(PrepArgs a) {
    for (int64_t f = blockIdx.x; f < a.total; f += gridDim.x) {
        const int k = xshape_of(a.I, a.K, f);
        const int64_t r = f - xshape_base(a.I, a.K, k);
        if (r >= a.cnt[a.T + k]) continue;
        const ShapeDev sd = a.sh[k];
        const int64_t i = a.row_inst[f];
        const int code = a.row_code[f];
        const double *src = a.plan_x + ((code == IMPC_REPLAN_ROW_FIRST && a.first_time[i]) ? a.I : i) * a.n;
        double *dst = sd.xws + r * a.n;
        for (int64_t e = threadIdx.x; e < a.n; e += blockDim.x) dst[e] = src[e];
        if (threadIdx.x == 0) sd.tlim[r] = code < 6 ? a.cand_limit : 0.0;
        const int kd = xshape_dyn(a.K, k);
        for (int o = threadIdx.x; o < kd; o += blockDim.x) {
            int64_t off;
            if (code == IMPC_REPLAN_ROW_CURRENT) {  // held over the horizon
                off = ((i * a.K + o) * 3) << 1 | 1;
            } else {
                int kk, intent;
                cand_obstacle(a.ob[i], a.slot_type[6 * i + code], code >= 4, o, a.prob + i * a.K * 4, kk, intent);
                off = ((((i * a.K + kk) * 4 + intent) * (int64_t)a.L) * 3) << 1;
            }
            sd.osrc[r * kd + o] = off;
        }
    }
}

// The issue cut-off (:612-613) after the assembly, on the device clock; the solve count of each
// shape (its single solves always, its candidates when issued)
__global__ void k_issue(int32_t T, int64_t *cnt, int64_t *solve, unsigned long long *clk, int32_t *issued_out,
                        double elapsed_s, double tick, double cutoff) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long now = wall_clock64();
    clk[1] = now;
    const double elapsed = elapsed_s + (double)(now - clk[0]) * tick;
    const bool issued = !(cutoff > 0.0) || elapsed < cutoff;
    for (int k = 0; k < T; k++) solve[k] = issued ? cnt[T + k] : cnt[k];
    *issued_out = issued ? 1 : 0;
}

struct CandArgs {
    int64_t I, n;
    int32_t K, L, nst;
    const ShapeDev *sh;
    const int8_t *branch;
    const int32_t *num_obs, *scnt, *slot_row, *cslot, *slot_type, *ob;
    const int32_t *issued;
    const double *pred_pos, *pred_size, *prob;
    const double **x_cand;
    int32_t *dyn_count;
    int8_t *valid;
    double *dpos, *dsize;  // [I][6][K + 1][L][3], the selection's padded obstacle sets
};

// per (instance, candidate): solveTraj's success (impc_lib::solve_traj_ok, :475-478, :513-518) when issued,
// the pointer to the solution, the obstacle count
__global__ void k_cand(CandArgs a) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.I * 6; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / 6;
        if (a.branch[i] != IMPC_REPLAN_FANOUT) {
            a.valid[e] = 0;
            a.x_cand[e] = nullptr;
            a.dyn_count[e] = 0;
            continue;
        }
        const int s = a.cslot[e], k = s < 4 ? a.num_obs[i] : a.num_obs[i] + 1;
        const int id = shape_id(a.K, a.nst, k, a.scnt[i]);
        const int64_t r = a.slot_row[6 * i + s];
        a.valid[e] = (*a.issued && impc_lib::solve_traj_ok(a.sh[id].info[r])) ? 1 : 0;
        a.x_cand[e] = a.sh[id].x + r * a.n;
        a.dyn_count[e] = k;
    }
}

// the candidates' obstacle sets in the selection's padded layout (entries past a candidate's
// count are never read by the selection and are not written)
__global__ void k_sel_sets(CandArgs a) {
    const int64_t per_c = (int64_t)(a.K + 1) * a.L, total = a.I * 6 * per_c;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ic = e / per_c, i = ic / 6;
        if (a.branch[i] != IMPC_REPLAN_FANOUT) continue;
        const int rr = (int)(e - ic * per_c), o = rr / a.L, st = rr % a.L;
        const int s = a.cslot[ic];
        const bool pair = s >= 4;
        if (o >= a.num_obs[i] + (pair ? 1 : 0)) continue;
        int kk, intent;
        cand_obstacle(a.ob[i], a.slot_type[6 * i + s], pair, o, a.prob + i * a.K * 4, kk, intent);
        const int64_t src = (((i * a.K + kk) * 4 + intent) * (int64_t)a.L + st) * 3;
        for (int d = 0; d < 3; d++) {
            a.dpos[e * 3 + d] = a.pred_pos[src + d];
            a.dsize[e * 3 + d] = a.pred_size[src + d];
        }
    }
}

struct CommitArgs {
    int64_t I, n;
    int32_t N;
    const ShapeDev *sh;
    const int8_t *branch;
    const int32_t *shp, *slot_row, *best;
    const double *const *x_cand;
    double *plan_x, *plan_states;
    int32_t *prev_count;
    int8_t *first_time, *valid;
};

// every plan into the planner state (:629-639 / :653-657): the selected candidate of a fan-out
// instance, the single solve when solveTraj succeeded; an instance without a plan keeps its state
__global__ __launch_bounds__(64) void k_commit(CommitArgs a) {
    for (int64_t i = blockIdx.x; i < a.I; i += gridDim.x) {
        const double *src = nullptr;
        if (a.branch[i] == IMPC_REPLAN_FANOUT) {
            const int b = a.best[i];
            if (b >= 0) src = a.x_cand[6 * i + b];
        } else {
            const int k = a.shp[i];
            const int64_t r = a.slot_row[6 * i];
            if (impc_lib::solve_traj_ok(a.sh[k].info[r])) src = a.sh[k].x + r * a.n;
        }
        if (src) {
            for (int64_t e = threadIdx.x; e < a.n; e += blockDim.x) {
                const double v = src[e];
                a.plan_x[i * a.n + e] = v;
                if (e < (int64_t)8 * a.N) a.plan_states[i * (int64_t)a.N * 8 + e] = v;
            }
        }
        if (threadIdx.x == 0) {
            if (src) {
                a.prev_count[i] = a.N;
                a.first_time[i] = 0;
            }
            a.valid[i] = src ? 1 : 0;
        }
    }
}

struct PackArgs {
    int64_t I, max_inst, inst_base;
    int32_t N, P, rank, K, nst;
    const ShapeDev *sh;
    const int8_t *branch, *valid, *first_time;
    const int32_t *prev_count, *best, *num_obs, *scnt, *ob, *cslot, *slot_row, *shp;
    const double *weighted, *plan_states;
    uint64_t *out;  // [max_inst][8 + 8 P] 64-bit words
};

// What the replan decided per instance (impc_replan_record, include/impc_replan.h): one wavefront
// per record row, grid-stride over max_inst rows.  The header's eight 64-bit words are composed in
// registers (every value is uniform over the wavefront) and stored by lanes 0..7; the P stage
// states follow as 8 P words, lane-strided; rows past I are zero.  Words, not doubles: the copy is
// bit for bit whatever the value (OSQP_NAN plans included).  The instance's QP is located as
// k_cand / k_commit locate it.
__global__ __launch_bounds__(64) void k_pack_records(PackArgs a) {
    const int lane = threadIdx.x;
    const int64_t words = 8 + 8 * (int64_t)a.P;
    for (int64_t row = blockIdx.x; row < a.max_inst; row += gridDim.x) {
        uint64_t *dst = a.out + row * words;
        if (row >= a.I) {
            for (int64_t e = lane; e < words; e += 64) dst[e] = 0;
            continue;
        }
        const int64_t i = row;
        const int br = a.branch[i], b = a.best[i];
        int k = -1;
        int64_t r = -1;
        double score = 0.0;
        if (br == IMPC_REPLAN_FANOUT) {
            if (b >= 0) {
                const int s = a.cslot[6 * i + b];
                k = shape_id(a.K, a.nst, s < 4 ? a.num_obs[i] : a.num_obs[i] + 1, a.scnt[i]);
                r = a.slot_row[6 * i + s];
                score = a.weighted[6 * i + b];
            }
        } else {
            k = a.shp[i];
            r = a.slot_row[6 * i];
        }
        impc_info inf{};
        if (k >= 0 && r >= 0) inf = a.sh[k].info[r];
        if (lane < 8) {
            const auto lo_hi = [](int32_t lo, int32_t hi) { return (uint64_t)(uint32_t)lo | (uint64_t)(uint32_t)hi << 32; };
            uint64_t w;
            switch (lane) {
                case 0: w = lo_hi(a.rank, (int32_t)(a.inst_base + i)); break;
                case 1:
                    w = lo_hi((int32_t)((uint32_t)(uint8_t)br | (uint32_t)(uint8_t)a.valid[i] << 8 |
                                        (uint32_t)(uint8_t)(a.first_time[i] != 0) << 16 |
                                        (uint32_t)(uint8_t)(a.prev_count[i] > 0) << 24),
                              br == IMPC_REPLAN_FANOUT ? b : -1);
                    break;
                case 2: w = lo_hi(a.num_obs[i], a.ob[i]); break;
                case 3: w = lo_hi((int32_t)inf.status_val, (int32_t)inf.iter); break;
                case 4: w = (uint64_t)__double_as_longlong(inf.obj_val); break;
                case 5: w = (uint64_t)__double_as_longlong(score); break;
                case 6: w = (uint64_t)__double_as_longlong(inf.pri_res); break;
                default: w = (uint64_t)__double_as_longlong(inf.dua_res); break;
            }
            dst[lane] = w;
        }
        const uint64_t *src = (const uint64_t *)(a.plan_states + i * (int64_t)a.N * 8);
        for (int64_t e = lane; e < 8 * (int64_t)a.P; e += 64) dst[8 + e] = src[e];
    }
}

// mpcPlanner::getPos / getVel (mpcPlanner.cpp:1257-1290) of every instance with a plan
__global__ void k_advance(int64_t I, int32_t N, int64_t n, double ts, double t, const int8_t *__restrict__ valid,
                          const double *__restrict__ plan_x, double *__restrict__ pos, double *__restrict__ vel) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < I; i += (int64_t)gridDim.x * blockDim.x) {
        if (!valid[i]) continue;
        int idx = (int)floor(t / ts);
        const double dt = t - idx * ts;
        idx = max(0, min(idx, N - 1));
        const int nxt = min(idx + 1, N - 1);
        const double *s = plan_x + i * n + 8 * idx, *e = plan_x + i * n + 8 * nxt;
        for (int c = 0; c < 3; c++) {
            pos[3 * i + c] = s[c] + (e[c] - s[c]) / ts * dt;
            vel[3 * i + c] = s[3 + c] + (e[3 + c] - s[3 + c]) / ts * dt;
        }
    }
}

// device allocations of one replan object, released together
struct Arena {
    std::vector<void *> ptrs;
    int alloc(size_t bytes, void **out) {
        HIP_OK(hipMalloc(out, std::max<size_t>(bytes, 8)));
        ptrs.push_back(*out);
        return IMPC_OK;
    }
    template <class T>
    int get(size_t count, T **out) {
        return alloc(count * sizeof(T), (void **)out);
    }
    void release() { release_from(0); }
    // free everything allocated after the first `mark` allocations
    void release_from(size_t mark) {
        while (ptrs.size() > mark) {
            (void)hipFree(ptrs.back());
            ptrs.pop_back();
        }
    }
    void drop(void *p) {
        auto it = std::find(ptrs.begin(), ptrs.end(), p);
        if (it == ptrs.end()) return;
        (void)hipFree(p);
        ptrs.erase(it);
    }
};

// one QP shape of the replan (k dynamic- and nst static-obstacle rows per stage): its solver batch
// and on-device builder
struct Shape {
    int32_t k = 0, nst = 0;
    int64_t cap = 0;
    impc_qp_dims dm{};
    impc_batch batch = nullptr;
    impc_mpc_builder bld = nullptr;
    ShapeDev dev{};
};

}  // namespace impc_rp

using namespace impc_rp;

struct impc_replan_s {
    impc_ctx ctx = nullptr;
    impc_replan_config cfg{};
    int64_t I = 0, n = 0, rows = 0;
    int32_t N = 0, K = 0, L = 0, S = 0;
    int32_t T = 0;                      // shapes in all: S, or S + S_st (K + 2) once static counts were bound
    const int32_t *scount = nullptr;    // the bound per-instance static counts (DEVICE, the caller's)
    int32_t *scnt = nullptr;            // [I] static rows of each instance's QPs in the last run
    Arena mem;
    // planner state
    double *plan_x = nullptr, *plan_states = nullptr;
    int32_t *prev_count = nullptr;
    int8_t *first_time = nullptr, *valid = nullptr, *zeros8 = nullptr;
    double *plan_ref = nullptr;     // ref_ [I][N][3]
    int32_t *ref_count = nullptr;   // ref_.size() [I]
    bool has_state = false;         // a state from the caller (impc_replan_set_state) or a run
    // rows of the shapes and per-instance outputs
    int8_t *branch = nullptr, *row_code = nullptr;
    int32_t *row_inst = nullptr, *num_obs = nullptr, *shp = nullptr, *slot_row = nullptr, *slot_type = nullptr;
    int32_t *best = nullptr, *ob = nullptr, *ctype = nullptr, *cslot = nullptr, *issued = nullptr;
    int64_t *cnt = nullptr, *solve = nullptr;
    unsigned long long *clk = nullptr;
    double *cprob = nullptr;
    ShapeDev *d_sh = nullptr;
    // selection
    const double **x_cand = nullptr;
    int32_t *dyn_count = nullptr, *best_pos = nullptr;
    double *dyn_pos = nullptr, *dyn_size = nullptr, *scores = nullptr, *weighted = nullptr;
    int8_t *cvalid = nullptr;
    int32_t nst = 0;        // static obstacles per instance (cfg.num_static)
    std::vector<Shape> sh;  // by shape id: S = K + 2 shapes by dynamic-obstacle count, + the first plans' with
                            // statics, + the (k, s < S_st) pairs once static counts were bound
    std::vector<impc_batch> group;
    impc_replan_stats stats{};
    bool ran = false;
    double last_limit = 0.0;
    double last_total_s = 0.0;
};

namespace {

int fail(int code, const char *msg) { return impc_lib::set_error(code, msg); }

const char *const kNoShapes = "replan: the horizon / obstacle count is beyond the structured kernel "
                              "(the object only holds plan state)";
const char *const kNoStatic = "replan: per-instance static counts need num_static > 0";

// *no_kernel: the pattern is not one the structured kernel takes (the only kernel of the grouped solve)
int make_shape(impc_replan rp, Shape &s, int32_t k, int32_t nst, int64_t cap, bool *no_kernel) {
    s.k = k, s.nst = nst, s.cap = cap;
    IMPC_TRY(impc_mpc_dims(&rp->cfg.mpc, nst, k, &s.dm));
    std::vector<int64_t> Pp(s.dm.n + 1), Pi(std::max<int64_t>(s.dm.nnzP, 1)), Ap(s.dm.n + 1), Ai(s.dm.nnzA);
    IMPC_TRY(impc_mpc_build_pattern(&rp->cfg.mpc, nst, k, Pp.data(), Pi.data(), Ap.data(), Ai.data()));
    IMPC_TRY(impc_batch_create(rp->ctx, s.dm.n, s.dm.m, Pp.data(), Pi.data(), Ap.data(), Ai.data(), cap, &s.batch));
    IMPC_TRY(impc_batch_set_settings(s.batch, &rp->cfg.settings));
    if (rp->cfg.queue_order == IMPC_QUEUE_LONGEST_FIRST) {
        // impc.scenarios.queue_weight: ||q||_inf / (position weight (N - 1)) weighed 1:10
        const double qw = 1.0 / (10.0 * (rp->N - 1) * rp->cfg.mpc.position_weight);
        IMPC_TRY(impc_batch_set_queue_order(s.batch, IMPC_QUEUE_LONGEST_FIRST, qw));
    }
    if (int rc = impc_batch_set_kernel(s.batch, IMPC_KERNEL_STRUCTURED)) {
        *no_kernel = rc == IMPC_UNSUPPORTED;
        return rc;
    }
    IMPC_TRY(impc_mpc_builder_create(rp->ctx, &rp->cfg.mpc, nst, k, rp->L, &s.bld));
    impc_lib::BatchInputs bi{};
    IMPC_TRY(impc_lib::batch_inputs_view(s.batch, &bi));
    double *x = nullptr;
    impc_info *info = nullptr;
    IMPC_TRY(impc_batch_device_results(s.batch, &x, nullptr, &info));
    s.dev.xws = bi.xws;
    s.dev.x = x;
    s.dev.info = info;
    IMPC_TRY(impc_lib::batch_tlim_device(s.batch, &s.dev.tlim));
    IMPC_TRY(rp->mem.get((size_t)std::max<int64_t>(1, cap * k), &s.dev.osrc));
    return IMPC_OK;
}

void free_shape(Shape &s) {
    if (s.batch) (void)impc_batch_destroy(s.batch);
    if (s.bld) (void)impc_mpc_builder_destroy(s.bld);
    s.batch = nullptr;
    s.bld = nullptr;
}

unsigned grid_for(impc_replan rp, int64_t work, int per = 256) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + per - 1) / per, (int64_t)impc_lib::num_cu(rp->ctx) * 8));
}

}  // namespace

extern "C" {

int impc_replan_create(impc_ctx ctx, const impc_replan_config *cfg, impc_replan *out) {
    if (!ctx || !cfg || !out) return fail(IMPC_INVALID_ARGUMENT, "replan: null context, config or output");
    *out = nullptr;
    const int64_t I = cfg->instances;
    const int32_t N = cfg->mpc.horizon, K = cfg->num_obstacles, L = cfg->pred_len;
    if (I < 1 || I > ((int64_t)1 << 24) || N < 2 || K < 1 || K > kMaxObstacles || L < 1 || cfg->num_static < 0 ||
        cfg->num_static > kMaxObstacles)
        return fail(IMPC_INVALID_ARGUMENT, "replan: 1 <= instances <= 2^24, horizon >= 2, 1 <= num_obstacles <= 30, "
                                           "pred_len >= 1, 0 <= num_static <= 30");
    if (cfg->mpc.num_half_space != 0)
        return fail(IMPC_UNSUPPORTED, "replan: the live planner path has no FOV half-spaces (num_half_space = 0)");
    if (cfg->queue_order != IMPC_QUEUE_FIFO && cfg->queue_order != IMPC_QUEUE_LONGEST_FIRST)
        return fail(IMPC_INVALID_ARGUMENT, "replan: unknown queue order");
    HIP_OK(hipSetDevice(impc_lib::device(ctx)));
    std::unique_ptr<impc_replan_s> rp(new impc_replan_s());
    rp->ctx = ctx;
    rp->cfg = *cfg;
    rp->I = I, rp->N = N, rp->K = K, rp->L = L, rp->nst = cfg->num_static;
    rp->S = K + 2 + (rp->nst > 0 ? 1 : 0);
    rp->T = rp->S;
    rp->n = 13 * (int64_t)N - 5;
    rp->rows = shape_base(I, K, rp->S - 1) + shape_cap(I, K, rp->S - 1);
    const int64_t n = rp->n, S = rp->S;
    Arena &a = rp->mem;
    int rc = IMPC_OK;
    auto cleanup = [&]() {
        for (Shape &s : rp->sh) free_shape(s);
        rp->mem.release();
    };
#define RP_CK(expr)       \
    if ((rc = (expr))) {  \
        cleanup();        \
        return rc;        \
    }
    RP_CK(a.get((size_t)((I + 1) * n), &rp->plan_x));
    RP_CK(a.get((size_t)((I + 1) * N * 8), &rp->plan_states));
    RP_CK(a.get((size_t)I, &rp->prev_count));
    RP_CK(a.get((size_t)I, &rp->first_time));
    RP_CK(a.get((size_t)I, &rp->valid));
    RP_CK(a.get((size_t)I, &rp->zeros8));
    RP_CK(a.get((size_t)(I * N * 3), &rp->plan_ref));
    RP_CK(a.get((size_t)I, &rp->ref_count));
    RP_CK(a.get((size_t)I, &rp->branch));
    RP_CK(a.get((size_t)rp->rows, &rp->row_inst));
    RP_CK(a.get((size_t)rp->rows, &rp->row_code));
    RP_CK(a.get((size_t)I, &rp->num_obs));
    RP_CK(a.get((size_t)I, &rp->shp));
    RP_CK(a.get((size_t)I, &rp->scnt));
    RP_CK(a.get((size_t)(6 * I), &rp->slot_row));
    RP_CK(a.get((size_t)(6 * I), &rp->slot_type));
    RP_CK(a.get((size_t)I, &rp->best));
    RP_CK(a.get((size_t)I, &rp->ob));
    RP_CK(a.get((size_t)(6 * I), &rp->ctype));
    RP_CK(a.get((size_t)(6 * I), &rp->cslot));
    RP_CK(a.get((size_t)1, &rp->issued));
    RP_CK(a.get((size_t)(2 * S + 3), &rp->cnt));
    RP_CK(a.get((size_t)S, &rp->solve));
    RP_CK(a.get((size_t)2, &rp->clk));
    RP_CK(a.get((size_t)(4 * I), &rp->cprob));
    RP_CK(a.get((size_t)S, &rp->d_sh));
    RP_CK(a.get((size_t)(6 * I), &rp->x_cand));
    RP_CK(a.get((size_t)(6 * I), &rp->dyn_count));
    RP_CK(a.get((size_t)I, &rp->best_pos));
    RP_CK(a.get((size_t)(I * 6 * (K + 1) * L * 3), &rp->dyn_pos));
    RP_CK(a.get((size_t)(I * 6 * (K + 1) * L * 3), &rp->dyn_size));
    RP_CK(a.get((size_t)(I * 6 * 3), &rp->scores));
    RP_CK(a.get((size_t)(I * 6), &rp->weighted));
    RP_CK(a.get((size_t)(I * 6), &rp->cvalid));
    hipStream_t st = impc_lib::stream(ctx);
    if (hipMemsetAsync(rp->zeros8, 0, (size_t)I, st) != hipSuccess ||
        hipMemsetAsync(rp->valid, 0, (size_t)I, st) != hipSuccess ||
        hipMemsetAsync(rp->scnt, 0, sizeof(int32_t) * (size_t)I, st) != hipSuccess ||
        hipMemsetAsync(rp->plan_ref, 0, sizeof(double) * (size_t)(I * N * 3), st) != hipSuccess ||
        hipMemsetAsync(rp->cnt, 0, sizeof(int64_t) * (size_t)(2 * S + 3), st) != hipSuccess ||
        hipMemsetAsync(rp->solve, 0, sizeof(int64_t) * (size_t)S, st) != hipSuccess) {
        cleanup();
        return fail(IMPC_DEVICE_ERROR, "replan: memset");
    }
    // one solver batch per shape, each reading its QP count from device memory
    rp->sh.resize((size_t)S);
    std::vector<ShapeDev> hdev((size_t)S);
    for (int32_t k = 0; k < S; k++) {
        Shape &s = rp->sh[(size_t)k];
        bool no_kernel = false;
        rc = make_shape(rp.get(), s, shape_dyn(K, k), k <= K + 1 ? rp->nst : 0, shape_cap(I, K, k), &no_kernel);
        if (rc && no_kernel) {
            // A horizon or obstacle count beyond the structured kernel (13 N - 5 variables over its
            // lanes, or its LDS): the object holds the planner state -- set_state, set_ref, the records'
            // views, the plan-execution calls of impc_exec.h -- and impc_replan_run is unsupported.
            for (Shape &d : rp->sh) free_shape(d);
            rp->sh.clear();
            rp->group.clear();
            rc = IMPC_OK;
            break;
        }
        if (rc) {
            cleanup();
            return rc;
        }
        RP_CK(impc_lib::batch_set_active_device(s.batch, rp->solve + k));
        hdev[(size_t)k] = s.dev;
        rp->group.push_back(s.batch);
    }
    if (!rp->sh.empty())
        RP_CK(impc_copy_to_device(ctx, rp->d_sh, hdev.data(), (int64_t)(sizeof(ShapeDev) * hdev.size())));
#undef RP_CK
    rc = impc_replan_set_state(rp.get(), nullptr, nullptr);
    if (rc) {
        cleanup();
        return rc;
    }
    rp->has_state = false;
    *out = rp.release();
    return IMPC_OK;
}

int impc_replan_destroy(impc_replan rp) {
    if (!rp) return IMPC_OK;
    (void)hipSetDevice(impc_lib::device(rp->ctx));
    (void)impc_ctx_synchronize(rp->ctx);
    for (Shape &s : rp->sh) free_shape(s);
    rp->mem.release();
    delete rp;
    return IMPC_OK;
}

int impc_replan_set_state(impc_replan rp, const double *plan_x, const int8_t *first_time) {
    if (!rp) return fail(IMPC_INVALID_ARGUMENT, "null replan");
    const int64_t I = rp->I, n = rp->n, N = rp->N;
    std::vector<double> px((size_t)((I + 1) * n), 0.0), ps((size_t)((I + 1) * N * 8), 0.0);
    if (plan_x) std::memcpy(px.data(), plan_x, sizeof(double) * (size_t)(I * n));
    for (int64_t i = 0; i < I; i++) std::memcpy(&ps[(size_t)(i * N * 8)], &px[(size_t)(i * n)], sizeof(double) * 8 * N);
    std::vector<int8_t> ft((size_t)I, 1);
    if (first_time)
        for (int64_t i = 0; i < I; i++) ft[(size_t)i] = first_time[i] ? 1 : 0;
    std::vector<int32_t> pc((size_t)I);
    for (int64_t i = 0; i < I; i++) pc[(size_t)i] = ft[(size_t)i] ? 0 : (int32_t)N;  // currentStatesSol_.size()
    std::vector<int8_t> v((size_t)I, 0);
    IMPC_TRY(impc_copy_to_device(rp->ctx, rp->plan_x, px.data(), (int64_t)(px.size() * 8)));
    IMPC_TRY(impc_copy_to_device(rp->ctx, rp->plan_states, ps.data(), (int64_t)(ps.size() * 8)));
    IMPC_TRY(impc_copy_to_device(rp->ctx, rp->first_time, ft.data(), I));
    IMPC_TRY(impc_copy_to_device(rp->ctx, rp->prev_count, pc.data(), 4 * I));
    IMPC_TRY(impc_copy_to_device(rp->ctx, rp->valid, v.data(), I));
    std::vector<int32_t> rc((size_t)I, 0);  // ref_.empty()
    IMPC_TRY(impc_copy_to_device(rp->ctx, rp->ref_count, rc.data(), 4 * I));
    rp->has_state = true;
    return IMPC_OK;
}

int impc_replan_set_ref(impc_replan rp, const double *ref) {
    if (!rp || !ref) return fail(IMPC_INVALID_ARGUMENT, "replan set_ref: null object or ref");
    IMPC_TRY(impc_copy_to_device(rp->ctx, rp->plan_ref, ref, (int64_t)sizeof(double) * rp->I * rp->N * 3));
    hipLaunchKernelGGL(impc_exec::k_ref_count, dim3(grid_for(rp, rp->I)), dim3(256), 0, impc_lib::stream(rp->ctx), rp->I,
                       rp->N, rp->prev_count, rp->ref_count);
    HIP_OK(hipGetLastError());
    return impc_ctx_synchronize(rp->ctx);
}

int impc_replan_ref_device(impc_replan rp, double **plan_ref, int32_t **ref_count) {
    if (!rp) return fail(IMPC_INVALID_ARGUMENT, "null replan");
    if (plan_ref) *plan_ref = rp->plan_ref;
    if (ref_count) *ref_count = rp->ref_count;
    return IMPC_OK;
}

int impc_replan_run(impc_replan rp, const impc_replan_inputs *in) {
    using clk = std::chrono::steady_clock;
    const auto t_entry = clk::now();
    if (!rp || !in) return fail(IMPC_INVALID_ARGUMENT, "replan: null object or inputs");
    if (!in->pos || !in->vel || !in->xref || !in->dyn_cur || !in->pred_pos || !in->pred_size || !in->prob)
        return fail(IMPC_INVALID_ARGUMENT, "replan: pos, vel, xref, dyn_cur, pred_pos, pred_size, prob are required");
    if (in->cur_count && !in->cur_size) return fail(IMPC_INVALID_ARGUMENT, "replan: cur_count needs cur_size");
    if (rp->nst > 0 && (!in->st_centroid || !in->st_size || !in->st_yaw))
        return fail(IMPC_INVALID_ARGUMENT, "replan: num_static > 0 needs st_centroid, st_size, st_yaw");
    if (rp->sh.empty()) return fail(IMPC_UNSUPPORTED, kNoShapes);
    impc_ctx ctx = rp->ctx;
    HIP_OK(hipSetDevice(impc_lib::device(ctx)));
    hipStream_t st = impc_lib::stream(ctx);
    IMPC_TRY(impc_lib::ctx_order_after_all(ctx, st));
    const int64_t I = rp->I, n = rp->n;
    const int32_t N = rp->N, K = rp->K, L = rp->L;

    // ---- the branch and the rows of every instance (:593-606)
    const int32_t T = rp->T, tile = std::min<int32_t>(T, kPlanTile);
    PlanArgs pa{I,
                K,
                T,
                tile,
                rp->nst,
                rp->nst > 0 ? K + 2 : 0,
                Decide{rp->first_time, in->has_pred, in->num_pred, in->cur_count, K, in->cur_size ? 1 : 0},
                rp->scount,
                rp->branch,
                rp->num_obs,
                rp->shp,
                rp->slot_row,
                rp->best,
                rp->scnt,
                rp->row_inst,
                rp->row_code,
                rp->cnt,
                rp->clk};
    const size_t lds = sizeof(int32_t) * (size_t)(2 * tile + 3) * (kPlanLanes + kPlanLanes / 64);
    hipLaunchKernelGGL(k_plan_rows, dim3((unsigned)((T + tile - 1) / tile)), dim3(kPlanLanes), lds, st, pa);
    HIP_OK(hipGetLastError());
    // ---- the fan-out's closest obstacle and candidate order
    PickArgs pk{I, K, N, rp->branch, rp->num_obs, in->pos, rp->plan_states, in->dyn_cur, in->prob, rp->prev_count,
                rp->ob, rp->ctype, rp->cslot, rp->slot_type, rp->cprob};
    hipLaunchKernelGGL(k_pick, dim3((unsigned)((I + 63) / 64)), dim3(64), 0, st, pk);
    HIP_OK(hipGetLastError());
    // ---- warm starts, time limits, obstacle sources; the assembly of every shape in place
    // (timeLimit = max(solverTimeLimit_ - t, solverTimeLimit_) = solverTimeLimit_ for t >= 0, :614)
    const double tl = in->solver_time_limit > 0.0 ? in->solver_time_limit : rp->cfg.settings.time_limit;
    PrepArgs pp{I, n, rp->rows, K, L, T, rp->cnt, rp->d_sh, rp->row_inst, rp->ob, rp->slot_type, rp->row_code,
                rp->first_time, rp->plan_x, in->prob, tl};
    hipLaunchKernelGGL(k_prep, dim3(grid_for(rp, rp->rows, 1)), dim3(64), 0, st, pp);
    HIP_OK(hipGetLastError());
    for (int32_t k = 0; k < T; k++) {
        Shape &s = rp->sh[(size_t)k];
        impc_lib::BatchInputs bi{};
        IMPC_TRY(impc_lib::batch_inputs_begin(s.batch, &bi));
        const bool stat = s.nst > 0;  // its first s.nst of the instance's S_st boxes
        IMPC_TRY(impc_lib::build_rows(s.bld, s.cap, rp->cnt + T + k, rp->row_inst + xshape_base(I, K, k), s.dev.osrc,
                                    in->pos, in->vel, in->xref, rp->plan_states, in->pred_pos, in->pred_size,
                                    in->dyn_cur, in->cur_size, stat ? in->st_centroid : nullptr,
                                    stat ? in->st_size : nullptr, stat ? in->st_yaw : nullptr, rp->nst, bi, st));
        IMPC_TRY(impc_lib::batch_inputs_end(s.batch, true));
    }
    // ---- the issue cut-off on the device clock; ONE grouped solve over every shape
    hipLaunchKernelGGL(k_issue, dim3(1), dim3(64), 0, st, T, rp->cnt, rp->solve, rp->clk, rp->issued, in->elapsed_s,
                       impc_lib::tick_s(ctx), rp->cfg.issue_cutoff_s);
    HIP_OK(hipGetLastError());
    IMPC_TRY(impc_batch_solve_group(rp->group.data(), (int)rp->group.size(), nullptr));
    // ---- candidate validity, selection, commit
    CandArgs ca{I, n, K, L, rp->nst, rp->d_sh, rp->branch, rp->num_obs, rp->scnt, rp->slot_row, rp->cslot, rp->slot_type, rp->ob,
                rp->issued, in->pred_pos, in->pred_size, in->prob, rp->x_cand, rp->dyn_count, rp->cvalid, rp->dyn_pos,
                rp->dyn_size};
    hipLaunchKernelGGL(k_cand, dim3(grid_for(rp, 6 * I)), dim3(256), 0, st, ca);
    hipLaunchKernelGGL(k_sel_sets, dim3(grid_for(rp, I * 6 * (K + 1) * L)), dim3(256), 0, st, ca);
    HIP_OK(hipGetLastError());
    impc_select_params sp{};
    sp.horizon = N, sp.num_candidates = 6, sp.max_dynamic = K + 1, sp.pred_len = L;
    sp.num_static = rp->nst, sp.prev_len = N;  // getTrajectoryScore's staticObstacles (:620)
    sp.dynamic_safety_dist = rp->cfg.mpc.dynamic_safety_dist;
    sp.static_safety_dist = rp->cfg.mpc.static_safety_dist;
    // (a fan-out instance is never on a first plan: scnt is its s_i, S_st without bound counts)
    IMPC_TRY(impc_lib::select_best_counted(ctx, &sp, I, rp->x_cand, rp->cvalid, rp->zeros8, rp->plan_states,
                                         rp->prev_count, in->xref, rp->nst ? in->st_centroid : nullptr,
                                         rp->nst ? in->st_size : nullptr, rp->nst ? rp->scnt : nullptr, rp->dyn_count,
                                         rp->dyn_pos, rp->dyn_size, rp->cprob, rp->best, rp->best_pos, rp->scores,
                                         rp->weighted, nullptr));
    CommitArgs cm{I, n, N, rp->d_sh, rp->branch, rp->shp, rp->slot_row, rp->best, rp->x_cand, rp->plan_x,
                  rp->plan_states, rp->prev_count, rp->first_time, rp->valid};
    hipLaunchKernelGGL(k_commit, dim3(grid_for(rp, I, 1)), dim3(64), 0, st, cm);
    HIP_OK(hipGetLastError());
    // ---- ref_ of every committed plan (:639 / :657)
    hipLaunchKernelGGL(impc_exec::k_commit_ref, dim3(grid_for(rp, I * N * 3)), dim3(256), 0, st, I, N, rp->valid,
                       in->xref, rp->plan_ref, rp->ref_count);
    HIP_OK(hipGetLastError());
    rp->ran = true;
    rp->has_state = true;
    rp->last_limit = tl;
    rp->last_total_s = std::chrono::duration<double>(clk::now() - t_entry).count();
    return IMPC_OK;
}

int impc_replan_get_stats(impc_replan rp, impc_replan_stats *out) {
    if (!rp || !out) return fail(IMPC_INVALID_ARGUMENT, "replan: null object or output");
    std::memset(out, 0, sizeof(*out));
    if (!rp->ran) return IMPC_OK;
    IMPC_TRY(impc_ctx_synchronize(rp->ctx));
    const int32_t S = rp->T;
    std::vector<int64_t> c((size_t)(2 * S + 3));
    unsigned long long ck[2];
    int32_t iss = 0;
    IMPC_TRY(impc_copy_to_host(rp->ctx, c.data(), rp->cnt, (int64_t)(sizeof(int64_t) * c.size())));
    IMPC_TRY(impc_copy_to_host(rp->ctx, ck, rp->clk, (int64_t)sizeof(ck)));
    IMPC_TRY(impc_copy_to_host(rp->ctx, &iss, rp->issued, (int64_t)sizeof(iss)));
    out->fanout = c[(size_t)(2 * S + IMPC_REPLAN_FANOUT)];
    out->single_first = c[(size_t)(2 * S + IMPC_REPLAN_SINGLE_FIRST)];
    out->single_current = c[(size_t)(2 * S + IMPC_REPLAN_SINGLE_CURRENT)];
    out->issued = iss;
    out->time_limit = rp->last_limit;
    out->stage_s = (double)(ck[1] - ck[0]) * impc_lib::tick_s(rp->ctx);
    out->total_s = rp->last_total_s;
    return IMPC_OK;
}

int impc_replan_view_device(impc_replan rp, impc_replan_view *out) {
    if (!rp || !out) return fail(IMPC_INVALID_ARGUMENT, "replan: null object or output");
    out->plan_x = rp->plan_x, out->plan_states = rp->plan_states, out->prev_count = rp->prev_count;
    out->first_time = rp->first_time, out->valid = rp->valid, out->branch = rp->branch;
    out->best_cand = rp->best, out->ob_idx = rp->ob, out->cand_type = rp->ctype, out->cand_slot = rp->cslot;
    out->num_obs = rp->num_obs, out->slot_row = rp->slot_row, out->shape = rp->shp;
    out->weighted = rp->weighted;
    return IMPC_OK;
}

namespace {

int shape_view(impc_replan rp, int32_t id, impc_batch *batch, int64_t *count, const int32_t **row_inst,
               const int8_t **row_code, const double **Px, const double **q, const double **Ax, const double **l,
               const double **u) {
    const Shape &s = rp->sh[(size_t)id];
    int64_t c = 0;
    if (rp->ran) {
        IMPC_TRY(impc_ctx_synchronize(rp->ctx));
        IMPC_TRY(impc_copy_to_host(rp->ctx, &c, rp->solve + id, (int64_t)sizeof(c)));
    }
    if (batch) *batch = s.batch;
    if (count) *count = c;
    const int64_t base = xshape_base(rp->I, rp->K, id);
    if (row_inst) *row_inst = rp->row_inst + base;
    if (row_code) *row_code = rp->row_code + base;
    impc_lib::BatchInputs bi{};
    IMPC_TRY(impc_lib::batch_inputs_view(s.batch, &bi));  // the inputs of the last assembly
    if (Px) *Px = bi.Px;
    if (q) *q = bi.q;
    if (Ax) *Ax = bi.Ax;
    if (l) *l = bi.l;
    if (u) *u = bi.u;
    return IMPC_OK;
}

// The shapes (k, s < S_st) of an object whose static counts are bound for the first time: their
// solver batches and builders, and the row / count / shape tables at their full size (the last
// run's contents carried over).  On any failure everything created here is freed and the object
// is left as it was.
int extend_shapes(impc_replan rp) {
    impc_ctx ctx = rp->ctx;
    HIP_OK(hipSetDevice(impc_lib::device(ctx)));
    IMPC_TRY(impc_ctx_synchronize(ctx));
    const int64_t I = rp->I;
    const int32_t K = rp->K, S = rp->S, nst = rp->nst, T2 = S + nst * (K + 2);
    const int64_t rows2 = xshape_base(I, K, T2 - 1) + xshape_cap(I, K, T2 - 1);
    Arena &a = rp->mem;
    const size_t mark = a.ptrs.size();
    std::vector<Shape> ext((size_t)(T2 - S));
    int32_t *row_inst = nullptr;
    int8_t *row_code = nullptr;
    int64_t *cnt = nullptr, *solve = nullptr;
    ShapeDev *d_sh = nullptr;
    int rc = IMPC_OK;
    auto undo = [&]() {
        for (Shape &s : ext) free_shape(s);
        a.release_from(mark);
    };
#define RP_CK(expr)      \
    if ((rc = (expr))) { \
        undo();          \
        return rc;       \
    }
    for (int32_t id = S; id < T2; id++) {
        bool no_kernel = false;
        RP_CK(make_shape(rp, ext[(size_t)(id - S)], xshape_dyn(K, id), xshape_stat(K, nst, id), xshape_cap(I, K, id),
                         &no_kernel));
    }
    RP_CK(a.get((size_t)rows2, &row_inst));
    RP_CK(a.get((size_t)rows2, &row_code));
    RP_CK(a.get((size_t)(2 * T2 + 3), &cnt));
    RP_CK(a.get((size_t)T2, &solve));
    RP_CK(a.get((size_t)T2, &d_sh));
    // the last run's tables in the new layout (ids 0 .. S - 1 keep their rows and counts)
    std::vector<int64_t> c0((size_t)(2 * S + 3)), s0((size_t)S), c2((size_t)(2 * T2 + 3), 0), s2((size_t)T2, 0);
    RP_CK(impc_copy_to_host(ctx, c0.data(), rp->cnt, (int64_t)(sizeof(int64_t) * c0.size())));
    RP_CK(impc_copy_to_host(ctx, s0.data(), rp->solve, (int64_t)(sizeof(int64_t) * s0.size())));
    for (int32_t k = 0; k < S; k++) {
        c2[(size_t)k] = c0[(size_t)k];
        c2[(size_t)(T2 + k)] = c0[(size_t)(S + k)];
        s2[(size_t)k] = s0[(size_t)k];
    }
    for (int b = 0; b < 3; b++) c2[(size_t)(2 * T2 + b)] = c0[(size_t)(2 * S + b)];
    RP_CK(impc_copy_to_device(ctx, cnt, c2.data(), (int64_t)(sizeof(int64_t) * c2.size())));
    RP_CK(impc_copy_to_device(ctx, solve, s2.data(), (int64_t)(sizeof(int64_t) * s2.size())));
    std::vector<ShapeDev> hdev((size_t)T2);
    for (int32_t id = 0; id < T2; id++) hdev[(size_t)id] = id < S ? rp->sh[(size_t)id].dev : ext[(size_t)(id - S)].dev;
    RP_CK(impc_copy_to_device(ctx, d_sh, hdev.data(), (int64_t)(sizeof(ShapeDev) * hdev.size())));
    if (hipMemset(row_inst, 0, sizeof(int32_t) * (size_t)rows2) != hipSuccess ||
        hipMemset(row_code, 0, (size_t)rows2) != hipSuccess ||
        hipMemcpy(row_inst, rp->row_inst, sizeof(int32_t) * (size_t)rp->rows, hipMemcpyDeviceToDevice) != hipSuccess ||
        hipMemcpy(row_code, rp->row_code, (size_t)rp->rows, hipMemcpyDeviceToDevice) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        undo();
        return fail(IMPC_DEVICE_ERROR, "replan: copying the row tables");
    }
    for (int32_t id = S; id < T2; id++) {
        RP_CK(impc_lib::batch_set_active_device(ext[(size_t)(id - S)].batch, solve + id));
    }
#undef RP_CK
    // nothing below fails: the existing batches take the device count of the new table as they took the old
    for (int32_t k = 0; k < S; k++) (void)impc_lib::batch_set_active_device(rp->sh[(size_t)k].batch, solve + k);
    a.drop(rp->row_inst), a.drop(rp->row_code), a.drop(rp->cnt), a.drop(rp->solve), a.drop(rp->d_sh);
    rp->row_inst = row_inst, rp->row_code = row_code, rp->cnt = cnt, rp->solve = solve, rp->d_sh = d_sh;
    for (Shape &s : ext) {
        rp->sh.push_back(s);
        rp->group.push_back(s.batch);
    }
    rp->T = T2;
    rp->rows = rows2;
    return IMPC_OK;
}

}  // namespace

int impc_replan_bind_static_count(impc_replan rp, const int32_t *count_device) {
    if (!rp) return fail(IMPC_INVALID_ARGUMENT, "null replan");
    if (rp->nst <= 0) return fail(IMPC_INVALID_ARGUMENT, kNoStatic);
    if (rp->sh.empty()) return fail(IMPC_UNSUPPORTED, kNoShapes);
    if (count_device && rp->T == rp->S) IMPC_TRY(extend_shapes(rp));
    rp->scount = count_device;
    return IMPC_OK;
}

int impc_replan_static_count_device(impc_replan rp, const int32_t **count) {
    if (!rp || !count) return fail(IMPC_INVALID_ARGUMENT, "replan: null object or output");
    *count = rp->scnt;
    return IMPC_OK;
}

int impc_replan_shape(impc_replan rp, int32_t obstacles, impc_batch *batch, int64_t *count, const int32_t **row_inst,
                      const int8_t **row_code, const double **Px, const double **q, const double **Ax,
                      const double **l, const double **u) {
    if (!rp || obstacles < 0 || obstacles >= rp->S)
        return fail(IMPC_INVALID_ARGUMENT, "replan: shape must be in 0 .. num_obstacles + 1 (+ 2 with num_static)");
    if (rp->sh.empty()) return fail(IMPC_UNSUPPORTED, "replan: no solver shapes (the object only holds plan state)");
    return shape_view(rp, obstacles, batch, count, row_inst, row_code, Px, q, Ax, l, u);
}

int impc_replan_shape_static(impc_replan rp, int32_t obstacles, int32_t statics, impc_batch *batch, int64_t *count,
                             const int32_t **row_inst, const int8_t **row_code, const double **Px, const double **q,
                             const double **Ax, const double **l, const double **u) {
    if (!rp || obstacles < 0 || obstacles > rp->K + 1 || statics < 0 || statics > rp->nst)
        return fail(IMPC_INVALID_ARGUMENT, "replan: shape (k, s) must be in 0 .. num_obstacles + 1, 0 .. num_static");
    if (rp->sh.empty()) return fail(IMPC_UNSUPPORTED, "replan: no solver shapes (the object only holds plan state)");
    if (statics < rp->nst && rp->T == rp->S)
        return fail(IMPC_INVALID_ARGUMENT, "replan: shapes below num_static exist once static counts were bound");
    return shape_view(rp, shape_id(rp->K, rp->nst, obstacles, statics), batch, count, row_inst, row_code, Px, q, Ax, l,
                      u);
}

namespace {

int check_pack(impc_replan rp, int64_t inst_base, int32_t plan_steps, int64_t max_inst, const void *out) {
    if (!rp) return fail(IMPC_INVALID_ARGUMENT, "replan records: null replan");
    if (!out) return fail(IMPC_INVALID_ARGUMENT, "replan records: null output buffer");
    if ((uintptr_t)out % 8) return fail(IMPC_INVALID_ARGUMENT, "replan records: the buffer must be 8-byte aligned");
    if (plan_steps < 0 || plan_steps > rp->N)
        return fail(IMPC_INVALID_ARGUMENT, "replan records: plan_steps must be in 0 .. horizon");
    if (max_inst < rp->I) return fail(IMPC_INVALID_ARGUMENT, "replan records: max_inst is smaller than the instance count");
    if (inst_base < 0 || inst_base + rp->I > ((int64_t)1 << 31))
        return fail(IMPC_INVALID_ARGUMENT, "replan records: inst_base >= 0 and inst_base + instances <= 2^31");
    if (!rp->ran) return fail(IMPC_INVALID_ARGUMENT, "replan records: no impc_replan_run on this object yet");
    return IMPC_OK;
}

// k_pack_records on the context stream, after everything the replan queued
int pack_records(impc_replan rp, int32_t rank, int64_t inst_base, int32_t plan_steps, int64_t max_inst, void *out) {
    HIP_OK(hipSetDevice(impc_lib::device(rp->ctx)));
    hipStream_t st = impc_lib::stream(rp->ctx);
    IMPC_TRY(impc_lib::ctx_order_after_all(rp->ctx, st));
    PackArgs pk{rp->I, max_inst, inst_base, rp->N, plan_steps, rank, rp->K, rp->nst, rp->d_sh, rp->branch, rp->valid,
                rp->first_time, rp->prev_count, rp->best, rp->num_obs, rp->scnt, rp->ob, rp->cslot, rp->slot_row, rp->shp,
                rp->weighted,
                rp->plan_states, (uint64_t *)out};
    hipLaunchKernelGGL(k_pack_records, dim3(grid_for(rp, max_inst, 1)), dim3(64), 0, st, pk);
    HIP_OK(hipGetLastError());
    return IMPC_OK;
}

}  // namespace

int impc_replan_pack_device(impc_replan rp, int32_t rank, int64_t inst_base, int32_t plan_steps, int64_t max_inst,
                            void *out) {
    IMPC_TRY(check_pack(rp, inst_base, plan_steps, max_inst, out));
    return pack_records(rp, rank, inst_base, plan_steps, max_inst, out);
}

int impc_replan_gather(impc_replan rp, impc_comm comm, int64_t inst_base, int32_t plan_steps, int64_t max_inst,
                       void *recv) {
    if (!comm) return fail(IMPC_INVALID_ARGUMENT, "replan records: null communicator");
    IMPC_TRY(check_pack(rp, inst_base, plan_steps, max_inst, recv));
    impc_ctx cctx = nullptr;
    int rank = 0, world = 1;
    IMPC_TRY(impc_lib::comm_view(comm, &cctx, &rank, &world));
    if (cctx != rp->ctx) return fail(IMPC_INVALID_ARGUMENT, "replan records: the communicator belongs to another context");
    // in place: this rank's block is packed where the all-gather expects it (send = recv + rank * bytes)
    const int64_t bytes = max_inst * IMPC_REPLAN_RECORD_BYTES(plan_steps);
    char *own = (char *)recv + (int64_t)rank * bytes;
    IMPC_TRY(pack_records(rp, rank, inst_base, plan_steps, max_inst, own));
    return impc_comm_allgather(comm, own, recv, bytes, nullptr);
}

int impc_replan_advance_device(impc_replan rp, double t, double *pos, double *vel) {
    if (!rp || !pos || !vel || !(t >= 0.0)) return fail(IMPC_INVALID_ARGUMENT, "replan advance: t >= 0, pos, vel");
    HIP_OK(hipSetDevice(impc_lib::device(rp->ctx)));
    hipLaunchKernelGGL(k_advance, dim3(grid_for(rp, rp->I)), dim3(256), 0, impc_lib::stream(rp->ctx), rp->I, rp->N,
                       rp->n, rp->cfg.mpc.ts, t, rp->valid, rp->plan_x, pos, vel);
    HIP_OK(hipGetLastError());
    return IMPC_OK;
}

namespace {

int exec_state(impc_replan rp, impc_exec::State *s) {
    if (!rp->has_state)
        return fail(IMPC_INVALID_ARGUMENT, "replan: no plan state yet (impc_replan_set_state or impc_replan_run first)");
    if (!(rp->cfg.mpc.ts > 0.0)) return fail(IMPC_INVALID_ARGUMENT, "replan: mpc.ts must be positive");
    *s = impc_exec::State{rp->I, rp->n, rp->N, rp->K, rp->cfg.mpc.ts, rp->plan_x, rp->plan_ref, rp->prev_count,
                          rp->ref_count};
    return IMPC_OK;
}

}  // namespace

int impc_replan_target_device(impc_replan rp, const impc_target_params *p, const impc_target_in *in,
                              const impc_target_out *out) {
    if (!rp || !p || !in || !out) return fail(IMPC_INVALID_ARGUMENT, "replan target: null object, params, in or out");
    if (!in->t || !in->cur_pos || !in->odom_yaw || !out->pos || !out->vel || !out->acc || !out->yaw || !out->done)
        return fail(IMPC_INVALID_ARGUMENT, "replan target: t, cur_pos, odom_yaw, pos, vel, acc, yaw, done are required");
    if (p->yaw_mode < IMPC_YAW_FACING || p->yaw_mode > IMPC_YAW_SMOOTH)
        return fail(IMPC_INVALID_ARGUMENT, "replan target: unknown yaw_mode");
    if (p->yaw_mode == IMPC_YAW_FACING && !in->facing_yaw)
        return fail(IMPC_INVALID_ARGUMENT, "replan target: IMPC_YAW_FACING needs facing_yaw");
    impc_exec::State s{};
    IMPC_TRY(exec_state(rp, &s));
    HIP_OK(hipSetDevice(impc_lib::device(rp->ctx)));
    hipLaunchKernelGGL(impc_exec::k_target, dim3(grid_for(rp, rp->I, 1)), dim3(64), 0, impc_lib::stream(rp->ctx), s, *p,
                       *in, *out);
    HIP_OK(hipGetLastError());
    return IMPC_OK;
}

int impc_replan_check_device(impc_replan rp, const impc_check_in *in, const impc_check_out *out) {
    if (!rp || !in || !out) return fail(IMPC_INVALID_ARGUMENT, "replan check: null object, in or out");
    if (!in->t || !in->cur_pos || !out->map_step || !out->dyn_step || !out->replan)
        return fail(IMPC_INVALID_ARGUMENT, "replan check: t, cur_pos, map_step, dyn_step, replan are required");
    if (in->num_obs && (!in->ob_pos || !in->ob_size))
        return fail(IMPC_INVALID_ARGUMENT, "replan check: num_obs needs ob_pos and ob_size");
    if (in->occ_inflated &&
        (!(in->map.resolution > 0.0) || in->map.dims[0] < 1 || in->map.dims[1] < 1 || in->map.dims[2] < 1))
        return fail(IMPC_INVALID_ARGUMENT, "replan check: the map needs a positive resolution and dimensions");
    impc_exec::State s{};
    IMPC_TRY(exec_state(rp, &s));
    HIP_OK(hipSetDevice(impc_lib::device(rp->ctx)));
    hipLaunchKernelGGL(impc_exec::k_check, dim3(grid_for(rp, rp->I, 1)), dim3(64), 0, impc_lib::stream(rp->ctx), s, *in,
                       *out);
    HIP_OK(hipGetLastError());
    return IMPC_OK;
}

}  // extern "C"
