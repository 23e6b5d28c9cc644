// lib_internal.hpp -- the one internal interface of libimpc_qp.so: what the library's HIP
// translation units (select, fanout, predict, detect, mpc_build, comm, reftraj, replan_state,
// replan_run, cluster) take from the solver's unit, impc_qp.hip, which keeps the context and batch
// types private -- the error plumbing, the context's device / stream and its caller-stream ordering,
// a batch's device arrays -- and the two calls replan_run.hip makes into the builder's and the
// selection's units.  Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/impc_comm.h"
#include "../../include/impc_mpc.h"
#include "../../include/impc_qp.h"
#include "../../include/impc_select.h"

namespace impc_lib {
// solveTraj's success for one solved QP (mpcPlanner.cpp:475-478, :513-518): initSolver (osqp_setup)
// succeeded and solveProblem returned NoError.  osqp_solve's exitflag -- what solveProblem returns
// -- is 0 for every final status, infeasible, max-iter, time limit and a NON_CVX from the residual
// test included (x = OSQP_NAN then), and 1 only when an adaptive-rho refactorisation fails, which
// leaves the status UNSOLVED; a failed setup is reported as NON_CVX with setup_exitflag set.
__host__ __device__ inline bool solve_traj_ok(const impc_info &inf) {
    return inf.setup_exitflag == 0 && inf.status_val != IMPC_UNSOLVED;
}
// record the message of the last error (impc_last_error) and return `code`
int set_error(int code, const std::string &msg);
int num_cu(impc_ctx ctx);
int device(impc_ctx ctx);
hipStream_t stream(impc_ctx ctx);
// seconds per tick of the device clock the time limits run on (hipDeviceAttributeWallClockRate)
double tick_s(impc_ctx ctx);

// Caller streams against the context's own stream (impc_qp.hip): a launch on `st` first waits for
// what is queued on the context stream (order_launch) or, for consumers of results and scratch of
// other streams, for every noted launch as well (order_after_all), and is noted afterwards
// (note_launch) so that the entry points that rewrite what it reads wait for it; quiesce waits on
// the host for the context stream and every noted launch.
int ctx_order_launch(impc_ctx ctx, hipStream_t st);
int ctx_order_after_all(impc_ctx ctx, hipStream_t st);
int ctx_note_launch(impc_ctx ctx, hipStream_t st);
int ctx_quiesce(impc_ctx ctx);
// host -> device on `st`, finished when the call returns
int h2d_sync(hipStream_t st, void *dst, const void *src, size_t bytes);

// A batch's device input arrays (QP-major, capacity B rows), for producers that write them in
// place (the replan's assembly and warm-start gathers): begin orders the context stream after
// every launch that may still read them; end marks the batch's values (and a primal warm start
// with zero duals when warm_x) as set, as impc_batch_set_values_device + _warm_start_device do.
struct BatchInputs {
    double *Px, *q, *Ax, *l, *u, *xws;
    int64_t n, m, nnzP, nnzA, B;
};
int batch_inputs_begin(impc_batch b, BatchInputs *out);
int batch_inputs_end(impc_batch b, bool warm_x);
// the same arrays without ordering (read-only inspection after the caller synchronised)
int batch_inputs_view(impc_batch b, BatchInputs *out);
// a batch's context, capacity B and device result records [B] (the cost gather, comm.hip)
int batch_info_view(impc_batch b, impc_ctx *ctx, int64_t *B, const impc_info **info);
// The batch's active QP count from device memory (structured kernel): every later solve takes the
// first *d_count of its B QPs, the count read by the kernels themselves -- no host round trip
// between the producer that decides it and the solve.  NULL returns to B (impc_batch_set_active).
int batch_set_active_device(impc_batch b, const int64_t *d_count);
// The batch's per-QP time-limit array [B] on the device (allocated zero = no limit on first use),
// switched on for the following solves; producers write it in place.
int batch_tlim_device(impc_batch b, double **out);

// a communicator's context, rank and world size (comm.hip)
int comm_view(impc_comm c, impc_ctx *ctx, int *rank, int *world);
// The device builder over replan rows (mpc_build.hip Args: dcount / row_inst / osrc / held arrays;
// static obstacles per instance, [*][st_stride][3] / [*][st_stride] with st_stride >= the builder's S
// boxes per instance, of which the builder reads the first S; unread when the builder has none),
// writing the QP values into a batch's input arrays; asynchronous on `st`.
int build_rows(impc_mpc_builder bd, int64_t cap, const int64_t *dcount, const int32_t *row_inst, const int64_t *osrc,
               const double *pos, const double *vel, const double *xref, const double *lin, const double *pred_pos,
               const double *pred_size, const double *held_pos, const double *held_size, const double *st_centroid,
               const double *st_size, const double *st_yaw, int32_t st_stride, const BatchInputs &out, hipStream_t st);
// impc_select_best_device (select.hip) with a static-obstacle count per instance: st_count [I] in device
// memory (0 .. p->num_static, clamped), instance i's getTrajectoryScore scoring its first st_count[i] boxes of
// st_centroid / st_size [I][p->num_static][3]; NULL = p->num_static for every instance (the public call).
int select_best_counted(impc_ctx ctx, const impc_select_params *p, int64_t instances, const double *const *x_cand,
                        const int8_t *valid, const int8_t *first_time, const double *prev_states,
                        const int32_t *prev_count, const double *xref, const double *st_centroid,
                        const double *st_size, const int32_t *st_count, const int32_t *dyn_count, const double *dyn_pos,
                        const double *dyn_size, const double *prob, int32_t *best_cand, int32_t *best_pos,
                        double *scores, double *weighted, void *stream);
}  // namespace impc_lib

// a failed HIP call: its text and HIP's message become the last error, the function returns IMPC_DEVICE_ERROR
#define HIP_OK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess)                                                                                 \
            return impc_lib::set_error(IMPC_DEVICE_ERROR, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
// a failed library call: the function returns its code
#define IMPC_TRY(expr)       \
    do {                     \
        int rc_ = (expr);    \
        if (rc_) return rc_; \
    } while (0)
