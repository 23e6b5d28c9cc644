// comm.hip -- the RCCL communicator of the C-ABI (include/impc_comm.h, impc_comm_*), its own
// translation unit of libimpc_qp.so (context, batches and error plumbing through lib_internal.hpp).
//
// The only cross-GPU exchange of the path is the all-gather of every QP's cost
// record after the solve.  Records are packed on the device (one D2D copy per batch into a
// staging block, zero padded to the largest rank's QP count) and moved by one ncclAllGather on the
// solver's stream -- tens of MB at most (262,144 x 64 B), latency-bound over xGMI.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/impc_comm.h"
#include "lib_internal.hpp"

using impc_lib::set_error;

struct impc_comm_s {
    impc_ctx ctx = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    void *stage = nullptr;  // packed send block (grow-only)
    size_t stage_bytes = 0;
    double *scalar = nullptr;  // impc_comm_max scratch
};

#define NCCL_OK(expr)                                                                                  \
    do {                                                                                               \
        ncclResult_t r_ = (expr);                                                                      \
        if (r_ != ncclSuccess)                                                                         \
            return set_error(IMPC_DEVICE_ERROR, std::string(#expr ": ") + ncclGetErrorString(r_)); \
    } while (0)

int impc_lib::comm_view(impc_comm c, impc_ctx *ctx, int *rank, int *world) {
    if (!c || !ctx || !rank || !world) return set_error(IMPC_INVALID_ARGUMENT, "null communicator");
    *ctx = c->ctx, *rank = c->rank, *world = c->world;
    return IMPC_OK;
}

extern "C" {

int impc_comm_unique_id(unsigned char id[IMPC_COMM_ID_BYTES]) {
    if (!id) return set_error(IMPC_INVALID_ARGUMENT, "null id");
    static_assert(sizeof(ncclUniqueId) == IMPC_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    NCCL_OK(ncclGetUniqueId(&u));
    std::memcpy(id, &u, sizeof u);
    return IMPC_OK;
}

int impc_comm_create(impc_ctx ctx, const unsigned char id[IMPC_COMM_ID_BYTES], int rank, int world, impc_comm *out) {
    if (!ctx || !id || !out || world < 1 || rank < 0 || rank >= world)
        return set_error(IMPC_INVALID_ARGUMENT, "invalid communicator arguments");
    *out = nullptr;
    HIP_OK(hipSetDevice(impc_lib::device(ctx)));
    std::unique_ptr<impc_comm_s> c(new impc_comm_s());
    c->ctx = ctx;
    c->rank = rank;
    c->world = world;
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    NCCL_OK(ncclCommInitRank(&c->comm, world, u, rank));
    HIP_OK(hipMalloc((void **)&c->scalar, 2 * sizeof(double)));
    *out = c.release();
    return IMPC_OK;
}

int impc_comm_destroy(impc_comm c) {
    if (!c) return IMPC_OK;
    (void)hipSetDevice(impc_lib::device(c->ctx));
    (void)impc_lib::ctx_quiesce(c->ctx);
    if (c->comm) (void)ncclCommDestroy(c->comm);
    if (c->stage) (void)hipFree(c->stage);
    if (c->scalar) (void)hipFree(c->scalar);
    delete c;
    return IMPC_OK;
}

int impc_comm_allgather(impc_comm c, const void *send, void *recv, int64_t bytes, void *stream) {
    if (!c || bytes < 0 || (bytes && (!send || !recv))) return set_error(IMPC_INVALID_ARGUMENT, "invalid all-gather");
    HIP_OK(hipSetDevice(impc_lib::device(c->ctx)));
    hipStream_t st = stream ? (hipStream_t)stream : impc_lib::stream(c->ctx);
    IMPC_TRY(impc_lib::ctx_order_launch(c->ctx, st));
    NCCL_OK(ncclAllGather(send, recv, (size_t)bytes, ncclChar, c->comm, st));
    return impc_lib::ctx_note_launch(c->ctx, st);
}

int impc_comm_gather_info(impc_comm c, impc_batch *bs, int count, int64_t max_qps, impc_info *recv, void *stream) {
    if (!c || (count && !bs) || count < 0 || max_qps < 0 || !recv) return set_error(IMPC_INVALID_ARGUMENT, "invalid gather");
    int64_t total = 0;
    impc_ctx bctx = nullptr;
    int64_t B = 0;
    const impc_info *info = nullptr;
    for (int k = 0; k < count; k++) {
        if (!bs[k] || impc_lib::batch_info_view(bs[k], &bctx, &B, &info) || bctx != c->ctx)
            return set_error(IMPC_INVALID_ARGUMENT, "batch of another context");
        total += B;
    }
    if (total > max_qps) return set_error(IMPC_INVALID_ARGUMENT, "max_qps is smaller than this rank's QP count");
    HIP_OK(hipSetDevice(impc_lib::device(c->ctx)));
    hipStream_t st = stream ? (hipStream_t)stream : impc_lib::stream(c->ctx);
    const size_t bytes = sizeof(impc_info) * (size_t)std::max<int64_t>(max_qps, 1);
    if (bytes > c->stage_bytes) {
        IMPC_TRY(impc_lib::ctx_quiesce(c->ctx));  // no gather in flight reads the old block
        if (c->stage) HIP_OK(hipFree(c->stage));
        c->stage = nullptr;
        HIP_OK(hipMalloc(&c->stage, bytes));
        c->stage_bytes = bytes;
    }
    // the solves that wrote d_info, and an earlier gather still reading the staging block, may
    // have run on other streams: wait for all of them
    IMPC_TRY(impc_lib::ctx_order_after_all(c->ctx, st));
    char *dst = (char *)c->stage;
    for (int k = 0; k < count; k++) {
        IMPC_TRY(impc_lib::batch_info_view(bs[k], &bctx, &B, &info));
        const size_t nb = sizeof(impc_info) * (size_t)B;
        HIP_OK(hipMemcpyAsync(dst, info, nb, hipMemcpyDeviceToDevice, st));
        dst += nb;
    }
    if (total < max_qps) HIP_OK(hipMemsetAsync(dst, 0, sizeof(impc_info) * (size_t)(max_qps - total), st));
    NCCL_OK(ncclAllGather(c->stage, recv, sizeof(impc_info) * (size_t)max_qps, ncclChar, c->comm, st));
    return impc_lib::ctx_note_launch(c->ctx, st);
}

int impc_comm_max(impc_comm c, double *value) {
    if (!c || !value) return set_error(IMPC_INVALID_ARGUMENT, "invalid argument");
    HIP_OK(hipSetDevice(impc_lib::device(c->ctx)));
    hipStream_t st = impc_lib::stream(c->ctx);
    IMPC_TRY(impc_lib::ctx_quiesce(c->ctx));
    HIP_OK(hipMemcpyAsync(c->scalar, value, sizeof(double), hipMemcpyHostToDevice, st));
    NCCL_OK(ncclAllReduce(c->scalar, c->scalar + 1, 1, ncclFloat64, ncclMax, c->comm, st));
    HIP_OK(hipMemcpyAsync(value, c->scalar + 1, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return IMPC_OK;
}

}  // extern "C"
