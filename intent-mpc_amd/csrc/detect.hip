// detect.hip -- the detector's track store and range gate (include/impc_detect.h), its own
// translation unit of libimpc_qp.so.  The gate is one wavefront per planning instance: the lanes stride over the world's
// obstacles 64 at a time, each chunk takes one 64-bit ballot of the in-range predicate, a kept
// lane's slot is the running base plus the popcount of the ballot below it (an ordered compaction,
// no atomics, no LDS), and the whole wavefront then copies each kept track's history out of the
// ring, newest first, with coalesced loads and stores, and zero-fills the empty slots.  The kernels
// move bytes (a few K H 48-byte rows per instance): memory-bound and small next to the solve.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/impc_detect.h"
#include "detect_gate.hpp"
#include "lib_internal.hpp"

using impc_lib::set_error;

struct impc_tracks_s {
    impc_ctx ctx = nullptr;
    int64_t worlds = 0;
    int M = 0, H = 0;
    int head = 0, len = 0;  // ring slot of the newest entry; entries held (the same for every obstacle)
    double *pos = nullptr, *vel = nullptr, *size = nullptr;  // [worlds][M][H][3]
};

namespace impc_detect {

// histCB's push_front for every obstacle: entry `head` of each ring = the newest box
__global__ __launch_bounds__(256) void k_push(int64_t total3, int H, int head, const double *pos, const double *vel,
                                              const double *size, double *rpos, double *rvel, double *rsize) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (world, obstacle, component)
    if (t >= total3) return;
    const int64_t o = t / 3;
    const int c = (int)(t % 3);
    const int64_t at = (o * H + head) * 3 + c;
    rpos[at] = pos[t];
    rvel[at] = c == 2 ? 0.0 : vel[t];  // (Vx, Vy, 0) (:537)
    rsize[at] = size[t];
}

struct GateArgs {
    impc_detect_params p;
    impc_detect_out o;
    int64_t worlds;
    int M, H, head, len;
    const double *rpos, *rvel, *rsize;
    const double *robot_pos, *robot_yaw;
};

__global__ __launch_bounds__(64) void k_gate(GateArgs a) {
    const int64_t inst = blockIdx.x;
    const int lane = threadIdx.x;
    const int K = a.p.max_out, H = a.H, M = a.M;
    const int64_t w = a.worlds == 1 ? 0 : inst;
    const double robot[3] = {a.robot_pos[3 * inst], a.robot_pos[3 * inst + 1], a.robot_pos[3 * inst + 2]};
    const double yaw = a.robot_yaw ? a.robot_yaw[inst] : 0.0;
    const int64_t H3 = (int64_t)H * 3;
    int base = 0;  // obstacles in range so far (uniform over the wavefront)
    for (int j0 = 0; j0 < M; j0 += 64) {
        const int j = j0 + lane;
        bool keep = false;
        const int64_t newest = j < M ? (((w * M + j) * H + a.head) * 3) : 0;
        if (j < M && a.len > 0) keep = in_sensor_range(a.rpos + newest, robot, a.robot_yaw != nullptr, yaw, a.p.fov, a.p.range);
        const unsigned long long ballot = __ballot(keep);
        const int slot = base + __popcll(ballot & ((1ull << lane) - 1ull));
        if (keep && slot < K) {  // the kept lane writes its own slot's scalars and newest entry
            const int64_t s = inst * K + slot;
            if (a.o.src) a.o.src[s] = j;
            if (a.o.hist_len) a.o.hist_len[s] = a.len;
            for (int c = 0; c < 3; c++) {
                if (a.o.cur_pos) a.o.cur_pos[3 * s + c] = a.rpos[newest + c];
                if (a.o.cur_vel) a.o.cur_vel[3 * s + c] = a.rvel[newest + c];
                if (a.o.cur_size) a.o.cur_size[3 * s + c] = a.rsize[newest + c] + a.p.robot_size[c];
            }
        }
        if (a.o.pos_hist || a.o.vel_hist) {
            // the whole wavefront copies each kept track's history, un-rotating the ring
            unsigned long long b = ballot;
            for (int s = base; b && s < K; s++) {
                const int jj = j0 + __ffsll((long long)b) - 1;
                b &= b - 1;
                const int64_t ring = (w * M + jj) * H3, dst = (inst * K + s) * H3;
                for (int64_t x = lane; x < H3; x += 64) {
                    const int e = (int)(x / 3);
                    int r = a.head + e;
                    if (r >= H) r -= H;
                    const int64_t from = ring + (int64_t)r * 3 + (x - 3 * (int64_t)e);
                    const bool held = e < a.len;
                    if (a.o.pos_hist) a.o.pos_hist[dst + x] = held ? a.rpos[from] : 0.0;
                    if (a.o.vel_hist) a.o.vel_hist[dst + x] = held ? a.rvel[from] : 0.0;
                }
            }
        }
        base += __popcll(ballot);
    }
    const int num = base < K ? base : K;
    if (lane == 0) {
        a.o.num[inst] = num;
        if (a.o.in_range) a.o.in_range[inst] = base;
    }
    // the empty slots, written on every call
    const int64_t s0 = inst * K + num;
    const int empty = K - num;
    for (int x = lane; x < empty; x += 64) {
        if (a.o.src) a.o.src[s0 + x] = -1;
        if (a.o.hist_len) a.o.hist_len[s0 + x] = 0;
    }
    for (int x = lane; x < empty * 3; x += 64) {
        if (a.o.cur_pos) a.o.cur_pos[3 * s0 + x] = 0.0;
        if (a.o.cur_vel) a.o.cur_vel[3 * s0 + x] = 0.0;
        if (a.o.cur_size) a.o.cur_size[3 * s0 + x] = 0.0;
    }
    for (int64_t x = lane; x < empty * H3; x += 64) {
        if (a.o.pos_hist) a.o.pos_hist[s0 * H3 + x] = 0.0;
        if (a.o.vel_hist) a.o.vel_hist[s0 * H3 + x] = 0.0;
    }
}

}  // namespace impc_detect

extern "C" int impc_tracks_create(impc_ctx ctx, int64_t worlds, int32_t M, int32_t H, impc_tracks *out) {
    if (!ctx || !out) return set_error(IMPC_INVALID_ARGUMENT, "tracks: null context or output");
    if (worlds < 1 || M < 1 || H < 1) return set_error(IMPC_INVALID_ARGUMENT, "tracks: worlds >= 1, M >= 1, H >= 1");
    if (worlds > ((int64_t)1 << 24) || (double)worlds * M * H * 24.0 > 6.4e10)
        return set_error(IMPC_INVALID_ARGUMENT, "tracks: worlds <= 2^24 and at most 64 GB of history per array");
    HIP_OK(hipSetDevice(impc_lib::device(ctx)));
    impc_tracks tr = new impc_tracks_s;
    tr->ctx = ctx;
    tr->worlds = worlds;
    tr->M = M;
    tr->H = H;
    const size_t bytes = sizeof(double) * 3 * (size_t)worlds * M * H;
    char *buf = nullptr;
    hipError_t e = hipMalloc((void **)&buf, 3 * bytes);
    if (e == hipSuccess) e = hipMemsetAsync(buf, 0, 3 * bytes, impc_lib::stream(ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(impc_lib::stream(ctx));
    if (e != hipSuccess) {
        if (buf) (void)hipFree(buf);
        delete tr;
        return set_error(IMPC_DEVICE_ERROR, std::string("tracks: allocation: ") + hipGetErrorString(e));
    }
    tr->pos = (double *)buf;
    tr->vel = (double *)(buf + bytes);
    tr->size = (double *)(buf + 2 * bytes);
    *out = tr;
    return IMPC_OK;
}

extern "C" int impc_tracks_destroy(impc_tracks tr) {
    if (!tr) return IMPC_OK;
    (void)hipSetDevice(impc_lib::device(tr->ctx));
    (void)hipStreamSynchronize(impc_lib::stream(tr->ctx));
    (void)hipFree(tr->pos);  // one allocation: pos, vel, size
    delete tr;
    return IMPC_OK;
}

extern "C" int impc_tracks_reset(impc_tracks tr) {
    if (!tr) return set_error(IMPC_INVALID_ARGUMENT, "null tracks");
    tr->head = tr->len = 0;
    return IMPC_OK;
}

extern "C" int impc_tracks_push_device(impc_tracks tr, const double *pos, const double *vel, const double *size,
                                       void *stream) {
    if (!tr || !pos || !vel || !size) return set_error(IMPC_INVALID_ARGUMENT, "tracks push: null argument");
    HIP_OK(hipSetDevice(impc_lib::device(tr->ctx)));
    hipStream_t st = stream ? (hipStream_t)stream : impc_lib::stream(tr->ctx);
    const int head = tr->head == 0 ? tr->H - 1 : tr->head - 1;  // push_front; at H entries it lands on the oldest
    const int64_t total3 = tr->worlds * tr->M * 3;
    hipLaunchKernelGGL(impc_detect::k_push, dim3((unsigned)((total3 + 255) / 256)), dim3(256), 0, st, total3, tr->H,
                       head, pos, vel, size, tr->pos, tr->vel, tr->size);
    HIP_OK(hipGetLastError());
    tr->head = head;
    if (tr->len < tr->H) tr->len++;
    return IMPC_OK;
}

static int detect_check(impc_tracks tr, const impc_detect_params *p, int64_t I, const double *robot_pos,
                        const double *robot_yaw, const impc_detect_out *out) {
    if (!tr || !p || !out) return set_error(IMPC_INVALID_ARGUMENT, "detect: null tracks, parameters or outputs");
    if (p->max_out < 1) return set_error(IMPC_INVALID_ARGUMENT, "detect: max_out >= 1");
    if (I < 0 || I > ((int64_t)1 << 24)) return set_error(IMPC_INVALID_ARGUMENT, "detect: 0 <= instances <= 2^24");
    if (tr->worlds != 1 && I != tr->worlds)
        return set_error(IMPC_INVALID_ARGUMENT, "detect: instances must equal the store's worlds (or worlds = 1)");
    if (!(p->fov >= 2 * M_PI) && !robot_yaw) return set_error(IMPC_INVALID_ARGUMENT, "detect: fov < 2 pi needs robot_yaw");
    if (I > 0 && (!robot_pos || !out->num)) return set_error(IMPC_INVALID_ARGUMENT, "detect: robot_pos and out.num are required");
    return IMPC_OK;
}

extern "C" int impc_detect_gather_device(impc_tracks tr, const impc_detect_params *p, int64_t I,
                                         const double *robot_pos, const double *robot_yaw,
                                         const impc_detect_out *out, void *stream) {
    IMPC_TRY(detect_check(tr, p, I, robot_pos, robot_yaw, out));
    if (I == 0) return IMPC_OK;
    HIP_OK(hipSetDevice(impc_lib::device(tr->ctx)));
    hipStream_t st = stream ? (hipStream_t)stream : impc_lib::stream(tr->ctx);
    impc_detect::GateArgs a{*p, *out, tr->worlds, tr->M, tr->H, tr->head, tr->len, tr->pos, tr->vel, tr->size,
                            robot_pos, robot_yaw};
    hipLaunchKernelGGL(impc_detect::k_gate, dim3((unsigned)I), dim3(64), 0, st, a);
    HIP_OK(hipGetLastError());
    return IMPC_OK;
}

extern "C" int impc_detect_gather(impc_tracks tr, const impc_detect_params *p, int64_t I, const double *robot_pos,
                                  const double *robot_yaw, const impc_detect_out *out) {
    IMPC_TRY(detect_check(tr, p, I, robot_pos, robot_yaw, out));
    if (I == 0) return IMPC_OK;
    HIP_OK(hipSetDevice(impc_lib::device(tr->ctx)));
    hipStream_t st = impc_lib::stream(tr->ctx);
    const size_t K = (size_t)p->max_out, IK = (size_t)I * K, H3 = (size_t)tr->H * 3;
    // device copies of the inputs and of every output asked for, in one allocation
    struct Part {
        void *host;
        size_t bytes, at;
    };
    Part parts[9] = {{out->num, 4 * (size_t)I, 0},      {out->in_range, 4 * (size_t)I, 0}, {out->src, 4 * IK, 0},
                     {out->hist_len, 4 * IK, 0},        {out->pos_hist, 8 * IK * H3, 0},   {out->vel_hist, 8 * IK * H3, 0},
                     {out->cur_pos, 8 * IK * 3, 0},     {out->cur_vel, 8 * IK * 3, 0},     {out->cur_size, 8 * IK * 3, 0}};
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    size_t total = up(24 * (size_t)I) + up(8 * (size_t)I);
    for (Part &q : parts) {
        q.at = total;
        if (q.host) total += up(q.bytes);
    }
    char *buf = nullptr;
    HIP_OK(hipMalloc((void **)&buf, total));
    double *dpos = (double *)buf, *dyaw = robot_yaw ? (double *)(buf + up(24 * (size_t)I)) : nullptr;
    auto dev = [&](int k) { return parts[k].host ? (void *)(buf + parts[k].at) : nullptr; };
    impc_detect_out d{(int32_t *)dev(0), (int32_t *)dev(1), (int32_t *)dev(2), (int32_t *)dev(3), (double *)dev(4),
                      (double *)dev(5),  (double *)dev(6),  (double *)dev(7),  (double *)dev(8)};
    int rc = impc_lib::h2d_sync(st, dpos, robot_pos, 24 * (size_t)I);
    if (!rc && robot_yaw) rc = impc_lib::h2d_sync(st, dyaw, robot_yaw, 8 * (size_t)I);
    if (!rc) rc = impc_detect_gather_device(tr, p, I, dpos, dyaw, &d, nullptr);
    if (!rc) {
        hipError_t e = hipSuccess;
        for (int k = 0; k < 9 && e == hipSuccess; k++)
            if (parts[k].host) e = hipMemcpyAsync(parts[k].host, buf + parts[k].at, parts[k].bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = set_error(IMPC_DEVICE_ERROR, std::string("detect download: ") + hipGetErrorString(e));
    }
    (void)hipFree(buf);
    return rc;
}
