// cluster_harness.cpp -- the serial form of include/impc_cluster.h over the functions of
// csrc/cluster.hpp, compiled for the host: what one instance's run computes, stage by stage, in the
// reference's own order (index-order 2-means sums included).  cluster_serial has the semantics of
// impc_cluster_run over host arrays.  With CLUSTER_HARNESS_MAIN it is a stand-alone program that runs
// a dumped set of cases (tests/test_cluster_host.py builds it with the sanitizers).
#ifndef __HIPCC__
#define __host__
#define __device__
#endif
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../intent-mpc_amd/csrc/cluster.hpp"

using namespace impc_clu;

namespace {

constexpr int kAxisCap = 1023;

struct Cloud {
    std::vector<double> tx, ty, tz;
    int nx = 0, ny = 0, nz = 0;
    std::vector<int> ix, iy, iz;  // per point
    std::vector<int> cellmap;     // lattice -> point
    int n() const { return (int)ix.size(); }
    void point(int p, double *o) const { o[0] = tx[ix[p]], o[1] = ty[iy[p]], o[2] = tz[iz[p]]; }
};

// the neighbours of p within eps, ascending (checkNearPoints, DBSCAN.h:87-97), through the stencil
template <class F>
void neighbours(const Cloud &c, const impc_cluster_params &pr, int p, F f) {
    const int rad = stencil_radius(pr.cloud_res, pr.eps);
    double pc[3];
    c.point(p, pc);
    for (int a = std::max(c.ix[p] - rad, 0); a <= std::min(c.ix[p] + rad, c.nx - 1); a++)
        for (int b = std::max(c.iy[p] - rad, 0); b <= std::min(c.iy[p] + rad, c.ny - 1); b++)
            for (int d = std::max(c.iz[p] - rad, 0); d <= std::min(c.iz[p] + rad, c.nz - 1); d++) {
                if (stencil_skip(a - c.ix[p], b - c.iy[p], d - c.iz[p], pr.cloud_res, pr.eps)) continue;
                const int q = c.cellmap[((size_t)a * c.ny + b) * c.nz + d];
                if (q < 0 || q == p) continue;
                const double qc[3] = {c.tx[a], c.ty[b], c.tz[d]};
                if (dbscan_dist(pc, qc) <= pr.eps) f(q);
            }
}

// The closed form of DBSCAN::run: label[p] = cluster index or IMPC_CLUSTER_NOISE; returns the clusters.
int dbscan(const Cloud &c, const impc_cluster_params &pr, std::vector<int> &label) {
    const int n = c.n();
    std::vector<char> core(n);
    for (int p = 0; p < n; p++) {
        int cnt = 0;
        neighbours(c, pr, p, [&](int) { cnt++; });
        core[p] = cnt >= pr.min_pts;
    }
    std::vector<int> start(n, -1), stack;
    std::vector<int> starts;
    for (int p = 0; p < n; p++) {  // components of the core points, by ascending smallest index
        if (!core[p] || start[p] >= 0) continue;
        starts.push_back(p);
        start[p] = p;
        stack.assign(1, p);
        while (!stack.empty()) {
            const int u = stack.back();
            stack.pop_back();
            neighbours(c, pr, u, [&](int q) {
                if (core[q] && start[q] < 0) start[q] = p, stack.push_back(q);
            });
        }
    }
    for (int p = 0; p < n; p++) {  // the border rule
        if (core[p]) continue;
        int best = -1;
        neighbours(c, pr, p, [&](int q) {
            if (core[q] && start[q] < p && (best < 0 || start[q] < best)) best = start[q];
        });
        start[p] = best;
    }
    label.assign(n, IMPC_CLUSTER_NOISE);
    for (int p = 0; p < n; p++)
        if (start[p] >= 0)
            label[p] = (int)(std::lower_bound(starts.begin(), starts.end(), start[p]) - starts.begin());
    return (int)starts.size();
}

void centre_of(const Cloud &c, const std::vector<int> &m, double *cen) {
    double lo[3], hi[3], p[3];
    c.point(m[0], lo), c.point(m[0], hi);
    for (int q : m) {
        c.point(q, p);
        for (int k = 0; k < 3; k++) {
            if (p[k] < lo[k])
                lo[k] = p[k];
            else if (p[k] > hi[k])
                hi[k] = p[k];
        }
    }
    for (int k = 0; k < 3; k++) cen[k] = mid(lo[k], hi[k]);
}

double orientation(const Cloud &c, const impc_cluster_params &pr, const double *tab, const std::vector<int> &m,
                   double *blo, double *bhi, int *bi) {
    double cen[3], best = 0.0;
    centre_of(c, m, cen);
    *bi = 0;
    for (int k = 0; k < 3; k++) blo[k] = bhi[k] = 0.0;
    for (int i = 0; i < pr.angle_num; i++) {
        double lo[3], hi[3], p[3], q[3];
        c.point(m[0], lo), c.point(m[0], hi);  // the UNROTATED points[0] (:239-240): it stays in the box
        for (int u : m) {
            c.point(u, p);
            rotate(tab[kAngleCols * i + 1], tab[kAngleCols * i + 2], p, cen, q);
            for (int k = 0; k < 3; k++) {
                if (q[k] < lo[k])
                    lo[k] = q[k];
                else if (q[k] > hi[k])
                    hi[k] = q[k];
            }
        }
        const double d = density_of((int)m.size(), lo, hi, pr.cloud_res);
        if (d > best) {
            best = d, *bi = i;
            for (int k = 0; k < 3; k++) blo[k] = lo[k], bhi[k] = hi[k];
        }
    }
    return best;
}

// runKmeans: false when a child is empty (or a seed does not exist)
bool kmeans(const Cloud &c, const impc_cluster_params &pr, const std::vector<int> &m, std::vector<int> &c0m,
            std::vector<int> &c1m) {
    double cen[3], p[3], c0[3], c1[3], d[2];
    centre_of(c, m, cen);
    const auto farthest = [&](const double *from) {
        double bd = 0.0;
        int b = -1;
        for (int u : m) {
            c.point(u, p);
            const double dist = seed_dist(p, from);
            if (dist > bd) bd = dist, b = u;
        }
        return b;
    };
    const int f = farthest(cen);
    if (f < 0) return false;
    c.point(f, c0);
    const int ff = farthest(c0);
    if (ff < 0) return false;
    c.point(ff, c1);
    for (int it = 0; it < pr.kmeans_iters; it++) {
        double s[2][3] = {{0, 0, 0}, {0, 0, 0}};
        int cnt[2] = {0, 0};
        for (int u : m) {
            c.point(u, p);
            const int l = classify2(p, c0, c1, d);
            for (int k = 0; k < 3; k++) s[l][k] += p[k];
            cnt[l]++;
        }
        for (int k = 0; k < 3; k++) {
            if (cnt[0]) s[0][k] /= cnt[0];
            if (cnt[1]) s[1][k] /= cnt[1];
            c0[k] = s[0][k], c1[k] = s[1][k];
        }
    }
    c0m.clear(), c1m.clear();
    for (int u : m) {
        c.point(u, p);
        (classify2(p, c0, c1, d) ? c1m : c0m).push_back(u);
    }
    return !c0m.empty() && !c1m.empty();
}

void run_one(const impc_cluster_params &pr, const double *tab, const impc_cluster_in &in, const impc_cluster_out &out,
             int64_t i) {
    if (in.active && !in.active[i]) return;
    const int P = pr.max_points, S = pr.max_boxes;
    Region r;
    region_of(pr, in.cur_pos + 3 * i, in.cur_vel + 3 * i, in.first && in.first[i], out.heading[i], r);
    out.heading[i] = r.heading;
    Cloud c;
    c.tx.resize(kAxisCap), c.ty.resize(kAxisCap), c.tz.resize(kAxisCap);
    c.nx = axis_table(r.x0, r.x1, pr.cloud_res, kAxisCap, c.tx.data());
    c.ny = axis_table(r.y0, r.y1, pr.cloud_res, kAxisCap, c.ty.data());
    c.nz = axis_table(pr.ground_height, pr.ceiling_height, pr.cloud_res, kAxisCap, c.tz.data());
    if (c.nx > kAxisCap || c.ny > kAxisCap || c.nz > kAxisCap) {
        out.flags[i] = IMPC_CLUSTER_POINTS;
        if (out.num_points) out.num_points[i] = -1;
        return;
    }
    c.cellmap.assign((size_t)c.nx * c.ny * c.nz, -1);
    int total = 0;
    for (int a = 0; a < c.nx; a++)
        for (int b = 0; b < c.ny; b++)
            for (int d = 0; d < c.nz; d++)
                if (in_cloud(r, in.map, in.map_max, in.occ_inflated, c.tx[a], c.ty[b], c.tz[d])) {
                    if (total < P) {
                        c.cellmap[((size_t)a * c.ny + b) * c.nz + d] = total;
                        c.ix.push_back(a), c.iy.push_back(b), c.iz.push_back(d);
                    }
                    total++;
                }
    if (out.num_points) out.num_points[i] = total;
    if (total == 0 || total > P) {
        out.flags[i] = total > P ? IMPC_CLUSTER_POINTS : 0;
        return;
    }
    const int n = total;
    if (out.cloud)
        for (int p = 0; p < n; p++) c.point(p, out.cloud + ((size_t)i * P + p) * 3);
    std::vector<int> label;
    const int ni = dbscan(c, pr, label);
    if (out.dbscan_label) std::copy(label.begin(), label.end(), out.dbscan_label + (size_t)i * P);
    if (out.num_initial) out.num_initial[i] = ni;
    if (ni > S) {
        out.flags[i] = IMPC_CLUSTER_BOXES;
        return;
    }
    std::vector<std::vector<int>> seq(ni);
    for (int p = 0; p < n; p++)
        if (label[p] >= 0) seq[label[p]].push_back(p);
    std::vector<char> done(ni, 0);
    double blo[3], bhi[3];
    int bi;
    for (int level = 0; level < pr.tree_level; level++) {
        std::vector<std::vector<int>> nseq;
        std::vector<char> ndone;
        bool empty = false;
        for (size_t k = 0; k < seq.size(); k++) {
            if (done[k] || orientation(c, pr, tab, seq[k], blo, bhi, &bi) >= pr.density_thresh) {
                nseq.push_back(seq[k]), ndone.push_back(1);
                continue;
            }
            std::vector<int> a, b;
            if (!kmeans(c, pr, seq[k], a, b)) empty = true;
            nseq.push_back(a), nseq.push_back(b), ndone.push_back(0), ndone.push_back(0);
        }
        if (empty || (int)nseq.size() > S) {
            out.flags[i] = empty ? IMPC_CLUSTER_EMPTY : IMPC_CLUSTER_BOXES;
            return;
        }
        seq.swap(nseq), done.swap(ndone);
    }
    out.flags[i] = 0;
    out.count[i] = (int32_t)seq.size();
    for (size_t k = 0; k < seq.size(); k++) {
        orientation(c, pr, tab, seq[k], blo, bhi, &bi);
        const size_t b = (size_t)i * S + k;
        box_of(blo, bhi, tab[kAngleCols * bi], out.centroid + 3 * b, out.size + 3 * b, out.yaw + b);
    }
}

}  // namespace

extern "C" int cluster_serial(const impc_cluster_params *pr, int64_t instances, const impc_cluster_in *in,
                              const impc_cluster_out *out, int threads) {
    if (!pr || !in || !out || instances < 1 || pr->angle_num < 1 || pr->max_points < 1 || pr->max_boxes < 1) return 1;
    std::vector<double> tab((size_t)kAngleCols * pr->angle_num);
    angle_table(pr->angle_num, tab.data());
    if (threads <= 1) {
        for (int64_t i = 0; i < instances; i++) run_one(*pr, tab.data(), *in, *out, i);
        return 0;
    }
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
            for (int64_t i = t; i < instances; i += threads) run_one(*pr, tab.data(), *in, *out, i);
        });
    for (auto &th : pool) th.join();
    return 0;
}

#ifdef CLUSTER_HARNESS_MAIN
// cluster_harness FILE: runs every case of a dump and prints the outputs' bytes as a checksum.  Dump
// (native endianness): int64 cases; per case impc_cluster_params, int64 I, impc_occ_map, double
// map_max[3], the grid's bytes, int64 calls, then per call int8 active[I], int8 first[I], double
// cur_pos[I][3], double cur_vel[I][3].  The state starts zeroed and is carried from call to call.
static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t cases = 0;
    if (!rd(f, &cases, 8)) return 2;
    unsigned long long sum = 1469598103934665603ull;
    const auto mix = [&](const void *p, size_t n) {
        for (size_t k = 0; k < n; k++) sum = (sum ^ ((const unsigned char *)p)[k]) * 1099511628211ull;
    };
    for (int64_t cs = 0; cs < cases; cs++) {
        impc_cluster_params pr;
        impc_cluster_in in{};
        int64_t I = 0, calls = 0;
        if (!rd(f, &pr, sizeof pr) || !rd(f, &I, 8) || !rd(f, &in.map, sizeof in.map) || !rd(f, in.map_max, 24)) return 2;
        std::vector<uint8_t> occ((size_t)in.map.dims[0] * in.map.dims[1] * in.map.dims[2]);
        if (!rd(f, occ.data(), occ.size()) || !rd(f, &calls, 8)) return 2;
        const size_t P = pr.max_points, S = pr.max_boxes, n = (size_t)I;
        std::vector<double> heading(n), cen(3 * n * S), size(3 * n * S), yaw(n * S), cloud(3 * n * P), pos(3 * n), vel(3 * n);
        std::vector<int32_t> count(n), flags(n), npts(n), ninit(n), lab(n * P);
        std::vector<int8_t> active(n), first(n);
        const impc_cluster_out out{heading.data(), count.data(), cen.data(),  size.data(),  yaw.data(),
                                   flags.data(),   npts.data(),  ninit.data(), cloud.data(), lab.data()};
        in.occ_inflated = occ.data(), in.active = active.data(), in.first = first.data();
        in.cur_pos = pos.data(), in.cur_vel = vel.data();
        for (int64_t k = 0; k < calls; k++) {
            if (!rd(f, active.data(), n) || !rd(f, first.data(), n) || !rd(f, pos.data(), 24 * n) ||
                !rd(f, vel.data(), 24 * n))
                return 2;
            if (cluster_serial(&pr, I, &in, &out, 1)) return 3;
            mix(heading.data(), 8 * n), mix(count.data(), 4 * n), mix(flags.data(), 4 * n), mix(npts.data(), 4 * n);
            for (size_t i = 0; i < n; i++) {
                const size_t b = (size_t)std::max(count[i], 0);
                mix(cen.data() + 3 * i * S, 24 * b), mix(size.data() + 3 * i * S, 24 * b), mix(yaw.data() + i * S, 8 * b);
            }
        }
    }
    fclose(f);
    printf("cases %lld checksum %016llx\n", (long long)cases, sum);
    return 0;
}
#endif
