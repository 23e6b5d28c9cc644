// cluster.hip -- include/impc_cluster.h: staticObstacleClusteringCB + obstacleClustering::run +
// getStaticObstacles for a batch of planning instances, one workgroup per instance (grid-stride),
// over the arithmetic of cluster.hpp.  Phases, separated by workgroup barriers:
//   1  heading, region, the three axis tables (one thread: a few dozen running-sum additions)
//   2  lattice scan, compacted in loop order (x outer, y, z inner): each wavefront owns a contiguous
//      quarter of the lattice, counts its points (ballot + popcount), and after one barrier writes
//      them behind the wavefronts before it -- packed lattice indices in LDS, lattice -> point map
//      in the workspace
//   3  core counts over the stencil of the lattice -> point map
//   4  components of the core points: min-label propagation with pointer jumping to a fixed point
//   5  the border rule, cluster ranks (the same two-pass scan), points ordered by (cluster, index)
//   6  the tree: one wavefront per node -- box, angle search, 2-means and the stable partition of
//      the node's segment are wave reductions with no workgroup barrier; one thread renumbers the
//      node list between levels
//   7  box emission, one wavefront per leaf
// DBSCAN's visiting order has a closed form: clusters are the components of the
// core points numbered by ascending smallest core index, a border point joins the adjacent cluster
// with the smallest start index below its own index, and is noise otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "cluster.hpp"
#include "lib_internal.hpp"

namespace impc_clu {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kAxisMax = 1023;  // ten bits per axis in a packed lattice index
constexpr double kInf = __builtin_huge_val();

struct Shared {
    Region r;
    int nx, ny, nz, n, nn, flags, changed, cur;
    int wc[kWaves];
};

struct Layout {  // the dynamic LDS of one workgroup, in bytes from its start
    int capx, capy, capz, P, S;
    __host__ __device__ size_t tab() const { return 0; }
    __host__ __device__ size_t shared() const { return 8 * (size_t)(capx + capy + capz); }
    __host__ __device__ size_t ints() const { return shared() + ((sizeof(Shared) + 7) & ~(size_t)7); }
    __host__ __device__ size_t bytes_at() const { return ints() + 4 * ((size_t)3 * P + 8 * (size_t)S); }
    __host__ __device__ size_t total() const { return (bytes_at() + P + 7) & ~(size_t)7; }
};

struct Args {
    impc_cluster_params pr;
    impc_cluster_in in;
    impc_cluster_out out;
    Layout lay;
    int64_t I, cells;
    int r2max;            // View::r2max
    int32_t *cellmap;     // [gridDim.x][cells]
    const double *angles;  // [angle_num][kAngleCols]
};

__device__ inline int lane_id() { return threadIdx.x & 63; }
__device__ inline int rank_in(unsigned long long m) {
    return __popcll(m & ((1ull << lane_id()) - 1ull));
}
__device__ inline void wave_sync() {  // LDS written by other lanes of this wavefront is visible after it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ inline double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline double wave_sum(double v) {
#pragma clang fp contract(off)
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}
__device__ inline int wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One workgroup's view of its instance
struct View {
    const double *tx, *ty, *tz;
    Shared *sh;
    int *pts, *lab, *ord, *nbeg, *nend, *nfin, *nsplit, *ncnt;  // nbeg / nend / nfin: [2][S]
    uint8_t *flg;
    int32_t *cellmap;
    const double *angles;
    int P, S;
    int r2max;  // the largest i^2 + j^2 + k^2 of a stencil offset that stencil_far does not rule out

    __device__ void coords(int packed, double *p) const {
        p[0] = tx[packed >> 20], p[1] = ty[(packed >> 10) & 1023], p[2] = tz[packed & 1023];
    }
    __device__ void point(int idx, double *p) const { coords(pts[idx], p); }
};

// calls f(q, coordinates of q) for every point q != p within the stencil of p's lattice cell
template <class F>
__device__ inline void for_neighbours(const View &v, const impc_cluster_params &pr, int p, F f) {
    const Shared &sh = *v.sh;
    const int pk = v.pts[p], ix = pk >> 20, iy = (pk >> 10) & 1023, iz = pk & 1023;
    const int rad = stencil_radius(pr.cloud_res, pr.eps);
    const int x0 = max(ix - rad, 0), x1 = min(ix + rad, sh.nx - 1);
    const int y0 = max(iy - rad, 0), y1 = min(iy + rad, sh.ny - 1);
    const int z0 = max(iz - rad, 0), z1 = min(iz + rad, sh.nz - 1);
    const int r2 = v.r2max;  // (an integer test; whole columns of the stencil are skipped by it too)
    for (int a = x0; a <= x1; a++)
        for (int b = y0; b <= y1; b++) {
            const int dab = (a - ix) * (a - ix) + (b - iy) * (b - iy);
            if (dab > r2) continue;
            for (int c = z0; c <= z1; c++) {
                if (dab + (c - iz) * (c - iz) > r2) continue;
                const int q = v.cellmap[(a * sh.ny + b) * sh.nz + c];
                if (q < 0 || q == p) continue;
                const double qc[3] = {v.tx[a], v.ty[b], v.tz[c]};
                f(q, qc);
            }
        }
}

// Two-pass order-preserving count / rank over items 0 .. L - 1: each wavefront owns a contiguous
// span.  pred(c) must be pure.  put(c, keep, index) is called for every item when `place` allows it
// (uniform; called with the total), with the item's index among the kept ones.  Returns the total.
// Called by the whole workgroup, converged.
template <class Pred, class Place, class Put>
__device__ inline int block_compact(Shared *sh, int L, Pred pred, Place place, Put put) {
    const int w = threadIdx.x >> 6, lane = lane_id();
    const int span = ((L + kThreads - 1) / kThreads) * 64;
    const int lo = min(w * span, L), hi = min(lo + span, L);
    int cnt = 0;
    for (int c0 = lo; c0 < hi; c0 += 64) {
        const int c = c0 + lane;
        cnt += __popcll(__ballot(c < hi && pred(c)));
    }
    if (lane == 0) sh->wc[w] = cnt;
    __syncthreads();
    int off = 0, total = 0;
    for (int k = 0; k < kWaves; k++) {
        if (k < w) off += sh->wc[k];
        total += sh->wc[k];
    }
    if (place(total)) {
        for (int c0 = lo; c0 < hi; c0 += 64) {
            const int c = c0 + lane;
            const bool keep = c < hi && pred(c);
            const unsigned long long m = __ballot(keep);
            if (c < hi) put(c, keep, off + rank_in(m));
            off += __popcll(m);
        }
    }
    __syncthreads();
    return total;
}

// min / max box of a segment of ord, and its centre (obstacleClustering.cpp:96-124, :192-218)
__device__ inline void node_centre(const View &v, int beg, int end, double *cen) {
    double lo[3] = {kInf, kInf, kInf}, hi[3] = {-kInf, -kInf, -kInf};
    for (int j = beg + lane_id(); j < end; j += 64) {
        double p[3];
        v.point(v.ord[j], p);
        for (int k = 0; k < 3; k++) lo[k] = fmin(lo[k], p[k]), hi[k] = fmax(hi[k], p[k]);
    }
    for (int k = 0; k < 3; k++) cen[k] = mid(wave_min(lo[k]), wave_max(hi[k]));
}

// getOrientation (:230-279): the first angle of the largest density; its rotated box
__device__ inline double node_orientation(const View &v, const impc_cluster_params &pr, int beg, int end, const double *cen,
                                          double *blo, double *bhi, int *bi) {
    double best = 0.0;
    *bi = 0;
    for (int k = 0; k < 3; k++) blo[k] = bhi[k] = 0.0;
    double first[3];  // rotClusterMin / Max start from the UNROTATED points[0] (:239-240): it stays in the box
    v.point(v.ord[beg], first);
    for (int i = 0; i < pr.angle_num; i++) {
        const double c = v.angles[kAngleCols * i + 1], s = v.angles[kAngleCols * i + 2];
        double lo[3] = {first[0], first[1], first[2]}, hi[3] = {first[0], first[1], first[2]};
        for (int j = beg + lane_id(); j < end; j += 64) {
            double p[3], q[3];
            v.point(v.ord[j], p);
            rotate(c, s, p, cen, q);
            for (int k = 0; k < 3; k++) lo[k] = fmin(lo[k], q[k]), hi[k] = fmax(hi[k], q[k]);
        }
        for (int k = 0; k < 3; k++) lo[k] = wave_min(lo[k]), hi[k] = wave_max(hi[k]);
        const double d = density_of(end - beg, lo, hi, pr.cloud_res);
        if (d > best) {
            best = d, *bi = i;
            for (int k = 0; k < 3; k++) blo[k] = lo[k], bhi[k] = hi[k];
        }
    }
    return best;
}

// the first point of the segment farthest from `from` (strict >, from 0: :143, :162); -1 when none is
__device__ inline int node_farthest(const View &v, int beg, int end, const double *from) {
    double bd = 0.0;
    int bj = 0x7fffffff;
    for (int j = beg + lane_id(); j < end; j += 64) {
        double p[3];
        v.point(v.ord[j], p);
        const double d = seed_dist(p, from);
        if (d > bd) bd = d, bj = j;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o, 64);
        const int oj = __shfl_xor(bj, o, 64);
        if (od > bd || (od == bd && oj < bj)) bd = od, bj = oj;
    }
    return bj == 0x7fffffff ? -1 : bj;
}

// runKmeans (:129-189) on a segment of ord: the final labels go to flg[j] (j the position in ord);
// returns the number of label-0 points, or -1 when a seed does not exist.  The label sums of a round
// are per-lane partial sums reduced over the wavefront, not the reference's index-order sums: the
// centroids may differ from its by rounding, the labels only where two distances are that close.
__device__ inline int node_kmeans(const View &v, const impc_cluster_params &pr, int beg, int end, const double *cen) {
#pragma clang fp contract(off)
    const int f = node_farthest(v, beg, end, cen);
    if (f < 0) return -1;
    double c0[3], c1[3];
    v.point(v.ord[f], c0);
    const int ff = node_farthest(v, beg, end, c0);
    if (ff < 0) return -1;
    v.point(v.ord[ff], c1);
    for (int it = 0; it < pr.kmeans_iters; it++) {
        double s0[3] = {0, 0, 0}, s1[3] = {0, 0, 0};
        int n0 = 0, n1 = 0;
        for (int j = beg + lane_id(); j < end; j += 64) {
            double p[3], d[2];
            v.point(v.ord[j], p);
            if (classify2(p, c0, c1, d)) {
                for (int k = 0; k < 3; k++) s1[k] += p[k];
                n1++;
            } else {
                for (int k = 0; k < 3; k++) s0[k] += p[k];
                n0++;
            }
        }
        n0 = wave_sum(n0), n1 = wave_sum(n1);
        for (int k = 0; k < 3; k++) {
            s0[k] = wave_sum(s0[k]), s1[k] = wave_sum(s1[k]);
            if (n0) s0[k] /= n0;
            if (n1) s1[k] /= n1;
            c0[k] = s0[k], c1[k] = s1[k];
        }
    }
    int n0 = 0;
    for (int j = beg + lane_id(); j < end; j += 64) {
        double p[3], d[2];
        v.point(v.ord[j], p);
        const int l = classify2(p, c0, c1, d);
        v.flg[j] = (uint8_t)l;
        n0 += !l;
    }
    return wave_sum(n0);
}

// stable partition of ord[beg, end) by flg: label 0 first (children keep the parent's order, :185-189)
__device__ inline void node_partition(const View &v, int beg, int end, int n0) {
    int *tmp = v.lab;  // free since phase 5
    int off0 = beg, off1 = beg + n0;
    for (int j0 = beg; j0 < end; j0 += 64) {
        const int j = j0 + lane_id();
        const bool in = j < end;
        const int l = in ? v.flg[j] : 0;
        const unsigned long long m1 = __ballot(in && l), m0 = __ballot(in && !l);
        if (in) tmp[l ? off1 + rank_in(m1) : off0 + rank_in(m0)] = v.ord[j];
        off0 += __popcll(m0), off1 += __popcll(m1);
    }
    wave_sync();
    for (int j = beg + lane_id(); j < end; j += 64) v.ord[j] = tmp[j];
    wave_sync();
}

__global__ __launch_bounds__(kThreads) void k_cluster(Args a) {
    extern __shared__ double smem[];
    char *base = (char *)smem;
    const Layout &lay = a.lay;
    const impc_cluster_params &pr = a.pr;
    double *tx = (double *)(base + lay.tab()), *ty = tx + lay.capx, *tz = ty + lay.capy;
    Shared *sh = (Shared *)(base + lay.shared());
    int *ints = (int *)(base + lay.ints());
    const int P = lay.P, S = lay.S;
    View v;
    v.tx = tx, v.ty = ty, v.tz = tz, v.sh = sh;
    v.pts = ints, v.lab = ints + P, v.ord = ints + 2 * P;
    v.nbeg = ints + 3 * P, v.nend = v.nbeg + 2 * S, v.nfin = v.nend + 2 * S, v.nsplit = v.nfin + 2 * S,
    v.ncnt = v.nsplit + S;
    v.flg = (uint8_t *)(base + lay.bytes_at());
    v.cellmap = a.cellmap + (int64_t)blockIdx.x * a.cells;
    v.angles = a.angles, v.P = P, v.S = S, v.r2max = a.r2max;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;

    for (int64_t inst = blockIdx.x; inst < a.I; inst += gridDim.x) {
        __syncthreads();  // the previous instance's reads of LDS are done
        if (a.in.active && !a.in.active[inst]) continue;

        // ---- 1: heading, region, axis tables
        if (tid == 0) {
            region_of(pr, a.in.cur_pos + 3 * inst, a.in.cur_vel + 3 * inst, a.in.first && a.in.first[inst],
                      a.out.heading[inst], sh->r);
            a.out.heading[inst] = sh->r.heading;
            sh->nx = axis_table(sh->r.x0, sh->r.x1, pr.cloud_res, lay.capx, tx);
            sh->ny = axis_table(sh->r.y0, sh->r.y1, pr.cloud_res, lay.capy, ty);
            sh->nz = axis_table(pr.ground_height, pr.ceiling_height, pr.cloud_res, lay.capz, tz);
            sh->flags = 0, sh->cur = 0, sh->nn = 0;
        }
        __syncthreads();
        const int nx = sh->nx, ny = sh->ny, nz = sh->nz;
        if (nx > lay.capx || ny > lay.capy || nz > lay.capz) {  // uniform
            if (tid == 0) {
                a.out.flags[inst] = IMPC_CLUSTER_POINTS;
                if (a.out.num_points) a.out.num_points[inst] = -1;
            }
            continue;
        }

        // ---- 2: lattice scan
        const int L = nx * ny * nz;
        const Region &rg = sh->r;
        const auto cell = [&](int c, int &ix, int &iy, int &iz) {
            iz = c % nz;
            const int t = c / nz;
            iy = t % ny, ix = t / ny;
        };
        const int n = block_compact(
            sh, L,
            [&](int c) {
                int ix, iy, iz;
                cell(c, ix, iy, iz);
                return in_cloud(rg, a.in.map, a.in.map_max, a.in.occ_inflated, tx[ix], ty[iy], tz[iz]);
            },
            [&](int total) { return total > 0 && total <= P; },
            [&](int c, bool keep, int idx) {
                v.cellmap[c] = keep ? idx : -1;
                if (keep) {
                    int ix, iy, iz;
                    cell(c, ix, iy, iz);
                    v.pts[idx] = ix << 20 | iy << 10 | iz;
                }
            });
        if (tid == 0) {
            if (a.out.num_points) a.out.num_points[inst] = n;
            if (n == 0 || n > P) a.out.flags[inst] = n > P ? IMPC_CLUSTER_POINTS : 0;
        }
        if (n == 0 || n > P) continue;  // an empty cloud: run() does nothing (obstacleClustering.cpp:15)
        if (a.out.cloud)
            for (int p = tid; p < n; p += kThreads) {
                double q[3];
                v.point(p, q);
                double *dst = a.out.cloud + (inst * P + p) * 3;
                dst[0] = q[0], dst[1] = q[1], dst[2] = q[2];
            }

        // ---- 3: core points (DBSCAN.h:87-101): at least min_pts OTHER points within eps
        for (int p = tid; p < n; p += kThreads) {
            double pc[3];
            v.point(p, pc);
            int cnt = 0;
            for_neighbours(v, pr, p, [&](int, const double *qc) { cnt += dbscan_dist(pc, qc) <= pr.eps; });
            const bool core = cnt >= pr.min_pts;
            v.flg[p] = core;
            v.lab[p] = core ? p : -1;
        }
        __syncthreads();

        // ---- 4: components of the core points.  Every label is the index of a core point of the
        // same component and only ever decreases; after k sweeps a label is at most the smallest
        // index within k hops, so n sweeps reach the fixed point (all labels of a component equal
        // to its smallest core index) and the loop below ends at the first sweep without a change.
        {
            volatile int *lab = v.lab;
            for (int it = 0; it < n; it++) {
                if (tid == 0) sh->changed = 0;
                __syncthreads();
                bool ch = false;
                for (int p = tid; p < n; p += kThreads) {
                    if (!v.flg[p]) continue;
                    double pc[3];
                    v.point(p, pc);
                    int m = lab[p];
                    const int was = m;
                    for_neighbours(v, pr, p, [&](int q, const double *qc) {
                        if (v.flg[q] && dbscan_dist(pc, qc) <= pr.eps) m = min(m, lab[q]);
                    });
                    if (m < was) lab[p] = m, ch = true;
                }
                if (ch) sh->changed = 1;
                __syncthreads();
                for (int p = tid; p < n; p += kThreads) {  // pointer jumping: labels strictly descend
                    if (!v.flg[p]) continue;
                    int l = lab[p];
                    for (int ll = lab[l]; ll < l; ll = lab[l]) l = ll;
                    lab[p] = l;
                }
                const int changed = sh->changed;
                __syncthreads();
                if (!changed) break;
            }
        }

        // ---- 5: border rule: the adjacent cluster with the smallest start below the point's own index
        for (int p = tid; p < n; p += kThreads) {
            if (v.flg[p]) continue;
            double pc[3];
            v.point(p, pc);
            int best = 0x7fffffff;
            for_neighbours(v, pr, p, [&](int q, const double *qc) {
                if (v.flg[q] && dbscan_dist(pc, qc) <= pr.eps) {
                    const int s = v.lab[q];
                    if (s < p && s < best) best = s;
                }
            });
            v.lab[p] = best == 0x7fffffff ? -1 : best;
        }
        __syncthreads();
        // cluster ranks: ascending start index; ord[start] holds the rank for the moment
        const int nn = block_compact(
            sh, n, [&](int p) { return v.flg[p] && v.lab[p] == p; }, [&](int) { return true; },
            [&](int p, bool keep, int idx) {
                if (keep) v.ord[p] = idx;
            });
        for (int p = tid; p < n; p += kThreads) {
            const int s = v.lab[p];
            const int cl = s >= 0 ? v.ord[s] : IMPC_CLUSTER_NOISE;
            v.lab[p] = cl;  // (only the owner reads lab[p]; starts are read through ord)
            if (a.out.dbscan_label) a.out.dbscan_label[inst * P + p] = cl;
        }
        if (tid == 0 && a.out.num_initial) a.out.num_initial[inst] = nn;
        if (nn > S) {
            if (tid == 0) a.out.flags[inst] = IMPC_CLUSTER_BOXES;
            continue;
        }
        for (int k = tid; k < S; k += kThreads) v.ncnt[k] = 0;
        __syncthreads();
        for (int p = tid; p < n; p += kThreads)
            if (v.lab[p] >= 0) atomicAdd(&v.ncnt[v.lab[p]], 1);
        __syncthreads();
        if (tid == 0) {
            int off = 0;
            for (int k = 0; k < nn; k++) {
                v.nbeg[k] = off, off += v.ncnt[k], v.nend[k] = off, v.nfin[k] = 0;
            }
            sh->nn = nn;
        }
        __syncthreads();
        for (int k = w; k < nn; k += kWaves) {  // members in ascending index order
            int off = v.nbeg[k];
            for (int p0 = 0; p0 < n; p0 += 64) {
                const int p = p0 + lane;
                const bool mine = p < n && v.lab[p] == k;
                const unsigned long long m = __ballot(mine);
                if (mine) v.ord[off + rank_in(m)] = p;
                off += __popcll(m);
            }
        }
        __syncthreads();

        // ---- 6: the refinement tree (obstacleClustering.cpp:20-69)
        for (int level = 0; level < pr.tree_level; level++) {
            const int cur = sh->cur, cn = sh->nn;
            const int *nb = v.nbeg + cur * S, *ne = v.nend + cur * S, *nf = v.nfin + cur * S;
            for (int k = w; k < cn; k += kWaves) {
                int split = -1;  // kept (and complete from now on)
                if (!nf[k]) {
                    const int beg = nb[k], end = ne[k];
                    double cen[3], blo[3], bhi[3];
                    int bi;
                    node_centre(v, beg, end, cen);
                    if (!(node_orientation(v, pr, beg, end, cen, blo, bhi, &bi) >= pr.density_thresh)) {
                        split = node_kmeans(v, pr, beg, end, cen);
                        if (split <= 0 || split >= end - beg) {
                            if (lane == 0) atomicOr(&sh->flags, IMPC_CLUSTER_EMPTY);
                            split = -1;
                        } else {
                            node_partition(v, beg, end, split);
                        }
                    }
                }
                if (lane == 0) v.nsplit[k] = split;
            }
            __syncthreads();
            if (tid == 0 && !sh->flags) {
                int *qb = v.nbeg + (cur ^ 1) * S, *qe = v.nend + (cur ^ 1) * S, *qf = v.nfin + (cur ^ 1) * S;
                int m = 0;
                for (int k = 0; k < cn; k++) {
                    const int parts = v.nsplit[k] < 0 ? 1 : 2;
                    if (m + parts > S) {
                        sh->flags = IMPC_CLUSTER_BOXES;
                        break;
                    }
                    if (parts == 1) {
                        qb[m] = nb[k], qe[m] = ne[k], qf[m] = 1, m++;
                    } else {
                        qb[m] = nb[k], qe[m] = nb[k] + v.nsplit[k], qf[m] = 0, m++;
                        qb[m] = nb[k] + v.nsplit[k], qe[m] = ne[k], qf[m] = 0, m++;
                    }
                }
                sh->nn = m, sh->cur = cur ^ 1;
            }
            __syncthreads();
            if (sh->flags) break;
        }

        // ---- 7: the boxes of the leaves, in sequence order (:71-78, :305-315)
        const int flags = sh->flags;
        if (tid == 0) a.out.flags[inst] = flags;
        if (flags) continue;
        const int cur = sh->cur, cn = sh->nn;
        if (tid == 0) a.out.count[inst] = cn;
        for (int k = w; k < cn; k += kWaves) {
            const int beg = v.nbeg[cur * S + k], end = v.nend[cur * S + k];
            double cen[3], blo[3], bhi[3], oc[3], os[3], oy;
            int bi;
            node_centre(v, beg, end, cen);
            node_orientation(v, pr, beg, end, cen, blo, bhi, &bi);
            box_of(blo, bhi, v.angles[kAngleCols * bi], oc, os, &oy);
            if (lane == 0) {
                const int64_t b = inst * S + k;
                for (int c = 0; c < 3; c++) a.out.centroid[3 * b + c] = oc[c], a.out.size[3 * b + c] = os[c];
                a.out.yaw[b] = oy;
            }
        }
    }
}

}  // namespace impc_clu

struct impc_cluster_s {
    impc_ctx ctx;
    impc_cluster_params pr;
    impc_clu::Layout lay;
    int64_t I, cells;
    int grid, r2max;
    int32_t *cellmap;
    double *angles;
    hipEvent_t last;  // the object's previous launch: the workspace has one user at a time
};

using namespace impc_clu;

static int fail(const std::string &msg) { return impc_lib::set_error(IMPC_INVALID_ARGUMENT, msg); }

extern "C" void impc_cluster_default_params(impc_cluster_params *p) {
    if (!p) return;
    *p = impc_cluster_params{0.2, 5.0, 2.0, 0.3, 2.0, 2.0, 0.3, 0.5, 0.9, 15, 3, 20, 10, 4096, 16};
}

extern "C" int impc_cluster_create(impc_ctx ctx, const impc_cluster_params *p, int64_t instances, impc_cluster *out) {
    if (!ctx || !p || !out) return fail("impc_cluster_create: null argument");
    if (instances < 1) return fail("impc_cluster_create: instances < 1");
    if (!(p->cloud_res > 0) || !(p->eps > 0) || !(p->region_x >= 0) || !(p->region_y >= 0) || !(p->offset >= 0) ||
        !(p->density_thresh > 0) || !(p->min_speed == p->min_speed) ||
        !(p->ceiling_height - p->ground_height < 1e300) || p->min_pts < 0 || p->tree_level < 0 || p->angle_num < 1 ||
        p->angle_num > 64 || p->kmeans_iters < 0 || p->max_points < 1 || p->max_boxes < 1 || p->max_points > (1 << 20) ||
        p->max_boxes > 4096)
        return fail("impc_cluster_create: parameter out of range");
    const double reach = p->region_x + p->offset;
    const double diag = sqrt(reach * reach + 4 * p->region_y * p->region_y) / p->cloud_res;
    if (!(diag < kAxisMax - 4) || !(p->eps / p->cloud_res < 64))
        return fail("impc_cluster_create: the region has more than 1023 lattice cells per axis");
    std::vector<double> tz(kAxisMax);
    const int nz = axis_table(p->ground_height, p->ceiling_height, p->cloud_res, kAxisMax, tz.data());
    if (nz > kAxisMax) return fail("impc_cluster_create: more than 1023 lattice layers between ground and ceiling");
    Layout lay;
    lay.capx = lay.capy = (int)ceil(diag) + 4;
    lay.capz = nz > 0 ? nz : 1;
    lay.P = p->max_points, lay.S = p->max_boxes;
    const int64_t cells = (int64_t)lay.capx * lay.capy * lay.capz;
    if (cells > (1 << 26)) return fail("impc_cluster_create: the region's lattice has more than 2^26 cells");

    HIP_OK(hipSetDevice(impc_lib::device(ctx)));
    int lds_max = 0;
    HIP_OK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, impc_lib::device(ctx)));
    if (lay.total() > (size_t)lds_max)
        return fail("impc_cluster_create: max_points " + std::to_string(lay.P) + " and max_boxes " + std::to_string(lay.S) +
                    " need " + std::to_string(lay.total()) + " bytes of shared memory per workgroup, the device has " +
                    std::to_string(lds_max));
    HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_cluster), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lay.total()));
    impc_cluster_s *c = new impc_cluster_s{};
    c->ctx = ctx, c->pr = *p, c->lay = lay, c->I = instances, c->cells = cells;
    const int rad = stencil_radius(p->cloud_res, p->eps);
    while (c->r2max < 3 * rad * rad && !stencil_far(c->r2max + 1, p->cloud_res, p->eps)) c->r2max++;
    c->grid = (int)std::min<int64_t>(instances, 4 * (int64_t)std::max(impc_lib::num_cu(ctx), 1));
    std::vector<double> tab((size_t)kAngleCols * p->angle_num);
    angle_table(p->angle_num, tab.data());
    hipError_t e = hipMalloc(&c->cellmap, sizeof(int32_t) * (size_t)cells * c->grid);
    if (e == hipSuccess) e = hipMalloc(&c->angles, sizeof(double) * tab.size());
    if (e == hipSuccess) e = hipMemcpy(c->angles, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->last, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)hipFree(c->cellmap), (void)hipFree(c->angles);
        delete c;
        return impc_lib::set_error(IMPC_DEVICE_ERROR, std::string("impc_cluster_create: ") + hipGetErrorString(e));
    }
    *out = c;
    return IMPC_OK;
}

extern "C" int impc_cluster_destroy(impc_cluster c) {
    if (!c) return IMPC_OK;
    (void)hipSetDevice(impc_lib::device(c->ctx));
    (void)hipEventSynchronize(c->last);
    (void)hipEventDestroy(c->last);
    (void)hipFree(c->cellmap), (void)hipFree(c->angles);
    delete c;
    return IMPC_OK;
}

extern "C" int impc_cluster_run_device(impc_cluster c, const impc_cluster_in *in, const impc_cluster_out *out,
                                       void *stream) {
    if (!c || !in || !out) return fail("impc_cluster_run_device: null argument");
    if (!in->cur_pos || !in->cur_vel || !in->occ_inflated || !out->heading || !out->count || !out->centroid ||
        !out->size || !out->yaw || !out->flags)
        return fail("impc_cluster_run_device: a required array is null");
    if (!(in->map.resolution > 0) || in->map.dims[0] < 1 || in->map.dims[1] < 1 || in->map.dims[2] < 1)
        return fail("impc_cluster_run_device: the map needs a positive resolution and positive dimensions");
    HIP_OK(hipSetDevice(impc_lib::device(c->ctx)));
    hipStream_t st = stream ? (hipStream_t)stream : impc_lib::stream(c->ctx);
    HIP_OK(hipStreamWaitEvent(st, c->last, 0));
    Args a;
    a.pr = c->pr, a.in = *in, a.out = *out, a.lay = c->lay, a.I = c->I, a.cells = c->cells;
    a.cellmap = c->cellmap, a.angles = c->angles, a.r2max = c->r2max;
    hipLaunchKernelGGL(k_cluster, dim3(c->grid), dim3(kThreads), c->lay.total(), st, a);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(c->last, st));
    return IMPC_OK;
}

extern "C" int impc_cluster_run(impc_cluster c, const impc_cluster_in *in, const impc_cluster_out *out) {
    if (!c || !in || !out) return fail("impc_cluster_run: null argument");
    if (!in->cur_pos || !in->cur_vel || !in->occ_inflated || !out->heading || !out->count || !out->centroid ||
        !out->size || !out->yaw || !out->flags)
        return fail("impc_cluster_run: a required array is null");
    if (!(in->map.resolution > 0) || in->map.dims[0] < 1 || in->map.dims[1] < 1 || in->map.dims[2] < 1)
        return fail("impc_cluster_run: the map needs a positive resolution and positive dimensions");
    HIP_OK(hipSetDevice(impc_lib::device(c->ctx)));
    hipStream_t st = impc_lib::stream(c->ctx);
    const size_t I = (size_t)c->I, P = (size_t)c->pr.max_points, S = (size_t)c->pr.max_boxes;
    struct Buf {
        void *dev;
        void *host;
        size_t bytes;
        bool back;
    };
    std::vector<Buf> bufs;
    hipError_t err = hipSuccess;
    const auto stage = [&](const void *host, size_t bytes, bool back) -> void * {
        if (!host || err != hipSuccess) return nullptr;
        void *d = nullptr;
        err = hipMalloc(&d, bytes ? bytes : 8);
        if (err != hipSuccess) return nullptr;
        bufs.push_back(Buf{d, const_cast<void *>(host), bytes, back});
        err = hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, st);
        return d;
    };
    impc_cluster_in di = *in;
    impc_cluster_out dout = *out;
    di.active = (const int8_t *)stage(in->active, I, false);
    di.first = (const int8_t *)stage(in->first, I, false);
    di.cur_pos = (const double *)stage(in->cur_pos, 24 * I, false);
    di.cur_vel = (const double *)stage(in->cur_vel, 24 * I, false);
    di.occ_inflated = (const uint8_t *)stage(
        in->occ_inflated, (size_t)in->map.dims[0] * (size_t)in->map.dims[1] * (size_t)in->map.dims[2], false);
    dout.heading = (double *)stage(out->heading, 8 * I, true);
    dout.count = (int32_t *)stage(out->count, 4 * I, true);
    dout.centroid = (double *)stage(out->centroid, 24 * I * S, true);
    dout.size = (double *)stage(out->size, 24 * I * S, true);
    dout.yaw = (double *)stage(out->yaw, 8 * I * S, true);
    dout.flags = (int32_t *)stage(out->flags, 4 * I, true);
    dout.num_points = (int32_t *)stage(out->num_points, 4 * I, true);
    dout.num_initial = (int32_t *)stage(out->num_initial, 4 * I, true);
    dout.cloud = (double *)stage(out->cloud, 24 * I * P, true);
    dout.dbscan_label = (int32_t *)stage(out->dbscan_label, 4 * I * P, true);
    int rc = IMPC_OK;
    if (err == hipSuccess) rc = impc_cluster_run_device(c, &di, &dout, st);
    if (err == hipSuccess && rc == IMPC_OK)
        for (const Buf &b : bufs)
            if (b.back && err == hipSuccess) err = hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (err == hipSuccess) err = es;
    for (const Buf &b : bufs) (void)hipFree(b.dev);
    if (rc != IMPC_OK) return rc;
    if (err != hipSuccess)
        return impc_lib::set_error(IMPC_DEVICE_ERROR, std::string("impc_cluster_run: ") + hipGetErrorString(err));
    return IMPC_OK;
}
