// Cycles per step of the structured kernel's 8-dim stage recursion a_{k+1} = t_{k+1} - F_k a_k
// (W = 19 steps, F and t in LDS), in several formulations, on gfx950.  Run with 1 wavefront per
// SIMD (64-lane blocks) and with 2 (512-lane blocks: waves w and w+4 share a SIMD).
//
//   0  lane grid 8x8, alternating strided/contiguous 8-lane sums, update_dpp(old = 0), an LDS
//      store of each stage (the kernel as of round 1)
//   1  as 0 with mov_dpp (bound_ctrl, no old operand)
//   2  as 1, results captured in registers (v_cndmask per step) instead of stored
//   3  as 1 without any store (the bare chain: lower bound of the lane-grid form)
//   4  broadcast form: lane i < 8 holds row i of F_k, a_k in SGPRs (v_readlane), products and a
//      depth-3 add tree in the lane (same rounding as the lane-grid sums); store per step
//   5  as 4 without the store
//   6  as 1, recursion fully unrolled up to the maximum W (runtime W, break past it): exact
//      waitcnts, exec-masked store of each stage
//   7  as 6, stages captured in registers with compile-time lane masks, stored after the sweep
//   8  row-broadcast form: lane l holds row (l & 7) of F_k (8 copies per wave), a_k lane i;
//      the 8 operands by v_mov_b64_dpp row_newbcast, 4 mul + 4 fma + depth-2 adds in the lane;
//      fully unrolled, captured in registers (copy l >> 3 keeps step m when m % 8 == l >> 3)
//   9  as 8 with an LDS store of each stage by lanes 0..7 (runtime loop)
//  10  as 1 with two independent chains interleaved in one instruction stream
//
// The four-block FP64 matrix instruction v_mfma_f64_4x4x4_4b_f64 (one f64 per lane for A, B and C/D),
// printed after the table above in the same run:
//   - its operand layout, found by feeding unit inputs (k_layout).  On gfx950, with lane = x + 4 b + 16 q
//     and b the block: A[i][k] sits in lane i + 4 b + 16 k, B[k][j] in lane j + 4 b + 16 k, C[i][j] and
//     D[i][j] in lane j + 4 b + 16 i; an element's four products are added to C in k-ascending fma order
//     (the sweeps below match that chain bit for bit);
//   - issue-to-issue cycles of dependent chains of it (k_lat);
//   - both W-step sweeps, capture and stores included, on host-made random F, t (km):
//      11 / 12  the lane grid as the kernel runs it (fma(-f, v, c / 8), constant-mask capture), forward /
//               backward
//      13 / 14  the step as one instruction: block (r, c) takes -F's 4x4 block, B = v[4 c + k] in all four
//               columns, C = c[4 r + i] / 2 in both blocks of a row, v'[4 r + i] = D(r, 0) + D(r, 1) by one
//               row DPP move + add; the block numbering alternates between even and odd steps (see the
//               mf_* maps) so that the sum lands where the next step's B wants it
//      15 / 16  as 13 / 14 with the capture select written in C++ (inverse ballot of the constant mask)
//      17 .. 30 the 4x4x4 step with its off-chain instructions moved (km's FORM 1 .. 7, forward / backward
//               each); every form loads (F, c) only for steps that exist:
//                 1  the capture selects of step m issued behind the MFMA of step m + 1, inside its wait
//                    states: each select names the MFMA's result as a read-write operand it does not touch,
//                    so it can stand neither in front of the MFMA nor behind the DPP moves, and the hazard
//                    recognizer still counts the MFMA -> DPP wait states (selects included)
//                 2  as 1 with (F, c) loaded three steps ahead
//                 3  no capture: step m's v stored by all 64 lanes (the 8 holders of an element write the
//                    same value to the same address) behind the MFMA of step m + 1; loads three ahead (as
//                    compiled, the 19 results stay in 38 VGPRs and the stores follow the last step)
//                 4  as 2 with the 16 capture masks in SGPRs from before the first sweep
//                 5  as 2 with the select written in C++ (inverse ballot) between two empty asm statements
//                    that name the MFMA's result: the selects are instructions the hazard recognizer counts
//                 6  the capture behind the step's own add as in 13 / 14, but as one instruction: v_mov_b64 under
//                    the keep mask in EXEC (s_mov_b64 exec around it in one asm statement; the sweeping wave
//                    has all 64 lanes active, and an SALU write of EXEC needs no wait state before a VALU
//                    instruction); loads two ahead
//                 7  as 6 with loads three ahead
//                 8  no capture registers, keep masks or stores after the sweep: every step's v', times the
//                    scale-back factor (an opaque 1.0 here), stored by all 64 lanes behind the step's own add,
//                    where the select pair sits in 13 / 14 (the 8 holders of an element write the same value);
//                    a compiler memory fence behind each store keeps them one per step; loads two ahead
//     and their difference from a long-double evaluation next to the lane grid's.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>

constexpr int W = 19, REP = 32;

template <int CTRL, bool BC>
__device__ double dpp(double v) {
    int lo, hi;
    if (BC) {
        lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true);
        hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true);
    } else {
        lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
        hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    }
    return __hiloint2double(hi, lo);
}
template <bool P32>
__device__ double pair_sum(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    if (P32) {
        auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        return __hiloint2double(rh[0], rl[0]) + __hiloint2double(rh[1], rl[1]);
    }
    auto rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return __hiloint2double(rh[0], rl[0]) + __hiloint2double(rh[1], rl[1]);
}
template <bool BC>
__device__ double contig(double v) {
    v = v + dpp<0xB1, BC>(v);
    v = v + dpp<0x4E, BC>(v);
    return v + dpp<0x141, BC>(v);
}
template <bool BC>
__device__ double strided(double v) {
    v = v + dpp<0x128, BC>(v);
    v = pair_sum<false>(v);
    return pair_sum<true>(v);
}
template <int N>
__device__ double nbc(double v) { return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + N, 0xF, 0xF, false); }
__device__ double rowdot(const double (&f)[8], double a) {
    const double s0 = fma(f[1], nbc<1>(a), f[0] * nbc<0>(a)), s1 = fma(f[3], nbc<3>(a), f[2] * nbc<2>(a));
    const double s2 = fma(f[5], nbc<5>(a), f[4] * nbc<4>(a)), s3 = fma(f[7], nbc<7>(a), f[6] * nbc<6>(a));
    return (s0 + s1) + (s2 + s3);
}
__device__ double prod_nc(double a, double b) {
    double p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}
__device__ double bcast(double v, int src) {
    int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

template <int MODE>
__global__ void kr(double *o, unsigned long long *cyc, int Wr) {
    __shared__ double F[8][64 * (W + 3)];
    __shared__ double t[8][13 * (W + 4)], out[8][13 * (W + 4)], junk[8][64];
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, i = l >> 3, j = l & 7;
    for (int p = l; p < 64 * (W + 3); p += 64) F[wv][p] = 0.01 * ((p * 37) % 17) - 0.08;
    for (int p = l; p < 13 * (W + 4); p += 64) t[wv][p] = 0.1 * ((p * 11) % 7) - 0.3;
    __syncthreads();
    const double *Fm = F[wv], *tb = t[wv];
    double *rb = out[wv], *jk = junk[wv] + l;
    double acc = 0.0;
    unsigned long long c0 = 0;
    for (int rep = -1; rep < REP; rep++) {
        if (rep == 0) c0 = __builtin_amdgcn_s_memtime();
        if (MODE == 10) {
            // two independent chains (different starts) interleaved in one instruction stream:
            // is a step issue-bound or latency-bound at this occupancy?
            double a = tb[i], b = tb[26 + i];
            double fe = Fm[l], te = tb[13 + j], fo = Fm[64 + l], to = tb[26 + i];
            for (int k = 0; k < W; k += 2) {
                const double f0 = fe, t0 = te;
                fe = Fm[64 * (k + 2) + l];
                te = tb[13 * (k + 3) + j];
                a = t0 - strided<true>(prod_nc(f0, a));
                b = 0.5 * t0 - strided<true>(prod_nc(f0, b));
                if (k + 1 >= W) break;
                const double f1 = fo, t1 = to;
                fo = Fm[64 * (k + 3) + l];
                to = tb[13 * (k + 4) + i];
                a = t1 - contig<true>(prod_nc(f1, a));
                b = 0.5 * t1 - contig<true>(prod_nc(f1, b));
            }
            acc += a + b;
        } else if (MODE >= 8) {
            const int r = l & 7, cp = l >> 3;
            double a = tb[r], f[8], fn[8], tn = tb[13 + r];
            double cap[3] = {0, 0, 0};
            _Pragma("unroll") for (int q = 0; q < 8; q++) f[q] = Fm[8 * r + q];
            if (MODE == 8) {
                _Pragma("unroll") for (int k = 0; k < W; k++) {
                    _Pragma("unroll") for (int q = 0; q < 8; q++) fn[q] = Fm[64 * (k + 1) + 8 * r + q];
                    const double tc = tn;
                    tn = tb[13 * (k + 2) + r];
                    a = tc - rowdot(f, a);
                    if ((k & 7) == cp) cap[k >> 3] = a;
                    _Pragma("unroll") for (int q = 0; q < 8; q++) f[q] = fn[q];
                }
                _Pragma("unroll") for (int qq = 0; qq < 3; qq++) {
                    const int k = 8 * qq + cp;
                    if (k < W) rb[13 * (k + 1) + r] = cap[qq];
                }
            } else {
                for (int k = 0; k < Wr; k++) {
                    _Pragma("unroll") for (int q = 0; q < 8; q++) fn[q] = Fm[64 * (k + 1) + 8 * r + q];
                    const double tc = tn;
                    tn = tb[13 * (k + 2) + r];
                    a = tc - rowdot(f, a);
                    *(l < 8 ? rb + 13 * (k + 1) + r : jk) = a;
                    _Pragma("unroll") for (int q = 0; q < 8; q++) f[q] = fn[q];
                }
            }
            acc += a;
        } else if (MODE <= 3) {
            constexpr bool BC = MODE >= 1;
            double co0 = 0, co1 = 0, ce0 = 0, ce1 = 0;
            double a = tb[i];
            double fe = Fm[l], te = tb[13 + j], fo = Fm[64 + l], to = tb[26 + i];
            for (int k = 0; k < W; k += 2) {
                const double f0 = fe, t0 = te;
                fe = Fm[64 * (k + 2) + l];
                te = tb[13 * (k + 3) + j];
                a = t0 - strided<BC>(prod_nc(f0, a));
                if (MODE <= 1) *(i == 0 ? rb + 13 * (k + 1) + j : jk) = a;
                if (MODE == 2) {
                    const bool h = (((k + 1) >> 1) & 7) == i;
                    co0 = (h && (k + 1) < 16) ? a : co0;
                    co1 = (h && (k + 1) >= 16) ? a : co1;
                }
                if (k + 1 >= W) break;
                const double f1 = fo, t1 = to;
                fo = Fm[64 * (k + 3) + l];
                to = tb[13 * (k + 4) + i];
                a = t1 - contig<BC>(prod_nc(f1, a));
                if (MODE <= 1) *(j == 0 ? rb + 13 * (k + 2) + i : jk) = a;
                if (MODE == 2) {
                    const bool h = (((k + 2) >> 1) & 7) == j;
                    ce0 = (h && (k + 2) < 16) ? a : ce0;
                    ce1 = (h && (k + 2) >= 16) ? a : ce1;
                }
            }
            acc += a + co0 + co1 + ce0 + ce1;
        } else if (MODE >= 6) {
            double co[2] = {0, 0}, ce[2] = {0, 0};
            double a = tb[i];
            double fe = Fm[l], te = tb[13 + j], fo = Fm[64 + l], to = tb[26 + i];
            _Pragma("unroll") for (int k = 0; k < W; k += 2) {
                if (k >= Wr) continue;
                const double f0 = fe, t0 = te;
                fe = Fm[64 * (k + 2) + l];
                te = tb[13 * (k + 3) + j];
                a = t0 - strided<true>(prod_nc(f0, a));
                if (MODE == 6) {
                    if (i == 0) rb[13 * (k + 1) + j] = a;
                } else if ((((k + 1) >> 1) & 7) == i) {
                    co[(k + 1) >> 4] = a;
                }
                if (k + 1 >= Wr) continue;
                const double f1 = fo, t1 = to;
                fo = Fm[64 * (k + 3) + l];
                to = tb[13 * (k + 4) + i];
                a = t1 - contig<true>(prod_nc(f1, a));
                if (MODE == 6) {
                    if (j == 0) rb[13 * (k + 2) + i] = a;
                } else if ((((k + 2) >> 1) & 7) == j) {
                    ce[(k + 2) >> 4] = a;
                }
            }
            if (MODE == 7) {
                _Pragma("unroll") for (int qq = 0; qq < 2; qq++) {
                    const int so = 2 * (8 * qq + i) + 1, se = 2 * (8 * qq + j);
                    if (so <= Wr) rb[13 * so + j] = co[qq];
                    if (se >= 1 && se <= Wr) rb[13 * se + i] = ce[qq];
                }
            }
            acc += a;
        } else {
            // broadcast form: lane r = l & 7 holds row r of F_k (row-major layout in this probe)
            const int r = l & 7;
            double av[8];
            _Pragma("unroll") for (int q = 0; q < 8; q++) av[q] = tb[q];
            double f[8], tn = tb[13 + r];
            _Pragma("unroll") for (int q = 0; q < 8; q++) f[q] = Fm[8 * r + q];
            for (int k = 0; k < W; k++) {
                double fc[8];
                _Pragma("unroll") for (int q = 0; q < 8; q++) fc[q] = f[q];
                const double tc = tn;
                _Pragma("unroll") for (int q = 0; q < 8; q++) f[q] = Fm[64 * (k + 1) + 8 * r + q];
                tn = tb[13 * (k + 2) + r];
                double p[8];
                _Pragma("unroll") for (int q = 0; q < 8; q++) p[q] = prod_nc(fc[q], av[q]);
                const double s = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
                const double res = tc - s;
                if (MODE == 4) *(l < 8 ? rb + 13 * (k + 1) + r : jk) = res;
                _Pragma("unroll") for (int q = 0; q < 8; q++) av[q] = bcast(res, q);
            }
            acc += av[0];
        }
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    o[threadIdx.x] = acc + rb[l];
    if (threadIdx.x == 0) cyc[MODE] = (c1 - c0) / (REP * W);
}

// ---- modes 11..14: the four-block v_mfma_f64_4x4x4_4b_f64 -------------------------------------
typedef unsigned long long u64;
__device__ double mfma4(double a, double b, double c) { return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0); }

// Operand layout: A = 1 in lane la only, B = 1 in lane lb only, C = 0; msk[64 la + lb] = the lanes
// whose D is not zero (same block and same k: row i of A's lane, column j of B's lane).
__global__ void k_layout(u64 *msk) {
    const int l = threadIdx.x;
    for (int la = 0; la < 64; la++)
        for (int lb = 0; lb < 64; lb++) {
            const double d = mfma4(l == la ? 1.0 : 0.0, l == lb ? 1.0 : 0.0, 0.0);
            const u64 m = __ballot(d != 0.0);
            if (l == 0) msk[64 * la + lb] = m;
        }
}

// Issue-to-issue cycles of dependent chains of the instruction (64 in a row, compiler's own waits):
// 0 D -> C, 1 D -> B, 2 D -> v_add_f64 -> B, 3 D -> row DPP pair sum (2 mov_dpp + add) -> B
template <int V>
__global__ void k_lat(double *o, u64 *cyc) {
    const int l = threadIdx.x;
    const double a = 0.001 * l, b = 0.5 + 0.001 * l, c = 0.25;
    u64 c0 = 0;
    double x = b, y = c;
    for (int rep = -1; rep < REP; rep++) {
        if (rep == 0) c0 = __builtin_amdgcn_s_memtime();
        _Pragma("unroll") for (int q = 0; q < 64; q++) {
            if (V == 0) y = mfma4(a, x, y);
            if (V == 1) x = mfma4(a, x, y);
            if (V == 2) x = mfma4(a, x, y) + 1.0;
            if (V == 3) {
                const double d = mfma4(a, x, y);
                x = d + dpp<0x141, true>(d);
            }
        }
        asm volatile("" : "+v"(x), "+v"(y));
    }
    const u64 c1 = __builtin_amdgcn_s_memtime();
    if (l == 0) cyc[V] = (c1 - c0) * 10 / (REP * 64);
    o[l] = x + y;
}

// ---- lane and block maps of the 4x4x4 form (plain integer functions: they also compile for the host)
// Layout found on gfx950 (k_layout): lane = x + 4 b + 16 q with b the block;
//   A[i][k] of block b sits in lane i + 4 b + 16 k, B[k][j] in lane j + 4 b + 16 k, D[i][j] (and C) in
//   lane j + 4 b + 16 i.
// A step v' = c - M v (M 8x8 as 2x2 blocks of 4x4) is one instruction: block b carries M's block
// (r, c'), B = v[4 c' + k] in every column j, C = S c[4 r + i] in every column (S = kMfmaScale = 1/2:
// both blocks of a row r carry half of c, so no lane needs a zero), and v'[4 r + i] = D(r,0) + D(r,1).
// Even steps number the blocks b = 2 r + c': the partner is lane ^ 4 (row_half_mirror, D is the same
// in all four columns) and the sum leaves v'[4 (b >> 1) + q] in lane (x, b, q) -- which is the B
// operand of an odd step, whose blocks are numbered b = r + 2 c' (partner lane ^ 8, row_ror:8),
// leaving v'[4 (b & 1) + q]: the even step's B again.  No transpose on the chain.
constexpr double kMfmaScale = 0.5;
__host__ __device__ constexpr int mf_x(int l) { return l & 3; }
__host__ __device__ constexpr int mf_b(int l) { return (l >> 2) & 3; }
__host__ __device__ constexpr int mf_q(int l) { return l >> 4; }
__host__ __device__ constexpr int mf_r(int l, bool odd) { return odd ? mf_b(l) & 1 : mf_b(l) >> 1; }  // block row
__host__ __device__ constexpr int mf_c(int l, bool odd) { return odd ? mf_b(l) >> 1 : mf_b(l) & 1; }  // block column
// slot (row-major 8 r + c of F_k) that lane l feeds to A: -F_k forward, -F_k' backward
__host__ __device__ constexpr int mf_fslot(int l, bool odd, bool fwd) {
    const int row = 4 * mf_r(l, odd) + mf_x(l), col = 4 * mf_c(l, odd) + mf_q(l);
    return fwd ? 8 * row + col : 8 * col + row;
}
__host__ __device__ constexpr int mf_in(int l, bool odd) { return 4 * mf_c(l, odd) + mf_q(l); }   // element of v in B
__host__ __device__ constexpr int mf_out(int l, bool odd) { return 4 * mf_r(l, odd) + mf_q(l); }  // element of c, v'
// the 8 lanes sharing an output element differ in this index; lane with other == (m / 2) % 8 keeps step m
__host__ __device__ constexpr int mf_other(int l, bool odd) { return mf_x(l) + 4 * mf_c(l, odd); }
__host__ __device__ constexpr u64 mf_mask(int v, bool odd) {
    return odd ? 0x0001000100010001ull * (0x11ull << ((v & 3) + 8 * (v >> 2))) : 0x0101010101010101ull << v;
}

template <bool IB = false>
__device__ void capc(double &d, double r, u64 MSK) {
    if (IB) {  // the same select, visible to the compiler's scheduler and hazard counting
        d = __builtin_amdgcn_inverse_ballot_w64(MSK) ? r : d;
        return;
    }
    int lo = __double2loint(d), hi = __double2hiint(d);
    asm("v_cndmask_b32 %0, %0, %1, %2" : "+v"(lo) : "v"(__double2loint(r)), "s"(MSK));
    asm("v_cndmask_b32 %0, %0, %1, %2" : "+v"(hi) : "v"(__double2hiint(r)), "s"(MSK));
    d = __hiloint2double(hi, lo);
}

// capc's select, ordered behind the producer of `tie` and in front of its readers (tie is not touched)
__device__ void capd(double &d, double r, u64 MSK, double &tie) {
    int lo = __double2loint(d), hi = __double2hiint(d);
    asm("v_cndmask_b32 %0, %0, %2, %3" : "+v"(lo), "+v"(tie) : "v"(__double2loint(r)), "s"(MSK));
    asm("v_cndmask_b32 %0, %0, %2, %3" : "+v"(hi), "+v"(tie) : "v"(__double2hiint(r)), "s"(MSK));
    d = __hiloint2double(hi, lo);
}

// the capture as one 64-bit move under the mask in EXEC (all 64 lanes are active around it)
__device__ void capx(double &d, double r, u64 MSK) {
    asm("s_mov_b64 exec, %2\n\tv_mov_b64 %0, %1\n\ts_mov_b64 exec, -1" : "+v"(d) : "v"(r), "s"(MSK));
}

// Modes 11 / 12: the lane grid as the kernel runs it (fma(-f, v, c / 8), 8-lane sums, constant-mask
// capture, stores after the sweep), forward / backward.  Modes 13 / 14: the 4x4x4 form.  F, t from the
// host (gF row-major F_k, gt stride 13), results of wave 0 to gout for the arithmetic check.
template <int MODE, int FORM = 0>
__global__ void km(const double *gF, const double *gt, double *gout, double *o, u64 *cyc) {
    __shared__ double F[8][64 * (W + 3)];
    __shared__ double t[8][13 * (W + 4)], out[8][13 * (W + 4)];
    constexpr bool MF = MODE >= 13, FWD = (MODE & 1) != 0, IB = MODE >= 15;
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, i = l >> 3, j = l & 7;
    for (int p = l; p < 64 * (W + 3); p += 64) {
        const int k = p >> 6, e = p & 63;
        // lane grid: even k transposed (the kernel's f_el); 4x4x4: -F_k row-major
        F[wv][p] = MF ? -gF[p] : (!(k & 1) ? gF[64 * k + 8 * (e & 7) + (e >> 3)] : gF[p]);
    }
    for (int p = l; p < 13 * (W + 4); p += 64) t[wv][p] = gt[p] * (MF ? kMfmaScale : 0.125), out[wv][p] = 0.0;
    __syncthreads();
    const double *Fm = F[wv], *tb = t[wv];
    double *rb = out[wv];
    double acc = 0.0;
    u64 c0 = 0;
    u64 mk[16];
    if (FORM == 4) {
        _Pragma("unroll") for (int q = 0; q < 16; q++) {
            mk[q] = mf_mask(q & 7, q >> 3);
            asm volatile("" : "+s"(mk[q]));
        }
    }
    double back = 1.0;  // FORM 8: the kernel's scale-back multiply, by a factor the compiler cannot fold
    asm volatile("" : "+v"(back));
    for (int rep = -1; rep < REP; rep++) {
        if (rep == 0) c0 = __builtin_amdgcn_s_memtime();
        double ce[2] = {0, 0}, co[2] = {0, 0};
        if (FORM > 0) {
            constexpr int PD = (FORM == 1 || FORM == 6 || FORM == 8) ? 2 : 3;
            const int fs[2] = {mf_fslot(l, false, FWD), mf_fslot(l, true, FWD)};
            const int os[2] = {mf_out(l, false), mf_out(l, true)};
            double a = (1.0 / kMfmaScale) * tb[(FWD ? 0 : 13 * W) + mf_in(l, false)];
            auto fk = [](int m) { return 64 * (FWD ? m : W - 1 - m); };
            auto tk = [](int m) { return 13 * (FWD ? m + 1 : W - 1 - m); };
            double fq[PD], tq[PD];
            _Pragma("unroll") for (int p = 0; p < PD; p++) fq[p] = Fm[fk(p) + fs[p & 1]], tq[p] = tb[tk(p) + os[p & 1]];
            _Pragma("unroll") for (int m = 0; m < W; m++) {
                const double f0 = fq[m % PD], t0 = tq[m % PD];
                if (m + PD < W) fq[m % PD] = Fm[fk(m + PD) + fs[(m + PD) & 1]], tq[m % PD] = tb[tk(m + PD) + os[(m + PD) & 1]];
                double d = mfma4(f0, a, t0);
                if (FORM == 8) {
                    a = (m & 1) ? d + dpp<0x128, true>(d) : d + dpp<0x141, true>(d);
                    rb[tk(m) + os[m & 1]] = back * a;
                    asm volatile("" ::: "memory");  // the store is issued here, not collected behind the sweep
                    continue;
                }
                if (FORM >= 6) {
                    a = (m & 1) ? d + dpp<0x128, true>(d) : d + dpp<0x141, true>(d);
                    if (m + 1 < W) capx((m & 1) ? co[m >> 4] : ce[m >> 4], a, mf_mask((m >> 1) & 7, m & 1));
                    continue;
                }
                if (m > 0) {  // step m - 1, whose v is still in a
                    const int n = m - 1;
                    if (FORM == 3) {
                        rb[tk(n) + os[n & 1]] = a;
                    } else if (FORM == 5) {
                        double &cd = (n & 1) ? co[n >> 4] : ce[n >> 4];
                        asm("" : "+v"(a), "+v"(d));
                        capc<true>(cd, a, mf_mask((n >> 1) & 7, n & 1));
                        asm("" : "+v"(cd), "+v"(d));
                    } else capd((n & 1) ? co[n >> 4] : ce[n >> 4], a, FORM == 4 ? mk[((n >> 1) & 7) + 8 * (n & 1)] : mf_mask((n >> 1) & 7, n & 1), d);
                }
                a = (m & 1) ? d + dpp<0x128, true>(d) : d + dpp<0x141, true>(d);
                if (FORM == 5) {  // the step's order: MFMA, selects, LDS reads, DPP moves and add
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
                }
            }
            if (FORM == 8) {
            } else if (FORM == 3) {
                rb[tk(W - 1) + os[(W - 1) & 1]] = a;
            } else {
                capc(((W - 1) & 1) ? co[(W - 1) >> 4] : ce[(W - 1) >> 4], a, mf_mask(((W - 1) >> 1) & 7, (W - 1) & 1));
                _Pragma("unroll") for (int q = 0; q < 2; q++) {
                    const int m0 = 16 * q + 2 * mf_other(l, false), m1 = 16 * q + 2 * mf_other(l, true) + 1;
                    if (m0 < W) rb[tk(m0) + os[0]] = ce[q];
                    if (m1 < W) rb[tk(m1) + os[1]] = co[q];
                }
            }
            acc += a;
        } else if (!MF) {
            // even steps m: strided sum when the stage k is even (forward k = m, backward k = W-1-m)
            constexpr bool S0 = FWD ? true : ((W - 1) & 1) == 0 ? false : true;  // bwd: odd k strided
            const int i0 = S0 ? i : j, j0 = S0 ? j : i;                         // even step: in at i0, out at j0
            double a = 8.0 * tb[FWD ? i0 : 13 * W + i0];
            auto fk = [&](int m) { const int k = FWD ? m : W - 1 - m; return 64 * (k > 0 ? k : 0) + l; };
            auto tk = [&](int m) { const int k = FWD ? m + 1 : W - 1 - m; return 13 * (k > 0 ? k : 0); };
            double fe = Fm[fk(0)], te = tb[tk(0) + j0], fo = Fm[fk(1)], to = tb[tk(1) + i0];
            _Pragma("unroll") for (int m = 0; m < W; m += 2) {
                const double f0 = fe, t0 = te;
                fe = Fm[fk(m + 2)];
                te = tb[tk(m + 2) + j0];
                const double p0 = __builtin_fma(-f0, a, t0);
                a = S0 ? strided<true>(p0) : contig<true>(p0);
                const u64 mi = 0xFFull << (8 * ((m >> 1) & 7)), mj = 0x0101010101010101ull << ((m >> 1) & 7);
                capc(ce[m >> 4], a, S0 ? mi : mj);
                if (m + 1 < W) {
                    const double f1 = fo, t1 = to;
                    fo = Fm[fk(m + 3)];
                    to = tb[tk(m + 3) + i0];
                    const double p1 = __builtin_fma(-f1, a, t1);
                    a = S0 ? contig<true>(p1) : strided<true>(p1);
                    capc(co[m >> 4], a, S0 ? mj : mi);
                }
            }
            _Pragma("unroll") for (int q = 0; q < 2; q++) {
                const int m0 = 16 * q + 2 * i0, m1 = 16 * q + 2 * j0 + 1;
                if (m0 < W) rb[13 * (FWD ? m0 + 1 : W - 1 - m0) + j0] = ce[q];
                if (m1 < W) rb[13 * (FWD ? m1 + 1 : W - 1 - m1) + i0] = co[q];
            }
            acc += a;
        } else {
            const int fse = mf_fslot(l, false, FWD), fso = mf_fslot(l, true, FWD);
            const int oe = mf_out(l, false), oo = mf_out(l, true);
            double a = (1.0 / kMfmaScale) * tb[(FWD ? 0 : 13 * W) + mf_in(l, false)];
            auto fk = [&](int m) { const int k = FWD ? m : W - 1 - m; return 64 * (k > 0 ? k : 0); };
            auto tk = [&](int m) { const int k = FWD ? m + 1 : W - 1 - m; return 13 * (k > 0 ? k : 0); };
            double fe = Fm[fk(0) + fse], te = tb[tk(0) + oe], fo = Fm[fk(1) + fso], to = tb[tk(1) + oo];
            _Pragma("unroll") for (int m = 0; m < W; m += 2) {
                const double f0 = fe, t0 = te;
                fe = Fm[fk(m + 2) + fse];
                te = tb[tk(m + 2) + oe];
                const double d0 = mfma4(f0, a, t0);
                a = d0 + dpp<0x141, true>(d0);
                capc<IB>(ce[m >> 4], a, mf_mask((m >> 1) & 7, false));
                if (m + 1 < W) {
                    const double f1 = fo, t1 = to;
                    fo = Fm[fk(m + 3) + fso];
                    to = tb[tk(m + 3) + oo];
                    const double d1 = mfma4(f1, a, t1);
                    a = d1 + dpp<0x128, true>(d1);
                    capc<IB>(co[m >> 4], a, mf_mask((m >> 1) & 7, true));
                }
            }
            _Pragma("unroll") for (int q = 0; q < 2; q++) {
                const int m0 = 16 * q + 2 * mf_other(l, false), m1 = 16 * q + 2 * mf_other(l, true) + 1;
                if (m0 < W) rb[13 * (FWD ? m0 + 1 : W - 1 - m0) + oe] = ce[q];
                if (m1 < W) rb[13 * (FWD ? m1 + 1 : W - 1 - m1) + oo] = co[q];
            }
            acc += a;
        }
    }
    const u64 c1 = __builtin_amdgcn_s_memtime();
    o[threadIdx.x] = acc;
    if (threadIdx.x == 0) cyc[FORM ? 15 + 2 * FORM + !FWD : MODE] = (c1 - c0) * 10 / (REP * W);
    if (wv == 0)
        for (int p = l; p < 13 * (W + 4); p += 64) gout[p] = rb[p];
}

// Host references of both sweeps on (gF, gt): REF 0 long double, REF 1 / 2 the 4x4x4 form's value if the
// instruction runs D = fma(A[i][3], B[3], .. fma(A[i][0], B[0], C)) (k ascending) / k descending per
// block, followed by the pair sum.  Results in the sweeps' layout (stride 13).
template <int REF>
static void host_sweep(const double *gF, const double *gt, bool fwd, long double *res) {
    long double v[8], vn[8];
    for (int r = 0; r < 8; r++) v[r] = gt[(fwd ? 0 : 13 * W) + r];
    for (int m = 0; m < W; m++) {
        const int k = fwd ? m : W - 1 - m, st = fwd ? m + 1 : k;
        for (int r = 0; r < 8; r++) {
            auto fe = [&](int c) { return fwd ? gF[64 * k + 8 * r + c] : gF[64 * k + 8 * c + r]; };
            if (REF == 0) {
                long double s = gt[13 * st + r];
                for (int c = 0; c < 8; c++) s -= (long double)fe(c) * v[c];
                vn[r] = s;
            } else {
                double d[2];
                for (int cb = 0; cb < 2; cb++) {
                    d[cb] = gt[13 * st + r] * kMfmaScale;
                    for (int kk = 0; kk < 4; kk++) {
                        const int c = 4 * cb + (REF == 1 ? kk : 3 - kk);
                        d[cb] = __builtin_fma(-fe(c), (double)v[c], d[cb]);
                    }
                }
                vn[r] = d[0] + d[1];
            }
        }
        for (int r = 0; r < 8; r++) res[13 * st + r] = v[r] = vn[r];
    }
}

static int mfma4_modes(double *o) {
    // operand layout
    u64 *dm, *dc, hm[4096], hc[36] = {};
    if (hipMalloc(&dm, sizeof(hm)) || hipMalloc(&dc, sizeof(hc))) return 1;
    hipLaunchKernelGGL(k_layout, 1, 64, 0, 0, dm);
    if (hipMemcpy(hm, dm, sizeof(hm), hipMemcpyDeviceToHost)) return 1;
    int bad = 0;
    for (int la = 0; la < 64; la++)
        for (int lb = 0; lb < 64; lb++) {
            const bool same = mf_b(la) == mf_b(lb) && mf_q(la) == mf_q(lb);  // same block, same k
            const u64 want = same ? 1ull << (mf_x(lb) + 4 * mf_b(la) + 16 * mf_x(la)) : 0;
            bad += hm[64 * la + lb] != want;
        }
    printf("-- v_mfma_f64_4x4x4_4b_f64 operand layout\n");
    printf("A[i][k] blk b: lane i+4b+16k, B[k][j]: lane j+4b+16k, D[i][j]: lane j+4b+16i -- %s (%d of 4096 differ)\n",
           bad ? "NOT what the hardware does" : "confirmed", bad);
    if (bad)
        for (int la = 0; la < 64; la++) {
            u64 sa = 0, sb = 0, pl = 0;  // D lanes fed by A lane la, by B lane la; B lanes that meet A lane la
            for (int x = 0; x < 64; x++) {
                sa |= hm[64 * la + x], sb |= hm[64 * x + la];
                if (hm[64 * la + x]) pl |= 1ull << x;
            }
            printf("lane %2d: A feeds D %016llx, meets B lanes %016llx; B feeds D %016llx\n", la, sa, pl, sb);
        }
    // dependent-issue latency
    for (int it = 0; it < 2; it++) {
        hipLaunchKernelGGL(k_lat<0>, 1, 64, 0, 0, o, dc);
        hipLaunchKernelGGL(k_lat<1>, 1, 64, 0, 0, o, dc);
        hipLaunchKernelGGL(k_lat<2>, 1, 64, 0, 0, o, dc);
        hipLaunchKernelGGL(k_lat<3>, 1, 64, 0, 0, o, dc);
    }
    if (hipMemcpy(hc, dc, sizeof(hc), hipMemcpyDeviceToHost)) return 1;
    const char *ln[] = {"D -> C", "D -> B", "D -> v_add_f64 -> B", "D -> 2 mov_dpp + add -> B"};
    printf("-- dependent chains of the instruction, cycles per link (1 wavefront)\n");
    for (int v = 0; v < 4; v++) printf("%-28s %5.1f\n", ln[v], hc[v] / 10.0);
    // the sweeps
    constexpr int NF = 64 * (W + 3), NT = 13 * (W + 4);
    constexpr int NM = 22;
    static double gF[NF], gt[NT], ho[NM][NT];
    static long double ref[2][3][NT];
    u64 s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0 - 0.5; };
    for (double &f : gF) f = 0.24 * rnd();
    for (double &t : gt) t = rnd();
    double *dF, *dt, *dout;
    if (hipMalloc(&dF, sizeof(gF)) || hipMalloc(&dt, sizeof(gt)) || hipMalloc(&dout, sizeof(gt))) return 1;
    if (hipMemcpy(dF, gF, sizeof(gF), hipMemcpyHostToDevice) || hipMemcpy(dt, gt, sizeof(gt), hipMemcpyHostToDevice)) return 1;
    for (int d = 0; d < 2; d++) {
        host_sweep<0>(gF, gt, d == 0, ref[d][0]);
        host_sweep<1>(gF, gt, d == 0, ref[d][1]);
        host_sweep<2>(gF, gt, d == 0, ref[d][2]);
    }
    const char *mn[] = {"grid, kernel form, forward", "grid, kernel form, backward", "mfma 4x4x4, forward", "mfma 4x4x4, backward",
                        "mfma 4x4x4, C++ select, fwd", "mfma 4x4x4, C++ select, bwd",
                        "1 select behind next MFMA, f", "1 select behind next MFMA, b",
                        "2 as 1, loads 3 ahead, fwd", "2 as 1, loads 3 ahead, bwd",
                        "3 store per step, no capt, f", "3 store per step, no capt, b",
                        "4 as 2, masks stay in SGPRs,f", "4 as 2, masks stay in SGPRs,b",
                        "5 as 2, C++ select fenced, f", "5 as 2, C++ select fenced, b",
                        "6 one mov under EXEC mask, f", "6 one mov under EXEC mask, b",
                        "7 as 6, loads 3 ahead, fwd", "7 as 6, loads 3 ahead, bwd",
                        "8 no capture, store/step, f", "8 no capture, store/step, b"};
    for (int threads : {64, 512}) {
        u64 hp[36] = {};  // the first of the two repeats
        for (int it = 0; it < 2; it++) {
            if (it == 1 && hipMemcpy(hp, dc, sizeof(hp), hipMemcpyDeviceToHost)) return 1;
            for (int m = 0; m < NM; m++) {
                if (m == 0) hipLaunchKernelGGL(km<11>, 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 1) hipLaunchKernelGGL(km<12>, 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 2) hipLaunchKernelGGL(km<13>, 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 3) hipLaunchKernelGGL(km<14>, 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 4) hipLaunchKernelGGL(km<15>, 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 5) hipLaunchKernelGGL(km<16>, 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 6) hipLaunchKernelGGL((km<13, 1>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 7) hipLaunchKernelGGL((km<14, 1>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 8) hipLaunchKernelGGL((km<13, 2>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 9) hipLaunchKernelGGL((km<14, 2>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 10) hipLaunchKernelGGL((km<13, 3>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 11) hipLaunchKernelGGL((km<14, 3>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 12) hipLaunchKernelGGL((km<13, 4>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 13) hipLaunchKernelGGL((km<14, 4>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 14) hipLaunchKernelGGL((km<13, 5>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 15) hipLaunchKernelGGL((km<14, 5>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 16) hipLaunchKernelGGL((km<13, 6>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 17) hipLaunchKernelGGL((km<14, 6>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 18) hipLaunchKernelGGL((km<13, 7>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 19) hipLaunchKernelGGL((km<14, 7>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 20) hipLaunchKernelGGL((km<13, 8>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (m == 21) hipLaunchKernelGGL((km<14, 8>), 1, threads, 0, 0, dF, dt, dout, o, dc);
                if (hipMemcpy(ho[m], dout, sizeof(gt), hipMemcpyDeviceToHost)) return 1;
            }
        }
        if (hipMemcpy(hc, dc, sizeof(hc), hipMemcpyDeviceToHost)) return 1;
        printf("-- %d lanes (%d wave(s) per SIMD), capture included\n", threads, threads > 256 ? 2 : 1);
        for (int m = 0; m < NM; m++)
            printf("%-30s %5.1f cyc/step  (%.3f x the grid, %.3f x the 4x4x4 kernel form; repeat before it %5.1f)\n", mn[m],
                   hc[11 + m] / 10.0, (double)hc[11 + m] / hc[11 + (m & 1)], (double)hc[11 + m] / hc[13 + (m & 1)], hp[11 + m] / 10.0);
    }
    // arithmetic (wave 0 of the last run): max |v - long double| / max |long double| over all stages
    printf("-- arithmetic, W = %d steps on random F, t\n", W);
    for (int m = 0; m < NM; m++) {
        const int d = m & 1, s0 = d == 0 ? 1 : 0;
        long double mx = 0, df = 0;
        int nb[3] = {0, 0, 0};
        for (int st = s0; st < s0 + W; st++)
            for (int r = 0; r < 8; r++) {
                const int p = 13 * st + r;
                mx = fmaxl(mx, fabsl(ref[d][0][p]));
                df = fmaxl(df, fabsl(ho[m][p] - ref[d][0][p]));
                for (int q = 1; q < 3; q++) nb[q] += ho[m][p] != (double)ref[d][q][p];
            }
        printf("%-30s rel diff from long double %.3Le", mn[m], df / mx);
        if (m >= 2) printf("; of %d values %d differ from the k-ascending fma chain, %d from k-descending", 8 * W, nb[1], nb[2]);
        printf("\n");
    }
    return 0;
}

int main() {
    double *o;
    unsigned long long *c, h[11] = {};
    if (hipMalloc(&o, 512 * sizeof(double)) || hipMalloc(&c, sizeof(h))) return 1;
    const char *nm[] = {"grid, update_dpp, store", "grid, mov_dpp, store", "grid, mov_dpp, capture",
                        "grid, mov_dpp, bare", "broadcast, store", "broadcast, bare", "unrolled, masked store",
                        "unrolled, const-mask capture", "row-bcast, unrolled capture", "row-bcast, store",
                        "grid, two chains interleaved"};
    for (int threads : {64, 512}) {
        for (int it = 0; it < 2; it++) {
            hipLaunchKernelGGL(kr<0>, 1, threads, 0, 0, o, c, W);
            hipLaunchKernelGGL(kr<1>, 1, threads, 0, 0, o, c, W);
            hipLaunchKernelGGL(kr<2>, 1, threads, 0, 0, o, c, W);
            hipLaunchKernelGGL(kr<3>, 1, threads, 0, 0, o, c, W);
            hipLaunchKernelGGL(kr<4>, 1, threads, 0, 0, o, c, W);
            hipLaunchKernelGGL(kr<5>, 1, threads, 0, 0, o, c, W);
            hipLaunchKernelGGL(kr<6>, 1, threads, 0, 0, o, c, W);
            hipLaunchKernelGGL(kr<7>, 1, threads, 0, 0, o, c, W);
            hipLaunchKernelGGL(kr<8>, 1, threads, 0, 0, o, c, W);
            hipLaunchKernelGGL(kr<9>, 1, threads, 0, 0, o, c, W);
            hipLaunchKernelGGL(kr<10>, 1, threads, 0, 0, o, c, W);
        }
        if (hipMemcpy(h, c, sizeof(h), hipMemcpyDeviceToHost)) return 1;
        printf("-- %d lanes (%d wave(s) per SIMD)\n", threads, threads > 256 ? 2 : 1);
        for (int m = 0; m < 11; m++) printf("%-28s %llu cyc/step\n", nm[m], h[m]);
    }
    return mfma4_modes(o);
}
