// mpc_wave.hpp -- the structured kernel's body: one mpcPlanner QP per team of NL = 256 lanes
// (4 wavefronts, one workgroup), all per-QP state on chip, 2 or 3 teams per CU.
//
// Why: the ADMM of OSQP 0.6.2 (reference osqp.h:78, osqp_solve) runs hundreds to thousands of
// iterations per QP; each needs one solve with M = P + sigma I + A' R A plus two SpMVs.  Streaming
// that state from HBM per iteration (the generic one-QP-per-lane kernel) is latency/bandwidth
// bound.  Here a team keeps its QP's factor rows, A values, iterates and bounds in VGPRs and the
// stage-coupling blocks, exchange vectors and the general rows' products in LDS (~50-66 KB per QP
// at N = 20), and the teams of the grid pull QPs from a work queue so QPs that need 4000
// iterations do not stall the ones that need 200.
//
// Shapes (template VS = variables per lane): VS = 1 (n <= 256, the reference's default horizon
// N = 20) at 2 waves per SIMD, or 3 in a launch with the QPs to fill a third team per CU whose
// batches' LDS fits it (the host's launch_teams); VS = 3 (n <= 768, N <= 59) at 1 wave per SIMD.  GS = 2..4
// general-row slots per lane.  WF = the shape's default stage count (19 / 39) as a compile-time
// constant, or 0 for any horizon.  TIER = the two-tier products layout (WaveLds) for obstacle-heavy
// patterns whose one-tier products would cost the CU its second team.
//
// Data layout (stage order v' = 13k + r, see mpc_structure.hpp):
//   var slot s of lane L  <-> v' = NL s + L   (VS slots):  x, q, P_jj, the variable's box row
//       (A value, z, y, l, u, type), row v'%13 of Ainv_k (13) and an 8-wide coupling row
//   general-row slot s    <-> g = NL s + L    (GS slots): 4 A values + columns, z, y, l, u, type
//   LDS (WaveLds): F_k (the 8x8 stage-coupling blocks), exchange vectors r / t / e / x~, team
//       reduction scratch, the int16 entry -> product-slot table, D / E (VS = 1), the products
//       buffer (column-slot layout); the check deltas of VS = 1 take dead LDS (WaveLds::DLT_OFF)
//
// Linear solve (block LDL^T of the stage-tridiagonal M, with Ahat_k the Schur complements):
//   G_k = Bbar_k Ahat_k^{-1} (8 x 13), F_k = G_k[:, :8]
//   forward : a_0 = r_0[:8],  a_{k+1} = r_{k+1}[:8] - G_k[:, 8:] r_k[8:] - F_k a_k   (8-dim recursion)
//   middle  : e_k = Ahat_k^{-1} (a_k, r_k[8:])                                     (parallel)
//   backward: x_{N-1} = e_{N-1},  x_k = e_k - G_k^T x_{k+1}[:8]                      (8-dim recursion)
// The 8-dim recursions are the only serial part (2 x (N-1) steps of an 8x8 mat-vec); one
// wavefront of the team (rw) runs each on its 8x8 lane grid with DPP / permlane reductions while
// the others wait at the barrier -- the parallel phases (rhs gather, S1, S3, S5, update,
// products) use all 256 lanes.
//
// The kernel body is written against a team policy `WV`: lane() in [0, NL), sync() (team barrier
// with LDS visibility), bcast(v, j) (v of lane j of the CALLER's wavefront), max()/sum() over the
// team, so the same code runs on the GPU (policy GpuTeam in impc_qp.hip) and, for tests only, in an
// NL-thread CPU emulation (tests/native/wave_emu.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/impc_qp.h"
#include "admm_core.hpp"
#include "mpc_structure.hpp"
#include "sweep_mfma_map.hpp"

namespace impc {

#define IMPC_WF __host__ __device__ __forceinline__

// The serial recursions' wavefront at a raised issue priority (s_setprio 2) while it runs them: the
// co-resident team's waves share its SIMD, and the recursion is the team's critical path (round 6:
// config 3 213.9 / 214.1 -> 210.8 / 210.5 ms per launch at priority 2, 211.1 / 211.2 at 3; identical
// iterations)
#if defined(__HIP_DEVICE_COMPILE__)
#define IMPC_PRIO_UP() __builtin_amdgcn_s_setprio(2)
#define IMPC_PRIO_DOWN() __builtin_amdgcn_s_setprio(0)
#else
#define IMPC_PRIO_UP() ((void)0)
#define IMPC_PRIO_DOWN() ((void)0)
#endif
// Phase-cost experiments (tools/exp.sh only): IMPC_DUP=<section id> runs that idempotent phase of
// the ADMM iteration twice; the bench's time difference is the phase's marginal cost.
#ifndef IMPC_DUP
#define IMPC_DUP -1
#endif
#define IMPC_REP(X) for (int rep_ = 0; rep_ < (IMPC_DUP == (X) ? 2 : 1); rep_++)

// Variants measured slower and removed in round 4 (their numbers stay in profiles/r0*/exp/README.md,
// their code in git history): the twisted two-ended elimination, pair-blocked and chunked stage
// recursions, folded recursion subtractions, wave priorities, LDS-only barriers, register-held pair
// captures, split dot-product chains, opaque phase bases, delta-less update instances, per-step
// history / store captures, (c, S)-carried sweeps, off-chip scaling vectors, Cholesky / 1x1-pivot
// stage inverses.  What is left is the measured-best form of each phase.
// Removed in round 13, each a build switch beside its successor until then (commit 60fcdf2 is the
// last that holds their code; the numbers are in profiles/r0*/ and profiles/r1*/): the round-4
// factorisation loops (IMPC_FACT2=0; setup 0.440 vs 0.358 ms per N = 40 QP) and the long shape's
// factorisation with the barrier between E_k and the next assembly (IMPC_FACT3=0; config 5 610.9 vs
// 604.0 ms), partial unrolls of the 13-term products and other assembly batch sizes (IMPC_F2U,
// IMPC_F2B), the four-chunk long-horizon sweeps (IMPC_CHUNK5=0; 1251.6 vs 1209.6 ms per config-5
// launch), the default horizon in chunks with an LDS region of its own (IMPC_CHUNK19; slower at two
// teams per CU) and the chunk rounds' repeat loops (IMPC_CHDUP), the lane-grid default-horizon sweep
// in device code (IMPC_SWEEP_MFMA=0; config 3 184.0 vs 171.8-171.9 ms), the matrix-instruction sweep
// without its prologue in front of the barrier or its early stores (IMPC_SWEEP_PRO / IMPC_SWEEP_EARLY
// = 0; 145.7-146.3 and 143.9-144.0 vs 142.2-142.4 ms; early stores without the prologue 147.3-147.4),
// recursion priorities other than 2 (IMPC_PRIO), the every-lane team-reduction combine of the
// four-wavefront team (IMPC_LCOMB=0 in impc_qp.hip; 210.35 vs 206.8 ms) and the emulation's branch
// counters (IMPC_COUNT, defined by nothing).

// Scheduling hint for the parallel phases' LDS reads: under the kernel's register pressure the
// machine scheduler otherwise issues them one ds_read2 at a time, each followed by its own
// lgkmcnt wait (S3 = 7 serialised LDS round trips); this asks for the phase's reads first, then
// its arithmetic, so the round trips overlap.
#if defined(__HIP_DEVICE_COMPILE__)
#define IMPC_LOADS_FIRST(NR, NV)                            \
    do {                                                    \
        __builtin_amdgcn_sched_group_barrier(0x100, NR, 0); \
        __builtin_amdgcn_sched_group_barrier(0x002, NV, 0); \
    } while (0)
#else
#define IMPC_LOADS_FIRST(NR, NV) ((void)0)
#endif

struct WaveTables {
    int32_t n, m, mg, N, W, CG, nnzP, nnzA;
    const int32_t *var_orig, *var_pdiag, *var_boxrow, *var_boxpos;
    const int32_t *gen_row, *gen_col, *gen_pos, *colg, *term_ptr, *term;
    int32_t HS;               // heavy columns (second products tier), MpcStructure::HS; 0: one tier
    const int32_t *col_hid;   // [n] heavy-column index or -1 (stage order)
    int32_t T1r;              // first-tier rows: cg4(CG) (one tier) or kProdTier1 (two tiers)
    // the scaling vectors D, E of a shape without them in its fixed LDS layout (WaveLds::ONCHIP
    // false): 1 = in LDS after the products region when the CU's LDS has the room (the batch
    // setup decides), 0 = in the per-QP HBM scratch (WaveIO::scal).  (In the struct's padding.)
    int32_t scal_lds;
};

struct WaveIO {
    int64_t B;
    const double *Px, *q, *Ax, *l, *u, *xws, *yws;  // QP-major inputs
    int32_t has_ws;    // 0: none, 1: x and y, 2: x with y = 0 (yws not read)
    double *xo, *yo;   // QP-major outputs (unscaled)
    double *scal;      // per-QP scratch [B][n + n + mg]: D, E(box), E(general)
    impc_info *info;
    unsigned long long *sec = nullptr;  // section-profiling build only: cycle sums [kSecCount]
    unsigned long long *qpt = nullptr;  // profiling: per-QP (start, end) device clock [B][2]
    // shared-structure values (impc_batch_set_values_shared): Px / Ax above are one copy each,
    // A entry p is Ax_var[b][vmap[p]] when vmap[p] >= 0
    int32_t shared = 0;
    int64_t nvar = 0;
    const int32_t *vmap = nullptr;
    const double *Ax_var = nullptr;
    // persistent workspace (impc_batch_set_persistent, OSQP's workspace between solves): per QP
    // [kPersistHdr + 3 n + 2 mg]: cost-scaling factors of the Ruiz passes, rho, then the scaled
    // iterates x, z (box), y (box), z (general), y (general).  resume = 2 (osqp_update_P / _A: new
    // matrix values): Ruiz scaling afresh on the new data, the stored rho and scaled iterates kept, as
    // OSQP 0.6.2 unscales, rescales and refactors but keeps work->x, z, y.  resume = 1: scale with the stored
    // factors (the same D, E, c and scaled P, A as the first setup), start from the stored rho and
    // iterates, and -- when q_updated -- scale q as osqp_update_lin_cost does ((D q) c).
    double *persist = nullptr;
    int32_t resume = 0, q_updated = 0;
    // per-QP time limits [B] (impc_batch_set_time_limits: each solveTraj call sets its own), or
    // nullptr for the settings' time_limit
    const double *tlim = nullptr;
    // resume = 2 with q updated after the matrix update: the q the workspace held when P / A
    // changed [B][n].  OSQP's scale_data after osqp_update_P / _A normalises the cost with that q;
    // the new q (io.q) is then scaled as osqp_update_lin_cost does, (D q) c
    const double *q_scale = nullptr;
};

constexpr int kPersistHdr = 24;      // ct[0 .. kPersistMaxScaling), rho at kPersistHdr - 1
constexpr int kPersistMaxScaling = 20;
IMPC_HD int64_t persist_stride(int n, int mg) { return kPersistHdr + 3 * (int64_t)n + 2 * (int64_t)mg; }

// Section profiling (profiling build of the library only, -DIMPC_SECTION_PROF): lane 0 of each
// team accumulates s_memtime deltas per section; IMPC_SEC(X) closes section X.
enum {
    kSecSetup, kSecFactor, kSecWarm, kSecRhs, kSecS1, kSecFwd, kSecS3, kSecBwd, kSecS5, kSecUpdate, kSecProducts,
    kSecChecks, kSecOutput, kSecFAsm, kSecFDense, kSecIters = 15, kSecCount = 16
};
// The clock is the 100 MHz s_memrealtime counter (the one the time-limit path reads; a
// SHADER_CYCLES s_getreg reads 0 on gfx950, and s_memtime perturbed the LDS wait counts of this
// kernel's instrumented build).  Units: 10 ns ticks.
#if defined(IMPC_SECTION_PROF) && defined(__HIP_DEVICE_COMPILE__)
#define IMPC_SEC_CLOCK() ((uint64_t)__builtin_amdgcn_s_memrealtime())
#define IMPC_SEC(X)                             \
    do {                                        \
        uint64_t t_ = IMPC_SEC_CLOCK();         \
        sec_acc[X] += t_ - sec_t0;              \
        sec_t0 = t_;                            \
    } while (0)
#define IMPC_SEC_START() (sec_t0 = IMPC_SEC_CLOCK())
#else
#define IMPC_SEC(X) ((void)0)
#define IMPC_SEC_START() ((void)0)
#endif

// team reduction scratch (WaveLds RED_OFF): values x wavefronts of one team reduction in its first
// kRedUsed doubles; the last 8 hold the rho table of the three-teams-per-CU instance (WaveQP::kRhoTab)
constexpr int kRedLen = 128;
constexpr int kRedUsed = kRedLen - 8;

// LDS doubles per wave for (VS, GS)
template <int NL, int VS, int GS>
struct WaveLds {
    static constexpr int NMAX = NL * VS;
    static constexpr int WMAX = (NMAX + 5) / 13 - 1;       // max control stages
    // stage count whose recursions are fully unrolled (the reference's default horizon N = 20
    // for the one-variable-per-lane shape, N = 40 for the long-horizon shape)
    static constexpr int WSPEC = NMAX <= 256 ? 19 : 39;
    // a second compile-time horizon of the long shape: the reference's live planner, N = 30
    // (autonomous_flight planner_param.yaml:25, mpc_interactive mpc_param.yaml:1); 0 = none
    static constexpr int WSPEC2 = NMAX <= 256 ? 0 : 29;
    // exchange vector length: zero tail past NMAX, and room for the factorisation scratch
    // (the sweeps' two-steps-ahead prefetches read at most 13 (W + 4) + 8 past the start), and
    // room for the factorisation's dense stage scratch (FA .. DIAGX below)
    static constexpr int NP = (NMAX + 48 > (779 + NMAX + 3) / 4) ? NMAX + 48 : (779 + NMAX + 3) / 4;
    static constexpr int F_OFF = 0;                         // [WMAX][64]
    static constexpr int R_OFF = F_OFF + WMAX * 64;         // rbuf
    static constexpr int T_OFF = R_OFF + NP;                // tbuf
    static constexpr int E_OFF = T_OFF + NP;                // ebuf
    static constexpr int X_OFF = E_OFF + NP;                // xbuf
    static constexpr int RED_OFF = X_OFF + NP;              // team reduction scratch [kRedLen]
    static constexpr int JUNK_OFF = RED_OFF + kRedLen;      // per-lane discard slots [NL]
    static constexpr int GSLOT_OFF = JUNK_OFF + NL;         // int16 [4 NL GS]: general entry -> product slot
    // One-variable-per-lane shape: the Ruiz scaling vectors D, E live here (the long-horizon shape
    // keeps them in HBM / registers: its LDS is full).  Layout: [var slots NMAX][box rows NMAX]
    // [general slots NL GS].
    static constexpr bool ONCHIP = VS == 1;
    static constexpr int VEC_N = 2 * NMAX + NL * GS;
    static constexpr int SCL_OFF = GSLOT_OFF + NL * GS;           // D, E (scaling)
    // The ADMM deltas dx, dy of that shape (written by the update phase of a check iteration, read
    // only by the check that follows it, each lane its own) take LDS that is dead between an
    // iteration's S5 and the next rhs gather, at compile-time offsets: dx[v] in the per-lane
    // discard slots, dy of the box rows in R[0 .. NL), dy of general-row slots 0 and 1 in
    // T[0 .. NL) and E[0 .. NL).  The exchange vectors' tails stay out (S3 of the default horizon's
    // last stage reads R[NMAX .. NMAX + 4) and needs the zeros there).  General-row slots 2 and up
    // (mg > 512) keep a region of their own, DLT_OFF.
    static constexpr int DLT_OFF = SCL_OFF + (ONCHIP ? VEC_N : 0);
    static constexpr int DLT_N = ONCHIP && GS > 2 ? NL * (GS - 2) : 0;
    static constexpr int P_OFF = DLT_OFF + DLT_N;  // products, column-slot layout (size below)
    static constexpr int CGM = 24;                          // max general entries per column
    // products region: entry t < T1r of column v at t * stride(n) + v (stride = n rounded up to
    // 64, plus a pad), so a column's gather is independent, conflict-free reads.  When that one
    // tier (T1r = CG4 rows of all n columns) would cost occupancy, a second tier holds the rest:
    // T1r = 4 and entry t >= 4 of a heavy column (index h = col_hid) at
    // 4 stride(n) + (t - 4)(HS + 1) + h -- only the positions and slack of a stage carry one
    // product per obstacle row, so the second tier is (CG4 - 4) rows of the HS heavy columns
    // instead of CG4 rows of all n (K = 21: 21 KB instead of 49 KB).  It doubles as the
    // factorisation's (4g + e) scratch and general-row rho.  Sized from the pattern at run time,
    // followed by 8 discard slots (index p_size).
    static constexpr int T1 = kProdTier1;
    static IMPC_WF int cg4(int CG) { return (CG + 3) & ~3; }
    // +PAD: the obstacle rows of one stage write their products to the same column in different
    // entry slots; a stride that is not a multiple of 16 doubles puts those ds_write_b64 (bank =
    // dword mod 32, 16-lane groups) on distinct banks.  Reads stay lane-contiguous.
    static constexpr IMPC_WF int stride(int n) { return ((n + 63) & ~63) + 1; }
    // the factorisation uses it as (4g + e) scratch followed by the general rows' rho (RHOG_P)
    static IMPC_WF int hsp(int HS) { return HS + 1; }  // second-tier row length
    static IMPC_WF int p_size(int CG, int n, int HS, int mg, int T1r) {
        const int c = T1r * stride(n) + (cg4(CG) > T1r ? (cg4(CG) - T1r) * hsp(HS) : 0), f = 5 * mg;
        return c > f ? c : f;
    }
    static IMPC_WF int p_size(const WaveTables &T) { return p_size(T.CG, T.n, T.HS, T.mg, T.T1r); }
    // D, E in LDS for a shape without them in the fixed layout (WaveTables::scal_lds)
    static IMPC_WF int scl2_off(const WaveTables &T) { return P_OFF + p_size(T) + 8; }
    static IMPC_WF int size(const WaveTables &T) {
        return scl2_off(T) + (!ONCHIP && T.scal_lds ? 2 * T.n + T.mg : 0);
    }
    // factorisation aliases (inside R..X region and the products buffer)
    static constexpr int FA = R_OFF, FL = FA + 169, FI = FL + 169, FB = FI + 169, FG = FB + 104, FE = FG + 104,
                         DIAGX = FE + 64;
    // general rows' rho during the factorisation: products region + 4 mg
    static_assert(DIAGX + NMAX <= RED_OFF, "factorisation scratch does not fit");
    // the coupling block of odd stages (the long shape's B_k is double-buffered by stage parity)
    static constexpr int FB2 = DIAGX + NMAX;
    static_assert(VS != 3 || FB2 + 104 <= RED_OFF, "factorisation scratch does not fit");
};

// the status register's mark of a failed refactorisation inside the iteration loop (never a
// reported status: the exit path writes UNSOLVED)
constexpr int64_t kRefailMark = -1000;

struct WaveRho {
    double rho, r_eq, r_ineq, r_loose, i_eq, i_ineq, i_loose;
    IMPC_WF void set(double r) {
        rho = r;
        r_ineq = r;
        r_eq = kRhoEqOverIneq * r;
        r_loose = kRhoMin;
        i_ineq = 1. / r_ineq;
        i_eq = 1. / r_eq;
        i_loose = 1. / r_loose;
    }
    // Value selection by arithmetic (t in {-1, 0, 1}): a ternary between fields would become a
    // select of member addresses and keep the whole per-QP object out of registers.
    IMPC_WF double of(int t) const {
        double e = t > 0 ? 1.0 : 0.0, i = t == 0 ? 1.0 : 0.0, l = t < 0 ? 1.0 : 0.0;
        return (e * r_eq + i * r_ineq) + l * r_loose;
    }
    IMPC_WF double inv(int t) const {
        double e = t > 0 ? 1.0 : 0.0, i = t == 0 ? 1.0 : 0.0, l = t < 0 ? 1.0 : 0.0;
        return (e * i_eq + i * i_ineq) + l * i_loose;
    }
};

IMPC_WF int row_type(double l, double u) {  // set_rho_vec (auxil.h:34)
    if ((l < -kInf * kMinScaling) && (u > kInf * kMinScaling)) return -1;
    if (u - l < kRhoTol) return 1;
    return 0;
}

// WF: the stage count W fixed at compile time (LD::WSPEC, the default horizon: every stage loop
// and LDS offset becomes a constant and no runtime-W code path shares the kernel's registers), or 0
// for any W read from the tables.
// TIER: the batch uses the two-tier products layout (WaveLds, T1r = kProdTier1); a one-tier
// batch (T1r = CG4) runs the TIER = false instance, whose gathers are the plain CG4-row loops.
// DENSE: the three-teams-per-CU instance (168 VGPRs per lane).  Its iteration loop is arranged so
// that nothing in it comes from scratch or scalar memory: the rows' rho / 1/rho are read from a
// six-entry LDS table by row type (kRhoTab) instead of held per row, the loop-invariant operands
// are per-pass values (begin_pass), one general entry's addresses are formed at their uses (gpk)
// and the projections are written out (clampz_raw).  The same operations on the same values as the
// plain form, which every other instance keeps unchanged.
template <class WV, int NL, int VS, int GS, int WF = 0, bool TIER = false, bool DENSE = false>
struct WaveQP {
    using LD = WaveLds<NL, VS, GS>;
    static_assert(WF == 0 || WF == LD::WSPEC || WF == LD::WSPEC2, "WF is 0 or one of the shape's compiled horizons");
    IMPC_WF int Wst() const { return WF ? WF : T.W; }
    WV &wv;
    const WaveTables &T;
    const WaveIO &io;
    const DevSettings &st;
    double *lds;
    int L;
    // ---- variable slots
    double x[VS], q[VS], pd[VS], ab[VS], zb[VS], yb[VS], lb[VS], ub[VS], dxv_[VS], dyb_[VS];
    double ainv[VS][13], cp[VS][8];
    int bt[VS], vs_[VS], vr_[VS], hid_[VS];
    bool vok[VS];
    // ---- general-row slots
    double a[GS][4], z[GS], y[GS], lg[GS], ug[GS], dyg_[GS];
    int gc[GS][4], gt[GS];
    bool gok[GS];
    WaveRho R;
    double c = 1.0, cinv = 1.0;
    int rw = 0;  // the wavefront that runs the stage recursions for this QP
    // settings / pattern scalars the ADMM iteration reads, held in registers (a grouped launch's
    // tables and settings live in global memory: read in the loop, each is a scalar-memory round
    // trip after every barrier)
    double sig_, alp_;
    int c4_, sd_;
#if defined(IMPC_SECTION_PROF) && defined(__HIP_DEVICE_COMPILE__)
    uint64_t sec_t0 = 0, sec_acc[kSecCount] = {};
#endif

    IMPC_WF WaveQP(WV &w, const WaveTables &t, const WaveIO &i, const DevSettings &s, double *l)
        : wv(w), T(t), io(i), st(s), lds(l), L(w.lane()), sig_(s.sigma), alp_(s.alpha), c4_(LD::cg4(t.CG)),
          sd_(LD::stride(t.n)) {}

    // the lane index, opaque to the optimiser: per-lane LDS addresses derived from it are formed
    // where they are used instead of being hoisted out of the ADMM loop (dozens of loop-invariant
    // address registers otherwise spill and come back as scratch loads inside the recursions)
    IMPC_WF int lane_o() const {
        int l = L;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(l));
#endif
        return l;
    }

    // a per-lane value the optimiser must treat as freshly computed (see lane_o)
    IMPC_WF static void opaque(int &v) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(v));
#else
        (void)v;
#endif
    }

    // team-uniform: R stays in scalar registers, and each row's rho / 1/rho is selected from it
    // by the row type where used instead of occupying 4 VGPRs per row slot
    // DENSE: the same six values also in LDS (kRhoTab + 1 + t: rho of row type t, + 4 + t: 1/rho),
    // where the iteration reads them with its other LDS operands.  (The optimiser hoists the selects
    // out of the ADMM loop: 12 VGPRs of the three-per-CU instance's 168.)  Every caller is team-wide
    // code; the barrier orders the table against the reads of the factorisation that follows.
    static constexpr int kRhoTab = LD::RED_OFF + kRedUsed;
    IMPC_WF void set_rho(double r) {
        R.set(wv.uniform(r));
        if constexpr (DENSE) {
            if (L == 0) {
                double *t = lds + kRhoTab;
                t[0] = R.r_loose, t[1] = R.r_ineq, t[2] = R.r_eq;
                t[3] = R.i_loose, t[4] = R.i_ineq, t[5] = R.i_eq;
            }
            wv.lsync();
        }
    }
    IMPC_WF double rho_of(int t) const {
        if constexpr (DENSE) return lds[kRhoTab + 1 + t]; else return R.of(t);
    }
    IMPC_WF double rho_inv(int t) const {
        if constexpr (DENSE) return lds[kRhoTab + 4 + t]; else return R.inv(t);
    }
    IMPC_WF double rhob(int s) const { return rho_of(bt[s]); }
    IMPC_WF double rhoib(int s) const { return rho_inv(bt[s]); }
    IMPC_WF double rhog_(int s) const { return rho_of(gt[s]); }
    IMPC_WF double rhoig_(int s) const { return rho_inv(gt[s]); }

    // DENSE: the loop-invariant per-lane operands of the iteration -- the projection bounds, q and the
    // second products tier's geometry -- as values of their own for each pass of the iteration loop
    // (begin_pass, once per check interval).  Held as the members above they live from the setup to
    // the output; at 168 VGPRs the register allocator splits such a range around the sweeps and
    // reloads it from scratch in front of each use, one exposed round trip per value and iteration
    // (five bounds in the update phase, the tier address and the row length in the rhs gather).  A
    // value that lives for the pass only, and is used in every iteration of it, keeps its register.
    struct Pass {
        double lb[VS], ub[VS], lg[GS], ug[GS], q[VS];
        int hq[VS];  // products index of the lane's second-tier column, or -1
        int hp;      // second-tier row length
    } ps_;
    IMPC_WF static void opaque(double &v) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(v));
#else
        (void)v;
#endif
    }
    IMPC_WF void begin_pass() {
        if constexpr (DENSE) {
            static_assert(!DENSE || (TIER && WF > 0), "the denser instance is the two-tier default horizon's");
            auto own = [](double v) {
                opaque(v);
                return v;
            };
            _Pragma("unroll") for (int s = 0; s < VS; s++) {
                ps_.lb[s] = own(lb[s]);
                ps_.ub[s] = own(ub[s]);
                ps_.q[s] = own(q[s]);
                ps_.hq[s] = hid_[s] >= 0 ? LD::T1 * LD::stride(13 * (WF + 1) - 5) + hid_[s] : -1;
                opaque(ps_.hq[s]);
            }
            _Pragma("unroll") for (int s = 0; s < GS; s++) {
                ps_.lg[s] = own(lg[s]);
                ps_.ug[s] = own(ug[s]);
            }
            ps_.hp = LD::hsp(T.HS);
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "+s"(ps_.hp));  // (team-uniform: stays in a scalar register)
#endif
        }
    }
    // packed (product slot << 16 | column) of general entry e of slot s as the iteration uses it.
    // DENSE: the last entry's is opaque there, so its two LDS addresses are formed at their uses
    // (6 VALU instructions) instead of held across the loop -- the registers that took the last
    // reload, of one such address, out of the update phase.
    IMPC_WF int gpk(int s, int e) const {
        int g = gc[s][e];
        if (DENSE && s == GS - 1 && e == 3) opaque(g);
        return g;
    }

    // ADMM deltas of the last iteration (termination checks only): LDS or registers
    // (LDS of the one-variable-per-lane shape: WaveLds::DLT_OFF's comment)
    IMPC_WF double &dxv(int s) {
        if constexpr (LD::ONCHIP) return lds[LD::JUNK_OFF + NL * s + L]; else return dxv_[s];
    }
    IMPC_WF double &dyb(int s) { if constexpr (LD::ONCHIP) return lds[LD::R_OFF + NL * s + L]; else return dyb_[s]; }
    IMPC_WF double &dyg(int s) {
        if constexpr (LD::ONCHIP)
            return lds[(s == 0 ? LD::T_OFF : s == 1 ? LD::E_OFF : LD::DLT_OFF + NL * (s - 2)) + L];
        else
            return dyg_[s];
    }
    // scaling vectors D, E (set by scale(), read at warm start, checks and unscaling): layout
    // [D n][E box n][E general mg], in LDS or in the per-QP HBM scratch
    IMPC_WF double *scal(int64_t b) {
        if constexpr (LD::ONCHIP) return lds + LD::SCL_OFF;
        else return T.scal_lds ? lds + LD::scl2_off(T) : io.scal + b * (int64_t)(2 * T.n + T.mg);
    }

    IMPC_WF double *F() { return lds + LD::F_OFF; }
    IMPC_WF double *rbuf() { return lds + LD::R_OFF; }
    IMPC_WF double *tbuf() { return lds + LD::T_OFF; }
    IMPC_WF double *ebuf() { return lds + LD::E_OFF; }
    IMPC_WF double *xbuf() { return lds + LD::X_OFF; }
    IMPC_WF double *pbuf() { return lds + LD::P_OFF; }

    // The long shape's factorisation keeps the Schur complement E_k in the register of the lane that
    // assembles M_k+1's matching entry (the destinations are assigned so that lane 8i + j computes
    // E[i][j] and assembles M[i][j]), double-buffers B_k by stage parity and drops the barrier between
    // E_k and the next stage's assembly.  Config 5's closed loop 610.9 -> 604.0 ms; on the default
    // horizon it measured 214.3 -> 215.2 ms, so that shape keeps the barrier
    // (profiles/r05/exp_phase/README.md)
    static constexpr bool F3 = VS == 3;

    // Chunked stage recursions of the long horizon (the compile-time W = 39 and W = 29 instances of
    // the three-slot shape).  That shape runs one team per CU, so the three wavefronts that wait out
    // a serial sweep leave their SIMDs idle.  Each W-step sweep runs as five chunks on the four
    // wavefronts, CL = 2 ceil(W/10) steps each and W - 4 CL in the last (W = 39: 8, 8, 8, 8, 7;
    // W = 29: 6, 6, 6, 6, 5), in two rounds.  Round 1: wave 0 runs the first chunk from the true start
    // while waves 1..3 run chunks 1..3 from zero for the chunk-end values only.  After a barrier,
    // round 2: each of waves 1..3 forms its chunk's true start from those ends and the chunk operators
    // (products of the chunk's -F_k, or -F_k^T backward, built with the factorisation:
    // a_{o+CL} = a^_{o+CL} + P a_o) in one 8-lane reduction and runs its chunk again, and wave 0 runs
    // the fifth, whose start a_4CL = a^_4CL + P3 a^_3CL + P3P2 a^_2CL + P3P2P1 a_CL is still one
    // 8-lane reduction.  Dependent chain per sweep: W steps -> 2 CL steps and one reduction (W = 39:
    // 16; the round-4 form, four chunks of 2 ceil(W/8), had 20 and measured 1251.6 vs 1209.6 ms per
    // config-5 launch).  Operators and ends live in the F region's tail (blocks >= W + 3, never
    // read).  CL is even, so every chunk starts on an even stage (the sweeps' index parity).
    static constexpr bool CHUNK = WF > 0 && NL == 256 && VS == 3;
    static constexpr int CL = WF > 0 ? 2 * ((WF + 9) / 10) : 2;
    static constexpr int CLAST = WF - 4 * CL;
    static constexpr int CH_OFF = LD::F_OFF + 64 * (WF + 3);
    // forward P1 P2 P3 P2P1 P3P2 P3P2P1, then the same backward (+kChB), then the ends
    enum { kChP1 = 0, kChP2 = 64, kChP3 = 128, kChP21 = 192, kChP32 = 256, kChP321 = 320, kChB = 384 };
    static constexpr int kChEnd = 768;
    static constexpr int kChEnds = 24;  // chunk-end values per direction
    static_assert(!CHUNK || CH_OFF + kChEnd + 2 * kChEnds <= LD::R_OFF, "chunk operators do not fit the F region");
    IMPC_WF double *chbuf() const { return lds + CH_OFF; }
    static_assert(!CHUNK || (CLAST >= 1 && CLAST <= CL), "chunk lengths");

    // zero the exchange vectors (their tails are the zero slots read by padded entries)
    IMPC_WF void clear_exchange() {
        for (int i = L; i < 4 * LD::NP; i += NL) lds[LD::R_OFF + i] = 0.0;
        wv.sync();
    }

    // ------------------------------------------------------------------ load + scaling
    IMPC_WF void load(int64_t b) {
        const int n = T.n, m = T.m;
        const int64_t bn = b * n, bm = b * m, bP = io.shared ? 0 : b * T.nnzP, bA = io.shared ? 0 : b * T.nnzA;
        // A value at CSC position p of this QP (shared-structure batches: the per-QP override)
        auto Aval = [&](int p) -> double {
            if (io.shared) {
                const int32_t v = io.vmap[p];
                return v >= 0 ? io.Ax_var[b * io.nvar + v] : io.Ax[p];
            }
            return io.Ax[bA + p];
        };
        _Pragma("unroll") for (int s = 0; s < VS; s++) {
            int v = NL * s + L;
            vok[s] = v < n;
            vs_[s] = vok[s] ? v / 13 : 0;
            vr_[s] = vok[s] ? v % 13 : 0;
            hid_[s] = TIER && vok[s] ? T.col_hid[v] : -1;  // second products tier (TIER batches)
            x[s] = q[s] = pd[s] = ab[s] = zb[s] = yb[s] = lb[s] = ub[s] = dxv_[s] = dyb_[s] = 0.0;
            bt[s] = 0;
            // the branch-free phases read a slot's factor rows whether or not it holds a variable
            _Pragma("unroll") for (int cc = 0; cc < 13; cc++) ainv[s][cc] = 0.0;
            _Pragma("unroll") for (int cc = 0; cc < 8; cc++) cp[s][cc] = 0.0;
            if (vok[s]) {
                int ov = T.var_orig[v];
                q[s] = (io.q_scale ? io.q_scale : io.q)[bn + ov];
                int pp = T.var_pdiag[v];
                pd[s] = pp >= 0 ? io.Px[bP + pp] : 0.0;
                ab[s] = Aval(T.var_boxpos[v]);
                int br = T.var_boxrow[v];
                lb[s] = dmin(dmax(io.l[bm + br], -kInf), kInf);
                ub[s] = dmin(dmax(io.u[bm + br], -kInf), kInf);
            }
        }
        _Pragma("unroll") for (int s = 0; s < GS; s++) {
            int g = NL * s + L;
            gok[s] = g < T.mg;
            z[s] = y[s] = lg[s] = ug[s] = dyg_[s] = 0.0;
            gt[s] = 0;
            const int16_t *gs = (const int16_t *)(lds + LD::GSLOT_OFF);
            const int pz = LD::p_size(T);
            _Pragma("unroll") for (int e = 0; e < 4; e++) {
                a[s][e] = 0.0;
                gc[s][e] = (pz << 16) | LD::NMAX;  // discard slot / zero tail of the x exchange
            }
            if (gok[s]) {
                _Pragma("unroll") for (int e = 0; e < 4; e++) {
                    int col = T.gen_col[4 * g + e], pos = T.gen_pos[4 * g + e];
                    if (col >= 0) {
                        gc[s][e] = ((int)gs[4 * g + e] << 16) | col;
                        a[s][e] = Aval(pos);
                    }
                }
                int row = T.gen_row[g];
                lg[s] = dmin(dmax(io.l[bm + row], -kInf), kInf);
                ug[s] = dmin(dmax(io.u[bm + row], -kInf), kInf);
            }
        }
        // deltas read by a check before any ADMM step: zero.  Those in the exchange vectors are
        // zeroed with them at the end of factorize(), after the setup's last use of that LDS as
        // scratch, and dx after it in solve() (the discard slots still hold the wavefronts'
        // placement here); the region of slots 2 and up here
        if constexpr (LD::ONCHIP)
            _Pragma("unroll") for (int s = 2; s < GS; s++) dyg(s) = 0.0;
    }

    // Per-workgroup tables (once per launch): the product slot of every general-row entry
    // (mpc_structure colg inverted into the column-slot layout, int16 in LDS; padded entries get
    // the discard slot), and a zeroed products region (slots no entry maps to must read 0).
    static IMPC_WF void load_tables(WV &w, const WaveTables &T, double *lds) {
        int16_t *gs = (int16_t *)(lds + LD::GSLOT_OFF);
        const int pz = LD::p_size(T);
        for (int e = w.lane(); e < 4 * NL * GS; e += NL) gs[e] = (int16_t)pz;
        double *pb = lds + LD::P_OFF;
        for (int e = w.lane(); e < pz + 8; e += NL) pb[e] = 0.0;
        w.sync();
        for (int e = w.lane(); e < T.n * T.CG; e += NL) {
            const int v = e / T.CG, t = e % T.CG, id = T.colg[e];
            if (id >= 0)
                gs[id] = (int16_t)(t < T.T1r ? t * LD::stride(T.n) + v
                                             : T.T1r * LD::stride(T.n) + (t - T.T1r) * LD::hsp(T.HS) + T.col_hid[v]);
        }
        w.sync();
    }

    IMPC_WF void zero_products() {
        double *pb = pbuf();
        const int cnt = LD::p_size(T) + 8;
        for (int i = L; i < cnt; i += NL) pb[i] = 0.0;
        wv.sync();
    }

    // column index / product slot of general entry e of slot s (packed: slot << 16 | column)
    IMPC_WF int gcol(int s, int e) const { return gc[s][e] & 0xFFFF; }
    IMPC_WF int gdst(int s, int e) const { return gc[s][e] >> 16; }

    // col_gather's loop for C4 = 4 NG: s = 0 + group 0 + group 1 + ..., each group (p0+p1)+(p2+p3)
    template <int NG>
    IMPC_WF static double gather_n(const double *pb, int sd) {
        double p[4 * NG];
        _Pragma("unroll") for (int t = 0; t < 4 * NG; t++) p[t] = pb[t * sd];
        double s = 0.0;
        _Pragma("unroll") for (int g = 0; g < NG; g++) s += (p[4 * g] + p[4 * g + 1]) + (p[4 * g + 2] + p[4 * g + 3]);
        return s;
    }

    // gather sum over the general entries of column v (column-slot layout, independent reads;
    // the sums add groups of four in entry order).  TIER: the first T1 rows, then -- for a heavy
    // column, h = its second-tier index (hid_, -1 for a light column) -- the second tier
    IMPC_WF double col_gather(int v, int h) {
        const double *pb = pbuf() + v;
        // (a compile-time horizon's products stride is a constant, n = 13 (WF + 1) - 5, so the
        // gather's reads take immediate offsets instead of per-read address arithmetic)
        const int C4 = c4_, sd = WF ? LD::stride(13 * (WF + 1) - 5) : sd_;
        double s = 0.0;
        if constexpr (!TIER) {
            (void)h;
            // the same sum, every read of the column issued before the first add (C4 is uniform)
            switch (C4) {
                case 4: return gather_n<1>(pb, sd);
                case 8: return gather_n<2>(pb, sd);
                case 12: return gather_n<3>(pb, sd);
                case 16: return gather_n<4>(pb, sd);
                case 20: return gather_n<5>(pb, sd);
                default: break;
            }
            for (int t = 0; t < C4; t += 4) {
                const double p0 = pb[t * sd], p1 = pb[(t + 1) * sd], p2 = pb[(t + 2) * sd], p3 = pb[(t + 3) * sd];
                s += (p0 + p1) + (p2 + p3);
            }
        } else {
            static_assert(LD::T1 == 4, "one first-tier group");
            s += (pb[0] + pb[sd]) + (pb[2 * sd] + pb[3 * sd]);
            if (h >= 0) {
                const int hp = LD::hsp(T.HS);
                const double *q = pbuf() + LD::T1 * sd + h;
                for (int t = 0; t < C4 - LD::T1; t += 4)
                    s += (q[t * hp] + q[(t + 1) * hp]) + (q[(t + 2) * hp] + q[(t + 3) * hp]);
            }
        }
        return s;
    }
    // col_gather of the iteration loop in the DENSE instance: the same reads and sums from the
    // pass's own copy of the second tier's geometry (begin_pass)
    IMPC_WF double col_gather_pass(int v, int slot) {
        static_assert(LD::T1 == 4, "one first-tier group");
        const double *pb = pbuf() + v;
        constexpr int sd = LD::stride(13 * (WF + 1) - 5);
        double s = 0.0;
        s += (pb[0] + pb[sd]) + (pb[2 * sd] + pb[3 * sd]);
        if (ps_.hq[slot] >= 0) {
            const int hp = ps_.hp;
            const double *q = pbuf() + ps_.hq[slot];
            for (int t = 0; t < c4_ - LD::T1; t += 4)
                s += (q[t * hp] + q[(t + 1) * hp]) + (q[(t + 2) * hp] + q[(t + 3) * hp]);
        }
        return s;
    }
    IMPC_WF double col_gather_max(int v, int h) {
        const double *pb = pbuf() + v;
        const int C4 = c4_, sd = sd_;
        double s = 0.0;
        for (int t = 0; t < (TIER ? LD::T1 : C4); t++) s = dmax(pb[t * sd], s);
        if (TIER && h >= 0) {
            const int hp = LD::hsp(T.HS);
            const double *q = pbuf() + LD::T1 * sd + h;
            for (int t = 0; t < C4 - LD::T1; t++) s = dmax(q[t * hp], s);
        }
        return s;
    }

    // scale_data (scaling.h:21): Ruiz equilibration + cost scaling; D, E kept in registers here,
    // written to the per-QP scratch at the end.
    // ps: the QP's persistent record (or null): the Ruiz passes' cost factors are stored there,
    // or replayed from it when resuming
    IMPC_WF void scale(int64_t b, double D[VS], double Eb[VS], double Eg[GS], double *ps) {
        const int n = T.n;
        _Pragma("unroll") for (int s = 0; s < VS; s++) D[s] = Eb[s] = 1.0;
        _Pragma("unroll") for (int s = 0; s < GS; s++) Eg[s] = 1.0;
        c = 1.0;
        double *pb = pbuf(), *xb = xbuf();
        // |A| entries of the general rows -> products buffer: pass 0's here, each later pass's at
        // the end of the pass before (after its scaling), ordered by that pass's team reduction
        if (st.scaling > 0) {
            _Pragma("unroll") for (int s = 0; s < GS; s++) {
                if (gok[s])
                    _Pragma("unroll") for (int e = 0; e < 4; e++) pb[gdst(s, e)] = fabs(a[s][e]);
            }
            wv.sync();
        }
        for (int it = 0; it < st.scaling; it++) {
            double Dt[VS], Etb[VS], Etg[GS];
            _Pragma("unroll") for (int s = 0; s < VS; s++) {
                // colnorm_sym(P) (diagonal), max with colnorm(A) = max(box, general entries)
                double d = fabs(pd[s]);
                double an = dmax(fabs(ab[s]), 0.0);
                if (vok[s]) an = dmax(col_gather_max(NL * s + L, hid_[s]), an);
                d = dmax(d, an);
                d = d < kMinScaling ? 1.0 : d;
                d = d > kMaxScaling ? kMaxScaling : d;
                Dt[s] = 1.0 / sqrt(d);
                double e = fabs(ab[s]);
                e = e < kMinScaling ? 1.0 : e;
                e = e > kMaxScaling ? kMaxScaling : e;
                Etb[s] = 1.0 / sqrt(e);
            }
            _Pragma("unroll") for (int s = 0; s < GS; s++) {
                double e = 0.0;
                _Pragma("unroll") for (int k = 0; k < 4; k++) e = dmax(fabs(a[s][k]), e);
                e = e < kMinScaling ? 1.0 : e;
                e = e > kMaxScaling ? kMaxScaling : e;
                Etg[s] = 1.0 / sqrt(e);
            }
            // D_temp of every column to LDS for the general rows
            _Pragma("unroll") for (int s = 0; s < VS; s++)
                if (vok[s]) xb[NL * s + L] = Dt[s];
            wv.sync();
            _Pragma("unroll") for (int s = 0; s < VS; s++) {
                pd[s] = (pd[s] * Dt[s]) * Dt[s];
                ab[s] = (ab[s] * Etb[s]) * Dt[s];
                q[s] = Dt[s] * q[s];
                D[s] = D[s] * Dt[s];
                Eb[s] = Eb[s] * Etb[s];
            }
            _Pragma("unroll") for (int s = 0; s < GS; s++) {
                _Pragma("unroll") for (int e = 0; e < 4; e++) a[s][e] = (a[s][e] * Etg[s]) * xb[gcol(s, e)];
                Eg[s] = Eg[s] * Etg[s];
            }
            // the next pass's |A| (every read of this pass's came before the D_temp barrier)
            if (it + 1 < st.scaling)
                _Pragma("unroll") for (int s = 0; s < GS; s++) {
                    if (gok[s])
                        _Pragma("unroll") for (int e = 0; e < 4; e++) pb[gdst(s, e)] = fabs(a[s][e]);
                }
            // cost normalisation
            double psum = 0.0, qn = 0.0;
            _Pragma("unroll") for (int s = 0; s < VS; s++) {
                if (vok[s]) {
                    psum += fabs(pd[s]);
                    qn = dmax(fabs(q[s]), qn);
                }
            }
            // both cost norms in one team reduction (the same combine orders as sum / max; its
            // barriers also order this pass's reads of pb / xb before the next pass's writes)
            double mx1[1] = {qn}, sm1[1] = {psum};
            wv.max_sum_n(mx1, sm1);
            double ct = sm1[0] / (double)n;
            qn = mx1[0];
            qn = qn < kMinScaling ? 1.0 : qn;
            qn = qn > kMaxScaling ? kMaxScaling : qn;
            ct = dmax(ct, qn);
            ct = ct < kMinScaling ? 1.0 : ct;
            ct = ct > kMaxScaling ? kMaxScaling : ct;
            ct = 1. / ct;
            if (ps) {
                if (io.resume == 1)  // replay; resume 2 (new P / A: osqp_update_P / _A) scales afresh
                    ct = ps[it];
                else if (L == 0)
                    ps[it] = ct;
            }
            _Pragma("unroll") for (int s = 0; s < VS; s++) {
                pd[s] *= ct;
                q[s] *= ct;
            }
            c *= ct;
        }
        c = wv.uniform(c);
        cinv = 1. / c;
        _Pragma("unroll") for (int s = 0; s < VS; s++) {
            lb[s] = Eb[s] * lb[s];
            ub[s] = Eb[s] * ub[s];
            bt[s] = row_type(lb[s], ub[s]);
        }
        _Pragma("unroll") for (int s = 0; s < GS; s++) {
            lg[s] = Eg[s] * lg[s];
            ug[s] = Eg[s] * ug[s];
            gt[s] = row_type(lg[s], ug[s]);
        }
        double *sc = scal(b);
        _Pragma("unroll") for (int s = 0; s < VS; s++)
            if (vok[s]) {
                sc[NL * s + L] = D[s];
                sc[T.n + NL * s + L] = Eb[s];
            }
        _Pragma("unroll") for (int s = 0; s < GS; s++)
            if (gok[s]) sc[2 * T.n + NL * s + L] = Eg[s];
    }

    // ------------------------------------------------------------ block factorisation
    // Returns 1 if a pivot is not positive (OSQP_NONCVX_ERROR).
    // the factorisation assembly's destination of slot r = L + NL u (0 <= r < kStageDests): the
    // identity, or (F3) slots 0..63 on the 8 x 8 Schur block M[i][j] (13 i + j, lane 8 i + j),
    // the rest in order over the other 209 (M rows 0..7 columns 8..12, M rows 8..12, then B)
    IMPC_WF static int stage_dest(int r) {
        if constexpr (F3) {
            if (r < 64) return 13 * (r >> 3) + (r & 7);
            const int c = r - 64;
            return c < 40 ? 13 * (c / 5) + 8 + c % 5 : 104 + (c - 40);
        }
        return r;
    }

    // Written for latency (round 5): the assembly codes loaded four at a time with the next stage's
    // ranges prefetched, the Gauss-Jordan steps' operands read at once, the 13-term products fully
    // unrolled.  The long shape's setup runs one team per CU, so these latencies are exposed: setup
    // 0.440 -> 0.358 ms per N = 40 QP against the round-4 loops, config 5's closed loop 626 -> 608 ms
    // per step (profiles/r05/exp_phase/README.md)
    IMPC_WF int factorize() {
        const int n = T.n, W = Wst(), N = W + 1;
        double *w = pbuf(), *rhog = pbuf() + 4 * T.mg, *diagx = lds + LD::DIAGX;
        double *A = lds + LD::FA, *Li = lds + LD::FL, *Ai = lds + LD::FI, *Bb = lds + LD::FB, *G = lds + LD::FG,
               *E = lds + LD::FE, *Fm = F();
        double e_reg = 0.0;  // F3: E_k-1[L >> 3][L & 7] (lanes < 64)
        _Pragma("unroll") for (int s = 0; s < GS; s++) {
            int g = NL * s + L;
            if (gok[s]) {
                _Pragma("unroll") for (int e = 0; e < 4; e++) w[4 * g + e] = a[s][e];
                rhog[g] = rhog_(s);
            }
        }
        _Pragma("unroll") for (int s = 0; s < VS; s++) {
            if (vok[s]) {
                double rb = rhob(s);
                diagx[NL * s + L] = (pd[s] + st.sigma) + rb * ab[s] * ab[s];
            }
        }
        wv.sync();
        int bad = 0;
        // the assembly program's range of each of this lane's destinations, one stage ahead (a
        // global load; the long shape runs one team per CU, so nothing hides its latency)
        constexpr int ND = (kStageDests + NL - 1) / NL;
        int32_t tp[ND][2];
        auto load_tp = [&](int k) {
            _Pragma("unroll") for (int u = 0; u < ND; u++) {
                const int d = stage_dest(L + NL * u);
                const bool ok = d < kStageDests && k < N;
                tp[u][0] = ok ? T.term_ptr[(int64_t)k * kStageDests + d] : 0;
                tp[u][1] = ok ? T.term_ptr[(int64_t)k * kStageDests + d + 1] : 0;
            }
        };
        load_tp(0);
        constexpr int kCodes = 4;  // assembly codes per batch
        for (int k = 0; k < N; k++) {
            const int sz = k < W ? 13 : 8;
            if constexpr (F3) Bb = lds + ((k & 1) ? LD::FB2 : LD::FB);
            // assemble M_kk and Bbar_k
            int32_t tc[ND][2];
            _Pragma("unroll") for (int u = 0; u < ND; u++) tc[u][0] = tp[u][0], tc[u][1] = tp[u][1];
            load_tp(k + 1);
            _Pragma("unroll") for (int u = 0; u < ND; u++) {
                if (L + NL * u >= kStageDests) continue;
                const int d = stage_dest(L + NL * u);
                const bool isB = d >= 169;
                if (isB && k == W) continue;
                const int dd = isB ? d - 169 : d;
                const int r = dd / 13, cc = dd % 13;
                double val = 0.0;
                if (isB || (r < sz && cc < sz)) {
                    // the codes four at a time, their LDS operands before the products (the sum
                    // keeps its term order)
                    const int32_t t0 = tc[u][0], t1 = tc[u][1];
                    for (int32_t t = t0; t < t1; t += kCodes) {
                        int32_t cd[kCodes];
                        _Pragma("unroll") for (int v = 0; v < kCodes; v++) cd[v] = t + v < t1 ? T.term[t + v] : 0;
                        double rg[kCodes], we[kCodes], wf[kCodes];
                        _Pragma("unroll") for (int v = 0; v < kCodes; v++) {
                            const int32_t g = cd[v] >> 4, e = (cd[v] >> 2) & 3, f = cd[v] & 3;
                            rg[v] = rhog[g];
                            we[v] = w[4 * g + e];
                            wf[v] = w[4 * g + f];
                        }
                        _Pragma("unroll") for (int v = 0; v < kCodes; v++)
                            if (t + v < t1) val += rg[v] * we[v] * wf[v];
                    }
                    if (!isB && r == cc) val += diagx[13 * k + r];
                    if (!isB && k > 0 && r < 8 && cc < 8)  // Schur complement (F3: this lane's E)
                        val -= F3 ? e_reg : E[8 * r + cc];
                }
                if (isB)
                    Bb[dd] = val;
                else
                    A[dd] = val;
            }
            wv.sync();
            IMPC_SEC(kSecFAsm);
            // Ahat_k^{-1} by Gauss-Jordan elimination: one element per lane, the pivots in order
            // (SPD, no pivoting needed; a non-positive-definite pivot flags the factorisation as
            // failed, as a failed Cholesky did), ping-pong between two LDS buffers so every step
            // is one barrier.  The last step writes the lower triangle to both halves of Ai
            // (exactly symmetric).
            {
                double *src = A, *dst = Li;
                // two pivots per step (2x2 block pivot Q = P^-1, P = S[J][J], J = {j, j+1}):
                //   D[J][J] = Q, D[J][c] = Q S[J][c], D[i][J] = -S[i][J] Q,
                //   D[i][c] = S[i][c] - (S[i][J] Q) S[J][c]; a non-PD pivot block flags failure
                for (int j = 0; j < sz; j += 2) {
                    const bool two = j + 1 < sz, last = j + (two ? 2 : 1) >= sz;
                    // element (gi, gc) of the 13 x 13 block per lane (a team of fewer than 169 lanes
                    // takes several)
                    for (int el = L; el < 169; el += NL) {
                        const int gi = el / 13, gc = el % 13;
                        if (gi >= sz || gc >= sz) continue;
                        const int i = last && gc > gi ? gc : gi, c = last && gc > gi ? gi : gc;
                        double v;
                        // every operand read at once (one LDS round trip per step), the lane's
                        // case selected after
                        const double p00 = src[13 * j + j], p01 = src[13 * j + (two ? j + 1 : j)];
                        const double p10 = src[13 * (two ? j + 1 : j) + j], p11 = src[13 * (two ? j + 1 : j) + (two ? j + 1 : j)];
                        const double s0 = src[13 * j + c], s1 = src[13 * (two ? j + 1 : j) + c];
                        const double a0 = src[13 * i + j], a1 = src[13 * i + (two ? j + 1 : j)];
                        const double sic = src[13 * i + c];
                        if (two) {
                            const double det = p00 * p11 - p01 * p10;
                            if (!(p00 > 0.0) || !(det > 0.0)) bad = 1;
                            const double rd = 1.0 / det;
                            const double q00 = p11 * rd, q01 = -(p01 * rd), q10 = -(p10 * rd), q11 = p00 * rd;
                            const int ri = i - j, ci = c - j;
                            const bool iJ = ri == 0 || ri == 1, cJ = ci == 0 || ci == 1;
                            const double vq = ri == 0 ? (ci == 0 ? q00 : q01) : (ci == 0 ? q10 : q11);
                            const double vr = ri == 0 ? q00 * s0 + q01 * s1 : q10 * s0 + q11 * s1;
                            const double u0 = a0 * q00 + a1 * q10, u1 = a0 * q01 + a1 * q11;
                            const double vc = -(ci == 0 ? u0 : u1);
                            const double vi = sic - (u0 * s0 + u1 * s1);
                            v = iJ ? (cJ ? vq : vr) : (cJ ? vc : vi);
                        } else {
                            if (!(p00 > 0.0)) bad = 1;
                            const double r = 1.0 / p00;
                            v = i == j ? (c == j ? r : s0 * r) : (c == j ? -(a0 * r) : sic - (a0 * r) * s0);
                        }
                        (last ? Ai : dst)[13 * gi + gc] = v;
                    }
                    wv.sync();
                    double *t = src;
                    src = dst;
                    dst = t;
                }
            }
            _Pragma("unroll") for (int s = 0; s < VS; s++)
                if (vok[s] && vs_[s] == k)
                    _Pragma("unroll") for (int cc = 0; cc < 13; cc++) ainv[s][cc] = cc < sz ? Ai[13 * vr_[s] + cc] : 0.0;
            if (k < W) {
                for (int p = L; p < 104; p += NL) {
                    int i = p / 13, cc = p % 13;
                    double s = 0.0;
                    _Pragma("unroll") for (int t = 0; t < 13; t++) s += Bb[13 * i + t] * Ai[13 * t + cc];
                    G[p] = s;
                }
                wv.sync();
                if (L < 64) {
                    int i = L >> 3, j = L & 7;
                    double s = 0.0;
                    _Pragma("unroll") for (int t = 0; t < 13; t++) s += G[13 * i + t] * Bb[13 * j + t];
                    if constexpr (F3)
                        e_reg = s;
                    else
                        E[8 * i + j] = s;
                    // recursion layout: lane (i,j) of step k reads F_k[j][i] when the column index
                    // sits on i (k even), F_k[i][j] otherwise (mfmap::f_slot); stored negated, so a
                    // recursion step is c + (-F) v in one fma or one matrix instruction
                    Fm[64 * k + 8 * i + j] = -(!(k & 1) ? G[13 * j + i] : G[13 * i + j]);
                }
                _Pragma("unroll") for (int s = 0; s < VS; s++) {
                    if (!vok[s]) continue;
                    if (vs_[s] == k && vr_[s] >= 8)
                        _Pragma("unroll") for (int j = 0; j < 8; j++) cp[s][j] = G[13 * j + vr_[s]];
                    if (vs_[s] == k + 1 && vr_[s] < 8)
                        _Pragma("unroll") for (int j = 0; j < 8; j++) cp[s][j] = j < 5 ? G[13 * vr_[s] + 8 + j] : 0.0;
                }
                if constexpr (!F3) wv.sync();
            }
            IMPC_SEC(kSecFDense);
        }
        _Pragma("unroll") for (int s = 0; s < VS; s++)
            if (vok[s] && vs_[s] == 0 && vr_[s] < 8)
                _Pragma("unroll") for (int j = 0; j < 8; j++) cp[s][j] = 0.0;
        if constexpr (CHUNK) chunk_ops();
        bad = (int)wv.max((double)bad);  // set by lane 0 only: team-wide, so every wavefront agrees
        clear_exchange();
        zero_products();  // the (4g + e) factorisation scratch shared the products region
        (void)n;
        return bad;
    }

    // F_k[r][c] from the recursion layout (factorize stores -F_k, even stages' blocks transposed)
    IMPC_WF static double f_el(const double *Fm, int k, int r, int c) {
        return -(!(k & 1) ? Fm[64 * k + 8 * c + r] : Fm[64 * k + 8 * r + c]);  // mfmap::f_slot
    }

    // P = the product of one chunk's step operators on one wavefront (lane (i, j) holds P[i][j]):
    // forward steps o..o+CL-1, P <- -F_k P with k ascending; backward steps o+CL-1..o, P <- -F_k^T P
    // with k descending
    IMPC_WF void chunk_prod(bool fwd, int o, double *P, int l) {
        const double *Fm = F();
        const int i = l >> 3, j = l & 7;
        P[l] = i == j ? 1.0 : 0.0;
        wv.wsync();
        for (int s = 0; s < CL; s++) {
            const int k = fwd ? o + s : o + CL - 1 - s;
            double pc[8];
            _Pragma("unroll") for (int m = 0; m < 8; m++) pc[m] = P[8 * m + j];
            double v = 0.0;
            _Pragma("unroll") for (int m = 0; m < 8; m++) v -= (fwd ? f_el(Fm, k, i, m) : f_el(Fm, k, m, i)) * pc[m];
            wv.wsync();
            P[l] = v;
            wv.wsync();
        }
    }
    IMPC_WF static void mat8(const double *A, const double *B, double *out, int l) {  // out = A B
        const int i = l >> 3, j = l & 7;
        double v = 0.0;
        _Pragma("unroll") for (int m = 0; m < 8; m++) v += A[8 * i + m] * B[8 * m + j];
        out[l] = v;
    }
    // The chunk operators (CHUNK): forward chunks c = 1..3 start at c CL; backward chunks c = 1..3 (in
    // sweep order) cover steps (5 - c) CL - 1 .. (4 - c) CL.  Six chunk products on four wavefronts,
    // then the two-chunk products, then the three-chunk ones.
    IMPC_WF void chunk_ops() {
        double *C = chbuf(), *Bk = C + kChB;
        const int w = L >> 6, l = L & 63;
        if (w < 3)
            chunk_prod(true, (w + 1) * CL, C + kChP1 + 64 * w, l);
        else
            chunk_prod(false, 3 * CL, Bk + kChP1, l);
        if (w < 2) chunk_prod(false, (2 - w) * CL, Bk + kChP2 + 64 * w, l);
        wv.sync();
        // w 0 / 1: forward P2 P1 / P3 P2; w 2 / 3: backward P2 P1 / P3 P2
        double *X = w < 2 ? C : Bk;
        mat8(X + kChP2 + 64 * (w & 1), X + kChP1 + 64 * (w & 1), X + kChP21 + 64 * (w & 1), l);
        wv.sync();
        if (w < 2) {  // w 0: forward P3 P2 P1, w 1: backward
            double *Y = w ? Bk : C;
            mat8(Y + kChP3, Y + kChP21, Y + kChP321, l);
        }
        wv.sync();
    }

    // One step of a stage recursion on the 8x8 lane grid: returns c - F v as R(c / 8 + nf v), R the
    // strided (STRIDE) or contiguous 8-lane sum and nf the stored -F element.  The sweeps' inputs c
    // come pre-scaled by kSweepPre = 1/8 (exact: S1 stores t / 8, S3 the state part of e / 8), so the
    // subtraction rides in the product's FMA: one instruction and one dependent operation less per
    // step on the serial chain.  (The matrix-instruction form, sweep_mfma, reads the same inputs.)
    static constexpr double kSweepPre = 0.125;
    template <bool STRIDE>
    IMPC_WF double rstep(double nf, double c8, double v) {
        const double p = __builtin_fma(nf, v, c8);
        return STRIDE ? wv.sum_stride8(p) : wv.sum_contig8(p);
    }

    // Sweeps with a compile-time step count WC (= WSPEC) are fully unrolled: every LDS wait is
    // exact and the step results stay in registers until the sweep ends, instead of an LDS store
    // per step whose completion the next step's wait would include (measured 195 -> 157 cycles
    // per step, tools/probe/recur_probe.hip).  Step m's result sits in the 8 lanes sharing its
    // output index; of those the lane whose other index is (m/2) mod 8 keeps it, in slot m/16 of
    // the even- or odd-step array (a compile-time lane mask, one v_cndmask pair per step).
    static constexpr int CQ = LD::WSPEC / 16 + 1;
    IMPC_WF static void cap(double (&c)[CQ], double r, int m, int other) {
        if (((m >> 1) & 7) == other) c[m >> 4] = r;
    }
    // cap with the lane test as a compile-time lane mask (OI: `other` is the lane's i = l >> 3, else
    // j = l & 7; lane l = 8 i + j of the recursion wavefront): the select by that constant mask in
    // an SGPR pair instead of a v_cmp per step (the CPU emulation takes the plain test)
    template <bool OI>
    IMPC_WF static void capm(double (&c)[CQ], double r, int m, int other) {
#if defined(__HIP_DEVICE_COMPILE__)
        (void)other;
        const int v = (m >> 1) & 7;
        const uint64_t msk = OI ? (0xFFull << (8 * v)) : (0x0101010101010101ull << v);
        double &d = c[m >> 4];
        int lo = __double2loint(d), hi = __double2hiint(d);
        asm("v_cndmask_b32 %0, %0, %1, %2" : "+v"(lo) : "v"(__double2loint(r)), "s"(msk));
        asm("v_cndmask_b32 %0, %0, %1, %2" : "+v"(hi) : "v"(__double2hiint(r)), "s"(msk));
        d = __hiloint2double(hi, lo);
#else
        cap(c, r, m, other);
#endif
    }
    // Store a sweep's W captured steps: even steps' outputs sit at index j (EJ) or i, odd steps'
    // at the other; step m is stage m + 1 (forward) or W - 1 - m (backward).
    template <bool EJ>
    IMPC_WF static void cap_store(const double (&c0)[CQ], const double (&c1)[CQ], double *buf, int W, bool fwd,
                                  int i, int j) {
        const int o0 = EJ ? i : j, e0 = EJ ? j : i;
        _Pragma("unroll") for (int q = 0; q < CQ; q++) {
            const int m0 = 16 * q + 2 * o0, m1 = 16 * q + 2 * e0 + 1;
            if (m0 < W) buf[13 * (fwd ? m0 + 1 : W - 1 - m0) + e0] = c0[q];
            if (m1 < W) buf[13 * (fwd ? m1 + 1 : W - 1 - m1) + o0] = c1[q];
        }
    }

    // The default horizon's sweep (W = 19) in device code runs in two parts, sweep_pro / sweep_run
    // below (round 12; profiles/r12/kernel_ab.txt): the prologue in front of the releasing barrier
    // took config 3 from 145.7-146.3 to 143.9-144.0 ms per launch, the early stores with it to
    // 142.2-142.4 (early stores without the prologue form the store addresses between the steps and
    // measured slower than the form without either, 147.3-147.4).  The long shape's runtime-W instance keeps its
    // W = 39 sweep whole (sweep_mfma).
#if defined(__HIP_DEVICE_COMPILE__)
    static constexpr bool kSweep19 = !CHUNK && LD::WSPEC == 19;

    // The matrix-instruction sweeps (device code only; the CPU emulation keeps the 8x8 lane grid).
    // The select of capm by a lane mask given as a constant (mfmap::keep_mask)
    IMPC_WF static void capk(double &d, double r, uint64_t msk) {
        int lo = __double2loint(d), hi = __double2hiint(d);
        asm("v_cndmask_b32 %0, %0, %1, %2" : "+v"(lo) : "v"(__double2loint(r)), "s"(msk));
        asm("v_cndmask_b32 %0, %0, %1, %2" : "+v"(hi) : "v"(__double2hiint(r)), "s"(msk));
        d = __hiloint2double(hi, lo);
    }
    // A fully unrolled sweep of WC steps on v_mfma_f64_4x4x4_4b_f64 (sweep_mfma_map.hpp: layout, block
    // numbering, why no transpose sits on the chain).  FWD: a_{k+1} = t_{k+1} - F_k a_k, step m is
    // stage k = m and produces stage m + 1; else x_k = e_k - F_k' x_{k+1}, step m is stage
    // k = WC - 1 - m.  A step is the instruction (A the stored -F_k element of the lane's block, B the
    // running vector, C the input c), one DPP move of the partner block's D and one add.  cb holds
    // c * kSweepPre = c / 8 and both blocks of a row add it, so the chain runs in units of
    // 2 kSweepPre = 1/4: v / 4 = 2 (c / 8) - F (v / 4), exact, and the captured steps are scaled back
    // when they are stored (sweep_run).  (Keeping F's sign and negating every other step's c
    // instead was measured: 182.4-182.7 ms per config-3 launch against 171.8-171.9 for this form
    // and the parent's 184.0, profiles/r09/kernel_ab.txt.)  The per-lane offsets come from the opaque
    // lane index here, not from outside the ADMM loop.
    // Capture as on the lane grid, the select pair behind the step's own add: behind the next step's
    // instruction, inside its wait states, it was measured slower, as was a read distance of three
    // (profiles/r11/).  What the sweep does around its steps is kept short instead: (F, c) are read
    // kSweepAhead steps ahead and only for steps that exist (no read past stage WC - 1 of F or stage
    // WC of cb, none repeated), the first step kept in a capture register is a plain copy (the other
    // lanes' content is overwritten by their own steps or never stored), and the stores after the
    // last step have no divergent branch.
    static constexpr int kSweepAhead = 2;
    template <int WC, bool FWD>
    IMPC_WF void sweep_mfma(const double *cb, double *ob) {
        constexpr int PD = kSweepAhead;
        static_assert(PD >= 1 && PD <= WC, "the (F, c) ring is filled from existing steps only");
        const double *Fm = lds + LD::F_OFF;
        const int lo = lane_o(), l = lo & 63;
        constexpr int k0 = FWD ? 0 : WC - 1, k1 = FWD ? 1 : WC - 2;  // stages of steps 0, 1
        const int fs[2] = {mfmap::a_slot(l, false, FWD, !(k0 & 1)), mfmap::a_slot(l, true, FWD, !(k1 & 1))};
        const int os[2] = {mfmap::out_idx(l, false), mfmap::out_idx(l, true)};
        auto fst = [](int m) { return 64 * (FWD ? m : WC - 1 - m); };       // m < WC
        auto cst = [](int m) { return 13 * (FWD ? m + 1 : WC - 1 - m); };   // m < WC
        double v = 2.0 * cb[13 * (FWD ? 0 : WC) + mfmap::in_idx(l, false)];  // (c / 8) (1/4) / (1/8)
        double fq[PD], cq[PD];
        _Pragma("unroll") for (int p = 0; p < PD; p++) fq[p] = Fm[fst(p) + fs[p & 1]], cq[p] = cb[cst(p) + os[p & 1]];
        double c0[CQ], c1[CQ];
        _Pragma("unroll") for (int m = 0; m < WC; m++) {
            const double f0 = fq[m % PD], e0 = cq[m % PD];
            if (m + PD < WC) {
                fq[m % PD] = Fm[fst(m + PD) + fs[(m + PD) & 1]];
                cq[m % PD] = cb[cst(m + PD) + os[(m + PD) & 1]];
            }
            v = (m & 1) ? wv.template mfma_step<true>(f0, e0, v) : wv.template mfma_step<false>(f0, e0, v);
            double &c = (m & 1) ? c1[m >> 4] : c0[m >> 4];
            if ((m & 14) == 0) c = v;  // the register's first step
            else capk(c, v, mfmap::keep_mask((m >> 1) & 7, m & 1));
        }
        _Pragma("unroll") for (int q = 0; q < CQ; q++) {  // registers no step of this WC reaches
            if (16 * q >= WC) c0[q] = 0.0;
            if (16 * q + 1 >= WC) c1[q] = 0.0;
        }
        // one lane per element stores, the others write their discard slot
        const int he = mfmap::other(l, false), ho = mfmap::other(l, true);
        constexpr double back = 1.0 / (2.0 * kSweepPre);
        double *junk = lds + LD::JUNK_OFF + lo;
        _Pragma("unroll") for (int q = 0; q < CQ; q++) {
            const int m0 = 16 * q + 2 * he, m1 = 16 * q + 2 * ho + 1;
            *(m0 < WC ? ob + 13 * (FWD ? m0 + 1 : WC - 1 - m0) + os[0] : junk) = back * c0[q];
            *(m1 < WC ? ob + 13 * (FWD ? m1 + 1 : WC - 1 - m1) + os[1] : junk) = back * c1[q];
        }
    }
    // The default horizon's sweep in two parts (kSweep19; the same reads, steps, values and stores as
    // sweep_mfma).  sweep_pro is what depends on neither cb's nor ob's content: the lane's F slots and
    // c indices by step parity, its element of the start vector, where it stores capture register q of
    // the even (s0) / odd (s1) steps -- the element it owns or its discard slot -- and the first
    // kSweepAhead F reads (F is constant across an iteration; factorize() rewrites it behind barriers
    // of its own).  iterate() has the sweeping wavefront form it in front of the barrier that releases
    // the sweep, where the other wavefronts' arrival covers it; from the opaque lane index inside the
    // iteration, as before.
    struct SweepPro {
        int lo, fs[2], os[2], in;
        double *s0[CQ], *s1[CQ];
        double fq[kSweepAhead];
    };
    template <int WC, bool FWD>
    IMPC_WF void sweep_stores(SweepPro &p, double *ob) {
        // one lane per element stores, the others write their discard slot
        const int l = p.lo & 63, he = mfmap::other(l, false), ho = mfmap::other(l, true);
        double *junk = lds + LD::JUNK_OFF + p.lo;
        _Pragma("unroll") for (int q = 0; q < CQ; q++) {
            const int m0 = mfmap::cap_step(q, false, he), m1 = mfmap::cap_step(q, true, ho);
            p.s0[q] = m0 < WC ? ob + 13 * (FWD ? m0 + 1 : WC - 1 - m0) + p.os[0] : junk;
            p.s1[q] = m1 < WC ? ob + 13 * (FWD ? m1 + 1 : WC - 1 - m1) + p.os[1] : junk;
        }
    }
    template <int WC, bool FWD>
    IMPC_WF void sweep_pro(SweepPro &p, double *ob) {
        const double *Fm = lds + LD::F_OFF;
        p.lo = lane_o();
        const int l = p.lo & 63;
        constexpr int k0 = FWD ? 0 : WC - 1, k1 = FWD ? 1 : WC - 2;  // stages of steps 0, 1
        p.fs[0] = mfmap::a_slot(l, false, FWD, !(k0 & 1)), p.fs[1] = mfmap::a_slot(l, true, FWD, !(k1 & 1));
        p.os[0] = mfmap::out_idx(l, false), p.os[1] = mfmap::out_idx(l, true);
        p.in = mfmap::in_idx(l, false);
        _Pragma("unroll") for (int q = 0; q < kSweepAhead; q++)
            p.fq[q] = Fm[64 * (FWD ? q : WC - 1 - q) + p.fs[q & 1]];
        sweep_stores<WC, FWD>(p, ob);
    }
    // The steps behind the barrier.  Each capture register is scaled back and stored
    // behind the last step that writes it (mfmap::cap_final: c0[0] / c1[0] go out during steps 15-18),
    // so only the last steps' registers are left when the sweep ends.
    template <int WC, bool FWD>
    IMPC_WF void sweep_run(const SweepPro &p, const double *cb) {
        constexpr int PD = kSweepAhead;
        static_assert(PD >= 1 && PD <= WC, "the (F, c) ring is filled from existing steps only");
        const double *Fm = lds + LD::F_OFF;
        auto fst = [](int m) { return 64 * (FWD ? m : WC - 1 - m); };       // m < WC
        auto cst = [](int m) { return 13 * (FWD ? m + 1 : WC - 1 - m); };   // m < WC
        constexpr double back = 1.0 / (2.0 * kSweepPre);
        double v = 2.0 * cb[13 * (FWD ? 0 : WC) + p.in];  // (c / 8) (1/4) / (1/8)
        double fq[PD], cq[PD];
        _Pragma("unroll") for (int q = 0; q < PD; q++) fq[q] = p.fq[q], cq[q] = cb[cst(q) + p.os[q & 1]];
        double c0[CQ], c1[CQ];
        _Pragma("unroll") for (int m = 0; m < WC; m++) {
            const double f0 = fq[m % PD], e0 = cq[m % PD];
            if (m + PD < WC) {
                fq[m % PD] = Fm[fst(m + PD) + p.fs[(m + PD) & 1]];
                cq[m % PD] = cb[cst(m + PD) + p.os[(m + PD) & 1]];
            }
            v = (m & 1) ? wv.template mfma_step<true>(f0, e0, v) : wv.template mfma_step<false>(f0, e0, v);
            double &c = (m & 1) ? c1[m >> 4] : c0[m >> 4];
            if ((m & 14) == 0) c = v;  // the register's first step
            else capk(c, v, mfmap::keep_mask((m >> 1) & 7, m & 1));
            if (m == mfmap::cap_final(WC, m >> 4, m & 1)) *((m & 1) ? p.s1[m >> 4] : p.s0[m >> 4]) = back * c;
        }
        _Pragma("unroll") for (int q = 0; q < CQ; q++) {  // registers no step of this WC reaches
            if (16 * q >= WC) c0[q] = 0.0;
            if (16 * q + 1 >= WC) c1[q] = 0.0;
        }
        _Pragma("unroll") for (int q = 0; q < CQ; q++) {
            if (mfmap::cap_final(WC, q, false) < 0) *p.s0[q] = back * c0[q];
            if (mfmap::cap_final(WC, q, true) < 0) *p.s1[q] = back * c1[q];
        }
    }
#endif

    // Forward steps o .. o + WC - 1 (o even) from a_o = a at index i, fully unrolled: the results
    // a_{o+1} .. a_{o+WC} stored to rb when CAP, the last one returned (every lane (i, j) holds
    // a_{o+WC}[i] or [j] by its parity).
    template <int WC, bool CAP>
    IMPC_WF double fwd_run(const double *tb, double *rb, int o, double a) {
        const double *Fm = lds + LD::F_OFF + 64 * o;
        tb += 13 * o;
        const int lo = lane_o(), l = lo & 63, i = l >> 3, j = l & 7;  // opaque: see lane_o
        // (F, t) of the next even / odd step, loaded two steps ahead (reads past the last stage
        // stay inside the LDS buffers and are never used)
        double fe = Fm[l], te = tb[13 + j], fo = Fm[64 + l], to = tb[26 + i];
        double c0[CQ], c1[CQ];
        _Pragma("unroll") for (int q = 0; q < CQ; q++) c0[q] = c1[q] = 0.0;
        _Pragma("unroll") for (int k = 0; k < WC; k += 2) {
            const double f0 = fe, t0 = te;
            fe = Fm[64 * (k + 2) + l];
            te = tb[13 * (k + 3) + j];
            a = rstep<true>(f0, t0, a);
            if constexpr (CAP) capm<true>(c0, a, k, i);
            if (k + 1 < WC) {
                const double f1 = fo, t1 = to;
                fo = Fm[64 * (k + 3) + l];
                to = tb[13 * (k + 4) + i];
                a = rstep<false>(f1, t1, a);
                if constexpr (CAP) capm<false>(c1, a, k + 1, j);
            }
        }
        if constexpr (CAP) cap_store<true>(c0, c1, rb + 13 * o, WC, true, i, j);
        return a;
    }

    // S2 body: a_{k+1} = t_{k+1} - F_k a_k for k = 0..W-1 (WC = W, or 0 for a runtime W).
    template <int WC>
    IMPC_WF void fwd_sweep(const double *tb, double *rb, int W) {
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (WC > 0) return sweep_mfma<WC, true>(tb, rb);
#endif
        const double *Fm = lds + LD::F_OFF;
        const int lo = lane_o(), l = lo & 63, i = l >> 3, j = l & 7;  // opaque: see lane_o
        double a = (1.0 / kSweepPre) * tb[i];  // a_0 = t_0 (tb holds t / 8)
        if constexpr (WC > 0) {
            (void)fwd_run<WC, true>(tb, rb, 0, a);
        } else {
            // (F, t) of the next even / odd step, loaded two steps ahead (reads past the last stage
            // stay inside the LDS buffers and are never used)
            double fe = Fm[l], te = tb[13 + j], fo = Fm[64 + l], to = tb[26 + i];
            // one lane per element writes, the rest write to discard slots (no divergent branch)
            double *junk = lds + LD::JUNK_OFF + lo;
            const bool wri = j == 0, wrj = i == 0;
            for (int k = 0; k < W; k += 2) {
                const double f0 = fe, t0 = te;
                fe = Fm[64 * (k + 2) + l];
                te = tb[13 * (k + 3) + j];
                a = rstep<true>(f0, t0, a);
                *(wrj ? rb + 13 * (k + 1) + j : junk) = a;
                if (k + 1 >= W) break;
                const double f1 = fo, t1 = to;
                fo = Fm[64 * (k + 3) + l];
                to = tb[13 * (k + 4) + i];
                a = rstep<false>(f1, t1, a);
                *(wri ? rb + 13 * (k + 2) + i : junk) = a;
            }
        }
    }

    // Backward steps o + WC - 1 .. o (o even, the first of parity ODD) from x_{o+WC} = x, fully
    // unrolled: x_{o+WC-1} .. x_o stored to xb when CAP, x_o returned.
    template <bool ODD, int WC, bool CAP>
    IMPC_WF double bwd_run(const double *eb, double *xb, int o, double x) {
        const double *Fm = lds + LD::F_OFF + 64 * o;
        eb += 13 * o;
        const int lo = lane_o(), l = lo & 63, i = l >> 3, j = l & 7;
        constexpr int k1 = WC - 2 > 0 ? WC - 2 : 0;
        double fa = Fm[64 * (WC - 1) + l], ea = eb[13 * (WC - 1) + (ODD ? j : i)];
        double fb = Fm[64 * k1 + l], ebv = eb[13 * k1 + (ODD ? i : j)];
        double c0[CQ], c1[CQ];
        _Pragma("unroll") for (int q = 0; q < CQ; q++) c0[q] = c1[q] = 0.0;
        _Pragma("unroll") for (int m = 0; m < WC; m += 2) {
            const int k = WC - 1 - m;
            const int k2 = k - 2 > 0 ? k - 2 : 0, k3 = k - 3 > 0 ? k - 3 : 0;
            const double f0 = fa, e0 = ea;
            fa = Fm[64 * k2 + l];
            ea = eb[13 * k2 + (ODD ? j : i)];
            x = rstep<ODD>(f0, e0, x);
            if constexpr (CAP) capm<ODD>(c0, x, m, ODD ? i : j);
            if (m + 1 < WC) {
                const double f1 = fb, e1 = ebv;
                fb = Fm[64 * k3 + l];
                ebv = eb[13 * k3 + (ODD ? i : j)];
                x = rstep<!ODD>(f1, e1, x);
                if constexpr (CAP) capm<!ODD>(c1, x, m + 1, ODD ? j : i);
            }
        }
        if constexpr (CAP) cap_store<ODD>(c0, c1, xb + 13 * o, WC, false, i, j);
        return x;
    }

    // S4 body for a first step k = W-1 of parity ODD: steps alternate strided (odd k) and
    // contiguous (even k) reductions; x_k sits at index j (odd k) / i (even k).  WC as above.
    template <bool ODD, int WC>
    IMPC_WF void bwd_sweep(const double *eb, double *xb, int W) {
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (WC > 0) return sweep_mfma<WC, false>(eb, xb);
#endif
        const double *Fm = lds + LD::F_OFF;
        const int lo = lane_o(), l = lo & 63, i = l >> 3, j = l & 7;
        if constexpr (WC > 0) W = WC;
        // x_W = e_W: W = (W-1)+1 has the opposite parity of the first step (eb holds e[:8] / 8)
        double x = (1.0 / kSweepPre) * eb[13 * W + (ODD ? i : j)];
        if constexpr (WC > 0) {
            (void)bwd_run<ODD, WC, true>(eb, xb, 0, x);
        } else {
            const int k1 = W - 2 > 0 ? W - 2 : 0;
            double fa = Fm[64 * (W - 1) + l], ea = eb[13 * (W - 1) + (ODD ? j : i)];
            double fb = Fm[64 * k1 + l], ebv = eb[13 * k1 + (ODD ? i : j)];
            double *junk = lds + LD::JUNK_OFF + lo;
            const bool wri = j == 0, wrj = i == 0;
            for (int k = W - 1; k >= 0; k -= 2) {
                const int k2 = k - 2 > 0 ? k - 2 : 0, k3 = k - 3 > 0 ? k - 3 : 0;
                const double f0 = fa, e0 = ea;
                fa = Fm[64 * k2 + l];
                ea = eb[13 * k2 + (ODD ? j : i)];
                x = rstep<ODD>(f0, e0, x);
                *(ODD ? (wrj ? xb + 13 * k + j : junk) : (wri ? xb + 13 * k + i : junk)) = x;
                if (k - 1 < 0) break;
                const double f1 = fb, e1 = ebv;
                fb = Fm[64 * k3 + l];
                ebv = eb[13 * k3 + (ODD ? i : j)];
                x = rstep<!ODD>(f1, e1, x);
                *(ODD ? (wri ? xb + 13 * (k - 1) + i : junk) : (wrj ? xb + 13 * (k - 1) + j : junk)) = x;
            }
        }
    }

    // S2 in chunks (CHUNK; see CH_OFF): steps c CL .. c CL + CL - 1 (c = 0..3) and 4 CL .. W - 1; waves
    // 1..3 run chunks 1..3 twice, wave 0 chunk 0 in round 1 and chunk 4 in round 2.
    IMPC_WF void fwd_chunked(const double *tb, double *rb) {
        const double *C = chbuf();
        double *ends = chbuf() + kChEnd;
        const int w = L >> 6, l = lane_o() & 63, i = l >> 3, j = l & 7;
        constexpr int A1 = 13 * CL;  // a_CL in rb (even stage: index i)
        if (w == 0) {
            (void)fwd_run<CL, true>(tb, rb, 0, 8.0 * tb[i]);  // a_0 = t_0 (tb holds t / 8)
        } else {
            const double e = fwd_run<CL, false>(tb, rb, w * CL, 0.0);
            if (j == 0) ends[8 * (w - 1) + i] = e;
        }
        wv.lsync();
        if (w == 1) {
            (void)fwd_run<CL, true>(tb, rb, CL, rb[A1 + i]);
        } else if (w == 2) {
            const double a = wv.sum_contig8(__builtin_fma(C[kChP1 + l], rb[A1 + j], 0.125 * ends[i]));
            (void)fwd_run<CL, true>(tb, rb, 2 * CL, a);
        } else if (w == 3) {
            const double p = __builtin_fma(C[kChP2 + l], ends[j],
                                           __builtin_fma(C[kChP21 + l], rb[A1 + j], 0.125 * ends[8 + i]));
            (void)fwd_run<CL, true>(tb, rb, 3 * CL, wv.sum_contig8(p));
        } else {
            const double p = __builtin_fma(
                C[kChP3 + l], ends[8 + j],
                __builtin_fma(C[kChP32 + l], ends[j], __builtin_fma(C[kChP321 + l], rb[A1 + j], 0.125 * ends[16 + i])));
            (void)fwd_run<CLAST, true>(tb, rb, 4 * CL, wv.sum_contig8(p));
        }
    }

    // S4 in chunks: steps W-1..4CL (wave 0, round 1, from x_W), 4CL-1..3CL / 3CL-1..2CL /
    // 2CL-1..CL (waves 1..3, both rounds), CL-1..0 (wave 0, round 2).
    IMPC_WF void bwd_chunked(const double *eb, double *xb) {
        const double *C = chbuf() + kChB;
        double *ends = chbuf() + kChEnd + kChEnds;
        const int w = L >> 6, l = lane_o() & 63, i = l >> 3, j = l & 7;
        constexpr int X4 = 13 * 4 * CL;      // x_4CL in xb (even stage: index i)
        constexpr bool LODD = (WF - 1) & 1;  // parity of the first chunk's first step W - 1
        if (w == 0) {
            (void)bwd_run<LODD, CLAST, true>(eb, xb, 4 * CL, 8.0 * eb[13 * WF + (LODD ? i : j)]);
        } else {
            const double e = bwd_run<true, CL, false>(eb, xb, (4 - w) * CL, 0.0);
            if (j == 0) ends[8 * (w - 1) + i] = e;
        }
        wv.lsync();
        if (w == 1) {
            (void)bwd_run<true, CL, true>(eb, xb, 3 * CL, xb[X4 + i]);
        } else if (w == 2) {
            const double x = wv.sum_contig8(__builtin_fma(C[kChP1 + l], xb[X4 + j], 0.125 * ends[i]));
            (void)bwd_run<true, CL, true>(eb, xb, 2 * CL, x);
        } else if (w == 3) {
            const double p = __builtin_fma(C[kChP2 + l], ends[j],
                                           __builtin_fma(C[kChP21 + l], xb[X4 + j], 0.125 * ends[8 + i]));
            (void)bwd_run<true, CL, true>(eb, xb, CL, wv.sum_contig8(p));
        } else {
            const double p = __builtin_fma(
                C[kChP3 + l], ends[8 + j],
                __builtin_fma(C[kChP32 + l], ends[j], __builtin_fma(C[kChP321 + l], xb[X4 + j], 0.125 * ends[16 + i])));
            (void)bwd_run<true, CL, true>(eb, xb, 0, wv.sum_contig8(p));
        }
    }

    // v = rho z - y products of the general rows for the next rhs
    IMPC_WF void write_v_products() {
        double *pb = pbuf();
        _Pragma("unroll") for (int s = 0; s < GS; s++) {
            // (an empty slot writes a zero product to the discard slot)
            double vv = rhog_(s) * z[s] - y[s];
            _Pragma("unroll") for (int e = 0; e < 4; e++) pb[gpk(s, e) >> 16] = a[s][e] * vv;
        }
        wv.lsync();
    }

    // --------------------------------------------------------------- one ADMM iteration
    IMPC_WF void iterate(bool need_delta) {
        const int W = Wst();
        double *rb = rbuf(), *tb = tbuf(), *eb = ebuf(), *xb = xbuf();
        const double sigma = sig_;
        const bool sweeper = (L >> 6) == rw;
#if defined(__HIP_DEVICE_COMPILE__)
        // kSweep19: each sweep's prologue, formed by its wavefront in front of the releasing barrier
        [[maybe_unused]] SweepPro fpro, bpro;
#endif
        IMPC_REP(kSecRhs) {
            // rhs = sigma x - q + A' v   (stage order; an empty slot's iterates, bounds and column
            // are zero, so it writes 0)
            _Pragma("unroll") for (int s = 0; s < VS; s++) {
                int v = NL * s + L;
                double vb = rhob(s) * zb[s] - yb[s];
                double r = sigma * x[s] - (DENSE ? ps_.q[s] : q[s]);
                r += ab[s] * vb;
                if constexpr (DENSE) r += col_gather_pass(v, s); else r += col_gather(v, hid_[s]);
                rb[v] = r;
            }
            wv.lsync();
        }
        IMPC_SEC(kSecRhs);
        IMPC_REP(kSecS1) {
            // S1: t_k = r_k[:8] - G_{k-1}[:, 8:] r_{k-1}[8:]  (every lane, without branches: a
            // stage-0 or empty slot has zero coupling coefficients, a control lane's t lands in a
            // slot nothing reads)
            _Pragma("unroll") for (int s = 0; s < VS; s++) {
                int v = NL * s + L;
                double t = rb[v];
                // (stage 0: the zero tail of the x exchange, not LDS below rb -- past the horizon's
                // last F block that is another QP's data or uninitialised)
                const double *rp = lds + (vs_[s] > 0 ? LD::R_OFF + 13 * (vs_[s] - 1) + 8 : LD::X_OFF + LD::NMAX);
                double rv[5];
                _Pragma("unroll") for (int cc = 0; cc < 5; cc++) rv[cc] = rp[cc];
                IMPC_LOADS_FIRST(5, 12);
                _Pragma("unroll") for (int cc = 0; cc < 5; cc++) t -= cp[s][cc] * rv[cc];
                tb[v] = kSweepPre * t;  // the forward sweep's input, pre-scaled (rstep)
            }
#if defined(__HIP_DEVICE_COMPILE__)
            if constexpr (kSweep19) {
                if (sweeper && W == LD::WSPEC) {
                    sweep_pro<LD::WSPEC, true>(fpro, rb);
                }
            }
#endif
            wv.lsync();
        }
        IMPC_SEC(kSecS1);
        IMPC_REP(kSecFwd) {
            // S2: forward 8-dim recursion a_{k+1} = t_{k+1} - F_k a_k on the 8x8 lane grid of each
            // wavefront (lane l = 8i + j).  Vectors of even stages sit at index i, of odd stages at
            // index j; F_k is stored as F_k[j][i] (k even) / F_k[i][j] (k odd), so even steps reduce
            // over i (strided: DPP row_ror 8, permlane16/32 swaps) and odd steps over j (contiguous
            // DPP), all in the VALU, with no transpose.  The next F and t are loaded two steps ahead.
            // One wavefront of the team (rw) runs it -- the others go straight to the barrier and
            // leave their SIMD's issue slots to the co-resident team.
            // (a_0 = t_0 = r_0[:8] is already in rb: stage 0 has no coupling, so S1 left it as is)
            // The long horizon's W = 39 instance runs it in chunks on all four wavefronts (CHUNK).
            if constexpr (CHUNK) {
                fwd_chunked(tb, rb);
            } else if (sweeper) {
                IMPC_PRIO_UP();
                if (W == LD::WSPEC) {
#if defined(__HIP_DEVICE_COMPILE__)
                    if constexpr (kSweep19) sweep_run<LD::WSPEC, true>(fpro, tb); else
#endif
                    fwd_sweep<LD::WSPEC>(tb, rb, W);
                } else
                    fwd_sweep<0>(tb, rb, W);
                IMPC_PRIO_DOWN();
            }
            wv.lsync();
        }
        IMPC_SEC(kSecFwd);
        IMPC_REP(kSecS3) {
            // S3: e_k = Ahat_k^{-1} rhat_k
            _Pragma("unroll") for (int s = 0; s < VS; s++) {
                const double *rk = lds + LD::R_OFF + 13 * vs_[s];
                double rv[13];
                _Pragma("unroll") for (int cc = 0; cc < 13; cc++) rv[cc] = rk[cc];
                IMPC_LOADS_FIRST(7, 20);
                double e = 0.0;
                _Pragma("unroll") for (int cc = 0; cc < 13; cc++) e += ainv[s][cc] * rv[cc];
                // the state part pre-scaled for the backward sweep (rstep); S5 reads the controls' e
                eb[NL * s + L] = vr_[s] < 8 ? kSweepPre * e : e;
            }
#if defined(__HIP_DEVICE_COMPILE__)
            if constexpr (kSweep19) {
                if (sweeper && W == LD::WSPEC) {
                    sweep_pro<LD::WSPEC, false>(bpro, xb);
                }
            }
#endif
            wv.lsync();
        }
        IMPC_SEC(kSecS3);
        IMPC_REP(kSecBwd) {
            // S4: backward 8-dim recursion x_k[:8] = e_k[:8] - F_k' x_{k+1}[:8] on the same grid and
            // stored layout: even steps reduce over j (contiguous), odd steps over i (strided).
            if (L < 8) xb[13 * W + L] = (1.0 / kSweepPre) * eb[13 * W + L];
            if constexpr (CHUNK) {
                bwd_chunked(eb, xb);
            } else if (sweeper) {
                IMPC_PRIO_UP();
                if (W == LD::WSPEC) {
#if defined(__HIP_DEVICE_COMPILE__)
                    if constexpr (kSweep19) sweep_run<LD::WSPEC, false>(bpro, eb); else
#endif
                    bwd_sweep<((LD::WSPEC - 1) & 1) != 0, LD::WSPEC>(eb, xb, W);
                } else if ((W - 1) & 1)
                    bwd_sweep<true, 0>(eb, xb, W);
                else
                    bwd_sweep<false, 0>(eb, xb, W);
                IMPC_PRIO_DOWN();
            }
            wv.lsync();
        }
        IMPC_SEC(kSecBwd);
        IMPC_REP(kSecS5) {
            // S5: controls x_k[8:] = e_k[8:] - G_k[:, 8:]' x_{k+1}[:8]  (every lane, the state lanes'
            // and empty slots' results to their discard slots)
            _Pragma("unroll") for (int s = 0; s < VS; s++) {
                const double *xn = lds + LD::X_OFF + 13 * (vs_[s] + 1);
                double t = eb[NL * s + L];
                double xv[8];
                _Pragma("unroll") for (int j = 0; j < 8; j++) xv[j] = xn[j];
                IMPC_LOADS_FIRST(5, 16);
                _Pragma("unroll") for (int j = 0; j < 8; j++) t -= cp[s][j] * xv[j];
                *(vok[s] && vr_[s] >= 8 ? xb + NL * s + L : lds + LD::JUNK_OFF + L) = t;
            }
            wv.lsync();
        }
        IMPC_SEC(kSecS5);
        update_and_products(need_delta);
    }

    // project_z (auxil.h): min(max(v, l), u), as v_max_f64 / v_min_f64 -- the same value as the
    // reference's c_max / c_min except the sign of a zero when v equals a zero bound
    IMPC_WF static double clampz(double v, double l, double u) { return __builtin_fmin(__builtin_fmax(v, l), u); }
    // The same two instructions written out (DENSE, device code): in front of each v_max_f64 /
    // v_min_f64 the compiler canonicalises a bound it cannot see the origin of (v_max_f64 b, b, b --
    // a bound defined outside the iteration's basic block, so six FP64 instructions per iteration
    // of the two-slot shape); a bound is never a NaN (load() clamps it), so that is the identity
    IMPC_WF static double clampz_raw(double v, double l, double u) {
#if defined(__HIP_DEVICE_COMPILE__)
        double r;
        asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(v), "v"(l));
        asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(r), "v"(u));
        return r;
#else
        return clampz(v, l, u);
#endif
    }

    // update_x and the box rows (update_z / project / update_y), the general rows, and the
    // products of the next rhs (the end of every ADMM iteration).  need_delta: the check-iteration
    // deltas are written.
    IMPC_WF void update_and_products(bool need_delta) {
        double *xb = xbuf();
        const double alpha = alp_, oma = (double)1.0 - alp_;
        _Pragma("unroll") for (int s = 0; s < VS; s++) {
            if (!vok[s]) continue;
            double xt = xb[NL * s + L];
            double xn = alpha * xt + oma * x[s];
            if (need_delta) dxv(s) = xn - x[s];
            x[s] = xn;
            double zt = ab[s] * xt;
            double zr = alpha * zt + oma * zb[s];
            double zn;
            if constexpr (DENSE) zn = clampz_raw(zr + rhoib(s) * yb[s], ps_.lb[s], ps_.ub[s]);
            else zn = clampz(zr + rhoib(s) * yb[s], lb[s], ub[s]);
            double dy = rhob(s) * (zr - zn);
            yb[s] += dy;
            if (need_delta) dyb(s) = dy;
            zb[s] = zn;
        }
        // general rows, without a per-slot branch: an empty slot's columns are the zero tail of the
        // x exchange, its A values, bounds and iterates zero, so it computes zeros
        double xg[GS][4];
        _Pragma("unroll") for (int s = 0; s < GS; s++) {
            _Pragma("unroll") for (int e = 0; e < 4; e++) xg[s][e] = xb[gpk(s, e) & 0xFFFF];
        }
        IMPC_LOADS_FIRST(4 * GS, 8 * GS);
        _Pragma("unroll") for (int s = 0; s < GS; s++) {
            double zt = 0.0;
            _Pragma("unroll") for (int e = 0; e < 4; e++) zt += a[s][e] * xg[s][e];
            double zr = alpha * zt + oma * z[s];
            double zn;
            if constexpr (DENSE) zn = clampz_raw(zr + rhoig_(s) * y[s], ps_.lg[s], ps_.ug[s]);
            else zn = clampz(zr + rhoig_(s) * y[s], lg[s], ug[s]);
            double dy = rhog_(s) * (zr - zn);
            y[s] += dy;
            if (need_delta) dyg(s) = dy;
            z[s] = zn;
        }
        // no barrier: the products go to their own LDS region, which nothing above reads, and
        // write_v_products ends with the barrier the next rhs gather needs
        IMPC_SEC(kSecUpdate);
        IMPC_REP(kSecProducts) write_v_products();
        IMPC_SEC(kSecProducts);
    }

    // ------------------------------------------------------------ update_info + checks
    struct Info {
        double pri_res, dua_res, pri_norm_u, dua_norm_u, pri_norm_s, dua_norm_s, pri_plain, dua_plain;
        // the infeasibility tests' first stages (is_primal_infeasible: ||E P(dy)||, u'P(dy)_+ +
        // l'P(dy)_-; is_dual_infeasible: ||D dx||, q'dx, and its ||D^-1 P dx||), reduced with the
        // norms above
        double pinf_nrm, pinf_lhs, dinf_nrm, dinf_qdx, dinf_pdx;
    };

    IMPC_WF void load_scal(int64_t b, double D[VS], double Eb[VS], double Eg[GS]) {
        const double *sc = scal(b);
        _Pragma("unroll") for (int s = 0; s < VS; s++) {
            D[s] = vok[s] ? sc[NL * s + L] : 1.0;
            Eb[s] = vok[s] ? sc[T.n + NL * s + L] : 1.0;
        }
        _Pragma("unroll") for (int s = 0; s < GS; s++) Eg[s] = gok[s] ? sc[2 * T.n + NL * s + L] : 1.0;
    }

    IMPC_WF void update_info(Info &inf, const double D[VS], const double Eb[VS], const double Eg[GS]) {
        const bool unsc = st.scaling > 0 && !st.scaled_termination;
        double *xb = xbuf(), *pb = pbuf();
        _Pragma("unroll") for (int s = 0; s < VS; s++)
            if (vok[s]) xb[NL * s + L] = x[s];
        // A'y products of the general rows
        _Pragma("unroll") for (int s = 0; s < GS; s++) {
            if (gok[s])
                _Pragma("unroll") for (int e = 0; e < 4; e++) pb[gdst(s, e)] = a[s][e] * y[s];
        }
        wv.sync();
        double pr_u = 0, z_u = 0, ax_u = 0, pr_p = 0, z_p = 0, ax_p = 0;
        _Pragma("unroll") for (int s = 0; s < VS; s++) {
            if (!vok[s]) continue;
            double ax = ab[s] * x[s], r = ax + -1 * zb[s], ei = 1. / Eb[s];
            pr_p = dmax(pr_p, fabs(r));
            z_p = dmax(z_p, fabs(zb[s]));
            ax_p = dmax(ax_p, fabs(ax));
            pr_u = dmax(pr_u, fabs(ei * r));
            z_u = dmax(z_u, fabs(ei * zb[s]));
            ax_u = dmax(ax_u, fabs(ei * ax));
        }
        _Pragma("unroll") for (int s = 0; s < GS; s++) {
            if (!gok[s]) continue;
            double ax = 0.0;
            _Pragma("unroll") for (int e = 0; e < 4; e++) ax += a[s][e] * xb[gcol(s, e)];
            double r = ax + -1 * z[s], ei = 1. / Eg[s];
            pr_p = dmax(pr_p, fabs(r));
            z_p = dmax(z_p, fabs(z[s]));
            ax_p = dmax(ax_p, fabs(ax));
            pr_u = dmax(pr_u, fabs(ei * r));
            z_u = dmax(z_u, fabs(ei * z[s]));
            ax_u = dmax(ax_u, fabs(ei * ax));
        }
        double dr_u = 0, q_u = 0, aty_u = 0, px_u = 0, dr_p = 0, q_p = 0, aty_p = 0, px_p = 0;
        _Pragma("unroll") for (int s = 0; s < VS; s++) {
            if (!vok[s]) continue;
            double aty = ab[s] * yb[s] + col_gather(NL * s + L, hid_[s]);
            double px = pd[s] * x[s];
            double r = q[s] + 1 * px;
            r = r + 1 * aty;
            double di = 1. / D[s];
            dr_p = dmax(dr_p, fabs(r));
            q_p = dmax(q_p, fabs(q[s]));
            aty_p = dmax(aty_p, fabs(aty));
            px_p = dmax(px_p, fabs(px));
            dr_u = dmax(dr_u, fabs(di * r));
            q_u = dmax(q_u, fabs(di * q[s]));
            aty_u = dmax(aty_u, fabs(di * aty));
            px_u = dmax(px_u, fabs(di * px));
        }
        {
            // the infeasibility tests' lane-local parts too (the check needs them whenever it does
            // not terminate): one team reduction for 16 maxima and 2 sums
            double pn, pl, dn, dq, dp;
            pinf_partials(Eb, Eg, pn, pl);
            dinf_partials(D, dn, dq, dp);
            double r[17] = {pr_u, z_u, ax_u, pr_p, z_p, ax_p, dr_u, q_u, aty_u, px_u, dr_p, q_p, aty_p, px_p, pn, dn, dp};
            double sm[2] = {pl, dq};
            wv.max_sum_n(r, sm);
            pr_u = r[0], z_u = r[1], ax_u = r[2], pr_p = r[3], z_p = r[4], ax_p = r[5], dr_u = r[6];
            q_u = r[7], aty_u = r[8], px_u = r[9], dr_p = r[10], q_p = r[11], aty_p = r[12], px_p = r[13];
            inf.pinf_nrm = r[14];
            inf.dinf_nrm = r[15];
            inf.dinf_pdx = r[16];
            inf.pinf_lhs = sm[0];
            inf.dinf_qdx = sm[1];
        }
        inf.pri_plain = pr_p;
        inf.dua_plain = dr_p;
        inf.pri_norm_s = dmax(z_p, ax_p);
        inf.dua_norm_s = dmax(dmax(q_p, aty_p), px_p);
        if (unsc) {
            inf.pri_res = T.m == 0 ? 0.0 : pr_u;
            inf.dua_res = cinv * dr_u;
            inf.pri_norm_u = dmax(z_u, ax_u);
            inf.dua_norm_u = dmax(dmax(q_u, aty_u), px_u) * cinv;
        } else {
            inf.pri_res = T.m == 0 ? 0.0 : pr_p;
            inf.dua_res = dr_p;
            inf.pri_norm_u = inf.pri_norm_s;
            inf.dua_norm_u = inf.dua_norm_s;
        }
        // (no barrier: the reduction's last one already follows every read of the exchange
        // buffers above)
    }

    // is_primal_infeasible's projection of dy onto the normal cone of the bounds (OSQP projects
    // delta_y in place; the next ADMM step overwrites it, so only the test's second stage sees it)
    IMPC_WF static double pinf_proj(double d, double l, double u) {
        if (u > kInf * kMinScaling) return (l < -kInf * kMinScaling) ? 0.0 : dmin(d, 0.0);
        if (l < -kInf * kMinScaling) return dmax(d, 0.0);
        return d;
    }
    // is_primal_infeasible, lane-local part: ||E P(dy)||_inf and u' max(P(dy), 0) + l' min(P(dy), 0)
    IMPC_WF void pinf_partials(const double Eb[VS], const double Eg[GS], double &nrm_o, double &lhs_o) {
        const bool unsc = st.scaling > 0 && !st.scaled_termination;
        double nrm = 0.0, lhs = 0.0;
        _Pragma("unroll") for (int s = 0; s < VS; s++) {
            if (!vok[s]) continue;
            const double d = pinf_proj(dyb(s), lb[s], ub[s]);
            nrm = dmax(nrm, fabs(unsc ? Eb[s] * d : d));
            lhs += ub[s] * dmax(d, 0) + lb[s] * dmin(d, 0);
        }
        _Pragma("unroll") for (int s = 0; s < GS; s++) {
            if (!gok[s]) continue;
            const double d = pinf_proj(dyg(s), lg[s], ug[s]);
            nrm = dmax(nrm, fabs(unsc ? Eg[s] * d : d));
            lhs += ug[s] * dmax(d, 0) + lg[s] * dmin(d, 0);
        }
        nrm_o = nrm;
        lhs_o = lhs;
    }
    // ... and the rest, from the team-reduced norm and sum
    IMPC_WF int pinf_stage2(double eps, double nrm, double lhs, const double D[VS]) {
        const bool unsc = st.scaling > 0 && !st.scaled_termination;
        int res = 0;
        if (nrm > kDivTol && lhs < eps * nrm) {
            double *pb = pbuf();
            _Pragma("unroll") for (int s = 0; s < GS; s++) {
                if (gok[s]) {
                    const double d = pinf_proj(dyg(s), lg[s], ug[s]);
                    _Pragma("unroll") for (int e = 0; e < 4; e++) pb[gdst(s, e)] = a[s][e] * d;
                }
            }
            wv.sync();
            double mx = 0.0;
            _Pragma("unroll") for (int s = 0; s < VS; s++) {
                if (!vok[s]) continue;
                double t = ab[s] * pinf_proj(dyb(s), lb[s], ub[s]) + col_gather(NL * s + L, hid_[s]);
                if (unsc) t = (1. / D[s]) * t;
                mx = dmax(mx, fabs(t));
            }
            mx = wv.max(mx);
            res = mx < eps * nrm;
            wv.sync();
        }
        return res;
    }

    // is_dual_infeasible, lane-local part: ||D dx||_inf, q' dx and ||D^-1 P dx||_inf
    IMPC_WF void dinf_partials(const double D[VS], double &nrm_o, double &qdx_o, double &pdx_o) {
        const bool unsc = st.scaling > 0 && !st.scaled_termination;
        double nrm = 0.0, qdx = 0.0, pdx = 0.0;
        _Pragma("unroll") for (int s = 0; s < VS; s++) {
            if (!vok[s]) continue;
            nrm = dmax(nrm, fabs(unsc ? D[s] * dxv(s) : dxv(s)));
            qdx += q[s] * dxv(s);
            double pv = pd[s] * dxv(s);
            if (unsc) pv = (1. / D[s]) * pv;
            pdx = dmax(pdx, fabs(pv));
        }
        nrm_o = nrm;
        qdx_o = qdx;
        pdx_o = pdx;
    }
    IMPC_WF int dinf_stage2(double eps, double nrm, double qdx, double mx, const double Eb[VS], const double Eg[GS]) {
        const bool unsc = st.scaling > 0 && !st.scaled_termination;
        const double cs = unsc ? c : 1.0;
        int res = 0;
        if (nrm > kDivTol && qdx < cs * eps * nrm) {
            if (mx < cs * eps * nrm) {
                double *xb = xbuf();
                _Pragma("unroll") for (int s = 0; s < VS; s++)
                    if (vok[s]) xb[NL * s + L] = dxv(s);
                wv.sync();
                double viol = 0.0;
                _Pragma("unroll") for (int s = 0; s < VS; s++) {
                    if (!vok[s]) continue;
                    double t = ab[s] * dxv(s);
                    if (unsc) t = (1. / Eb[s]) * t;
                    if ((ub[s] < kInf * kMinScaling && t > eps * nrm) || (lb[s] > -kInf * kMinScaling && t < -eps * nrm))
                        viol = 1.0;
                }
                _Pragma("unroll") for (int s = 0; s < GS; s++) {
                    if (!gok[s]) continue;
                    double t = 0.0;
                    _Pragma("unroll") for (int e = 0; e < 4; e++) t += a[s][e] * xb[gcol(s, e)];
                    if (unsc) t = (1. / Eg[s]) * t;
                    if ((ug[s] < kInf * kMinScaling && t > eps * nrm) || (lg[s] > -kInf * kMinScaling && t < -eps * nrm))
                        viol = 1.0;
                }
                viol = wv.max(viol);
                res = viol == 0.0;
                wv.sync();
            }
        }
        return res;
    }

    IMPC_WF int check_termination(const Info &inf, int approximate, int64_t &status, double &obj, const double D[VS],
                                  const double Eb[VS], const double Eg[GS]) {
        if ((inf.pri_res > kInf) || (inf.dua_res > kInf)) {
            status = IMPC_NON_CVX;
            obj = kNan;
            return 1;
        }
        double eps_abs = st.eps_abs, eps_rel = st.eps_rel, eps_pinf = st.eps_prim_inf, eps_dinf = st.eps_dual_inf;
        if (approximate) {
            eps_abs *= 10;
            eps_rel *= 10;
            eps_pinf *= 10;
            eps_dinf *= 10;
        }
        int prim_ok = 0, dual_ok = 0, prim_inf = 0, dual_inf = 0;
        const bool ptest = T.m != 0 && !(inf.pri_res < eps_abs + eps_rel * inf.pri_norm_u);
        prim_ok = !ptest;
        dual_ok = inf.dua_res < eps_abs + eps_rel * inf.dua_norm_u;
        // the first stages' norms and sums were reduced with the residual norms (update_info)
        if (ptest) prim_inf = pinf_stage2(eps_pinf, inf.pinf_nrm, inf.pinf_lhs, D);
        if (!dual_ok) dual_inf = dinf_stage2(eps_dinf, inf.dinf_nrm, inf.dinf_qdx, inf.dinf_pdx, Eb, Eg);
        if (prim_ok && dual_ok) {
            status = approximate ? IMPC_SOLVED_INACCURATE : IMPC_SOLVED;
            return 1;
        } else if (prim_inf) {
            status = approximate ? IMPC_PRIMAL_INFEASIBLE_INACCURATE : IMPC_PRIMAL_INFEASIBLE;
            obj = kInf;
            return 1;
        } else if (dual_inf) {
            status = approximate ? IMPC_DUAL_INFEASIBLE_INACCURATE : IMPC_DUAL_INFEASIBLE;
            obj = -kInf;
            return 1;
        }
        return 0;
    }

    IMPC_WF double rho_estimate(const Info &inf) const {
        double pri = inf.pri_plain / (inf.pri_norm_s + kDivTol);
        double dua = inf.dua_plain / (inf.dua_norm_s + kDivTol);
        double est = R.rho * sqrt(pri / (dua + kDivTol));
        return dmin(dmax(est, kRhoMin), kRhoMax);
    }

    // ------------------------------------------------------------------ whole solve
    // The scaling vectors D, E live in the per-QP global scratch (written by scale()) and are
    // reloaded only where OSQP needs them (warm start, termination checks, unscaling), so they do
    // not occupy registers across the ADMM loop.
    // the persistent workspace (WaveIO::persist) from the registers: rho and the scaled iterates
    IMPC_WF void write_persist(double *ps) {
        const int n = T.n;
        double *it = ps + kPersistHdr;
        if (L == 0) ps[kPersistHdr - 1] = R.rho;
        _Pragma("unroll") for (int s = 0; s < VS; s++)
            if (vok[s]) {
                const int v = NL * s + L;
                it[v] = x[s];
                it[n + v] = zb[s];
                it[2 * n + v] = yb[s];
            }
        _Pragma("unroll") for (int s = 0; s < GS; s++)
            if (gok[s]) {
                const int g = NL * s + L;
                it[3 * n + g] = z[s];
                it[3 * n + T.mg + g] = y[s];
            }
    }

    IMPC_WF void solve(int64_t b) {
        const int n = T.n, m = T.m;
        // time_limit clock: from the start of the QP's setup (load, scaling, factorisation), as
        // OSQP 0.6.2 counts setup_time + solve time on a first run (every solveTraj call is one);
        // the profiling record (qpt) starts at the same tick, so a QP stopped by its limit always
        // shows a recorded latency of at least that limit.  A persistent-workspace resume (OSQP's
        // non-first run) counts from the same tick: OSQP then counts update_time + solve time, and
        // here the update work (the scaling replay, the row types, the refactorisation) runs at the
        // start of the resumed solve -- one difference: OSQP refactors on osqp_update_bounds only
        // when a row changes type, the resume always does (its time counts against the limit)
        const uint64_t t0 = device_clock();
        rw = (int)(b % (NL / 64));  // spread the serial recursions of co-resident QPs over SIMDs
#if defined(__HIP_DEVICE_COMPILE__)
        // recursion wave from the hardware placement (HW_REG_HW_ID: WAVE_ID [3:0], SIMD_ID [5:4]):
        // the wave on SIMD (wave slot of the team's wave 0) mod 4, so co-resident teams, which sit
        // in different wave slots, run their recursions on different SIMDs; the QP-index choice
        // above when no wave of the team is on that SIMD
        if ((L & 63) == 0) lds[LD::JUNK_OFF + (L >> 6)] = (double)(__builtin_amdgcn_s_getreg((31 << 11) | 4) & 0x3f);
#endif
        IMPC_SEC_START();
        clear_exchange();
#if defined(__HIP_DEVICE_COMPILE__)
        {
            const int target = (int)lds[LD::JUNK_OFF] & 3;
            _Pragma("unroll") for (int w = NL / 64 - 1; w >= 0; w--)
                if (((int)lds[LD::JUNK_OFF + w] >> 4) == target) rw = w;
        }
#endif
        load(b);
        double *ps = io.persist ? io.persist + b * persist_stride(T.n, T.mg) : nullptr;
        {
            double D[VS], Eb[VS], Eg[GS];
            scale(b, D, Eb, Eg, ps);
            if (ps && ((io.resume == 1 && io.q_updated) || io.q_scale))  // osqp_update_lin_cost: q = c (D q)
                _Pragma("unroll") for (int s = 0; s < VS; s++)
                    if (vok[s]) q[s] = (D[s] * io.q[b * n + T.var_orig[NL * s + L]]) * c;
        }
        set_rho(ps && io.resume ? ps[kPersistHdr - 1] : dmin(dmax(st.rho, kRhoMin), kRhoMax));
        IMPC_SEC(kSecSetup);
        int bad = 0;
        IMPC_REP(kSecFactor) bad = factorize();  // (phase-cost experiments only)
        IMPC_SEC(kSecFactor);
        impc_info *out = io.info + b;
        if (bad) {
            _Pragma("unroll") for (int s = 0; s < VS; s++)
                if (vok[s]) io.xo[b * n + T.var_orig[NL * s + L]] = kNan;
            _Pragma("unroll") for (int s = 0; s < VS; s++)
                if (vok[s]) io.yo[b * m + T.var_boxrow[NL * s + L]] = kNan;
            _Pragma("unroll") for (int s = 0; s < GS; s++)
                if (gok[s]) io.yo[b * m + T.gen_row[NL * s + L]] = kNan;
            if (L == 0) {
                out->iter = 0;
                out->status_val = IMPC_NON_CVX;
                out->rho_updates = 0;
                out->setup_exitflag = IMPC_NONCVX_ERROR;
                out->obj_val = kNan;
                out->pri_res = out->dua_res = 0.0;
                out->rho_estimate = R.rho;
            }
            // a first setup that fails its factorisation leaves a defined workspace: the settings'
            // rho and zero iterates (osqp_setup's cold_start; load() zeroed them), so a resume after a
            // matrix update (impc_batch_update_matrices) starts as a fresh setup would; a failed
            // resume keeps the workspace it had (OSQP keeps work->x, z, y when osqp_update_P / _A
            // fails to refactor)
            if (ps && io.resume == 0) write_persist(ps);
            wv.sync();
            return;
        }
        if constexpr (LD::ONCHIP)  // dx of a check before any ADMM step (load())
            _Pragma("unroll") for (int s = 0; s < VS; s++) dxv(s) = 0.0;
        // iterates: zero, then osqp_warm_start (x <- Dinv x, y <- c Einv y, z <- A x)
        if (ps && io.resume && !io.has_ws && st.warm_start) {  // OSQP keeps its iterates between solves
            const double *it = ps + kPersistHdr;
            _Pragma("unroll") for (int s = 0; s < VS; s++) {
                if (!vok[s]) continue;
                const int v = NL * s + L;
                x[s] = it[v];
                zb[s] = it[n + v];
                yb[s] = it[2 * n + v];
            }
            _Pragma("unroll") for (int s = 0; s < GS; s++) {
                if (!gok[s]) continue;
                const int g = NL * s + L;
                z[s] = it[3 * n + g];
                y[s] = it[3 * n + T.mg + g];
            }
        } else if (io.has_ws) {
            double D[VS], Eb[VS], Eg[GS];
            load_scal(b, D, Eb, Eg);
            double *xb = xbuf();
            _Pragma("unroll") for (int s = 0; s < VS; s++) {
                if (!vok[s]) continue;
                int ov = T.var_orig[NL * s + L];
                double xv = io.xws[b * n + ov];
                x[s] = st.scaling > 0 ? (1. / D[s]) * xv : xv;
                double yv = io.has_ws == 1 ? io.yws[b * m + T.var_boxrow[NL * s + L]] : 0.0;
                if (st.scaling > 0) {
                    yv = (1. / Eb[s]) * yv;
                    yv *= c;
                }
                yb[s] = yv;
                zb[s] = ab[s] * x[s];
                xb[NL * s + L] = x[s];
            }
            wv.sync();
            _Pragma("unroll") for (int s = 0; s < GS; s++) {
                if (!gok[s]) continue;
                double yv = io.has_ws == 1 ? io.yws[b * m + T.gen_row[NL * s + L]] : 0.0;
                if (st.scaling > 0) {
                    yv = (1. / Eg[s]) * yv;
                    yv *= c;
                }
                y[s] = yv;
                double zz = 0.0;
                _Pragma("unroll") for (int e = 0; e < 4; e++) zz += a[s][e] * xb[gcol(s, e)];
                z[s] = zz;
            }
            wv.sync();
            clear_exchange();
        }
        write_v_products();
        IMPC_SEC(kSecWarm);

        int64_t status = IMPC_UNSOLVED, rho_updates = 0;
        int32_t iter;
        double obj = 0.0, rho_est = R.rho;
        Info inf{};
        int64_t info_iter = 0;
        const int chk = st.check_termination;
        int can_check = 0;
        // counters of the next check / rho update instead of iter % interval
        // the loop's settings read once into registers (the batch's settings live in global memory
        // for a grouped launch: read in the loop they cost a scalar-memory round trip each
        // iteration, after every barrier)
        int32_t max_iter = st.max_iter;  // (dropped to 0 by a failed refactorisation, below)
        const int32_t rho_int = st.adaptive_rho ? st.rho_interval : 0;
        // team-uniform, in scalar registers (io.tlim: the QP's own limit)
        const double tl = wv.uniform(io.tlim ? io.tlim[b] : st.time_limit), tick = st.tick_s;
        const bool tlim = tl > 0;
        int32_t chk_left = chk, rho_left = rho_int;
        // The refactorisation after an adaptive-rho update runs between two passes of the inner
        // iteration loop rather than inside it: the register allocator then places the spills the
        // factorisation's temporaries force around that (rare) call, outside the hot loop.
        bool refac = false;
        iter = 1;
        for (;;) {
            if (refac) {
                refac = false;
                // osqp_solve: a failed rho update ends the solve with exitflag 1.  It leaves the loop
                // through the loop's one exit -- the pass bound drops to 0, the status register
                // carries the mark -- so no second exit edge (and its live values) burdens the
                // register allocation of the passes (round 6: 217.5 -> 213.9 ms per config-3 launch)
                // A rho update on the solve's last iteration: no pass follows, and the post-loop
                // checks read that iteration's deltas, which share the exchange vectors with the
                // factorisation's scratch -- each lane carries its own across the call
                const bool last = LD::ONCHIP && iter > max_iter;
                double kdy[VS], kdg[GS];
                if (last) {
                    _Pragma("unroll") for (int s = 0; s < VS; s++) kdy[s] = vok[s] ? dyb(s) : 0.0;
                    _Pragma("unroll") for (int s = 0; s < GS; s++) kdg[s] = gok[s] ? dyg(s) : 0.0;
                }
                if (factorize()) {
                    max_iter = 0;
                    status = kRefailMark;
                }
                if (last) {  // (after factorize()'s last barrier; R[NL - 1] of an n < NL pattern stays 0)
                    _Pragma("unroll") for (int s = 0; s < VS; s++)
                        if (vok[s]) dyb(s) = kdy[s];
                    _Pragma("unroll") for (int s = 0; s < GS; s++) dyg(s) = kdg[s];
                }
                write_v_products();
                IMPC_SEC(kSecFactor);
            }
            // the hot loop: ADMM steps up to the next termination check / rho update (or the end);
            // the check and the update run between two passes of it, so their code and registers
            // sit outside it (the operations are those of one loop, in the same order)
            bool chk_now = false, rho_now = false, stop = false;
            // the pass runs to its next event nxt = min(iterations left, chk_left, rho_left) (counted
            // once per pass, not per iteration); only its last iteration can be a check /
            // rho-update / max_iter one.  osqp_solve's time-limit test sits after the ADMM steps,
            // before can_check is recomputed (so a stop keeps the previous iteration's value); one
            // team-wide decision
            if (iter <= max_iter) {
                int nxt = max_iter - iter + 1;
                if (chk && chk_left < nxt) nxt = chk_left;
                if (rho_int && rho_left < nxt) nxt = rho_left;
                const bool ce = chk && chk_left == nxt, re = rho_int && rho_left == nxt;
                const bool nd_last = ce || iter + nxt - 1 == max_iter || tlim;
                begin_pass();
                for (int t = 1;; t++) {
                    iterate(t == nxt ? nd_last : tlim);
                    if (tlim) {
                        const double el = wv.max((double)(device_clock() - t0) * tick);
                        if (el >= tl) {
                            status = IMPC_TIME_LIMIT_REACHED;
                            stop = true;
                            if (t > 1) can_check = 0;  // the previous iteration was no check
                            break;
                        }
                    }
                    if (t == nxt) break;
                    iter++;
                }
                if (!stop) {
                    chk_now = ce;
                    rho_now = re;
                    if (chk) chk_left = ce ? chk : chk_left - nxt;
                    if (rho_int) rho_left = re ? rho_int : rho_left - nxt;
                    can_check = chk_now;
                    if (!(chk_now || rho_now)) iter++;
                }
            }
            if (stop || iter > max_iter) break;
            if (can_check) {
                IMPC_SEC_START();
                double D[VS], Eb[VS], Eg[GS];
                load_scal(b, D, Eb, Eg);
                int done = 0;
                IMPC_REP(kSecChecks) {  // (phase-cost experiments only: the check is idempotent)
                    update_info(inf, D, Eb, Eg);
                    done = check_termination(inf, 0, status, obj, D, Eb, Eg);
                }
                info_iter = iter;
                write_v_products();
                IMPC_SEC(kSecChecks);
                if (done) break;
            }
            if (rho_now) {
                if (!can_check) {
                    double D[VS], Eb[VS], Eg[GS];
                    load_scal(b, D, Eb, Eg);
                    update_info(inf, D, Eb, Eg);
                    info_iter = iter;
                    write_v_products();
                }
                double rn = rho_estimate(inf);
                rho_est = rn;
                if ((rn > R.rho * st.adaptive_rho_tolerance) || (rn < R.rho / st.adaptive_rho_tolerance)) {
                    IMPC_SEC(kSecChecks);
                    set_rho(dmin(dmax(rn, kRhoMin), kRhoMax));
                    rho_updates += 1;
                    refac = true;
                }
            }
            iter++;  // this iteration is complete; the next pass starts at the next one
        }
        if (status == kRefailMark) {
            // OSQP 0.6.2 jumps to exit: no termination check, no stored solution (the outputs keep
            // the previous solve's), status stays UNSOLVED, info.iter is the last update_info's;
            // the workspace keeps the new rho and its iterates as they are
            if (ps) write_persist(ps);
            if (L == 0) {
                out->iter = info_iter;
                out->status_val = IMPC_UNSOLVED;
                out->rho_updates = rho_updates;
                out->setup_exitflag = 0;
                out->pri_res = inf.pri_res;
                out->dua_res = inf.dua_res;
                out->rho_estimate = rho_est;
            }
            wv.sync();
            return;
        }
        IMPC_SEC_START();
        double D[VS], Eb[VS], Eg[GS];
        load_scal(b, D, Eb, Eg);
        if (!can_check) {  // post-loop update_info / check, as osqp_solve
            update_info(inf, D, Eb, Eg);
            info_iter = iter - 1;
            check_termination(inf, 0, status, obj, D, Eb, Eg);
        }
        const bool has_sol = status != IMPC_PRIMAL_INFEASIBLE && status != IMPC_PRIMAL_INFEASIBLE_INACCURATE &&
                             status != IMPC_DUAL_INFEASIBLE && status != IMPC_DUAL_INFEASIBLE_INACCURATE &&
                             status != IMPC_NON_CVX;
        if (has_sol) {
            double qf = 0.0;
            _Pragma("unroll") for (int s = 0; s < VS; s++)
                if (vok[s]) qf += (double).5 * pd[s] * x[s] * x[s] + q[s] * x[s];
            obj = wv.sum(qf);
            if (st.scaling > 0) obj *= cinv;
        }
        if (status == IMPC_UNSOLVED) {
            if (!check_termination(inf, 1, status, obj, D, Eb, Eg)) status = IMPC_MAX_ITER_REACHED;
        }
        rho_est = rho_estimate(inf);
        const bool has_sol2 = status != IMPC_PRIMAL_INFEASIBLE && status != IMPC_PRIMAL_INFEASIBLE_INACCURATE &&
                              status != IMPC_DUAL_INFEASIBLE && status != IMPC_DUAL_INFEASIBLE_INACCURATE &&
                              status != IMPC_NON_CVX;
        const bool scaled = st.scaling > 0;
        _Pragma("unroll") for (int s = 0; s < VS; s++) {
            if (!vok[s]) continue;
            int v = NL * s + L;
            io.xo[b * n + T.var_orig[v]] = has_sol2 ? (scaled ? D[s] * x[s] : x[s]) : kNan;
            double yv = has_sol2 ? (scaled ? (Eb[s] * yb[s]) * cinv : yb[s]) : kNan;
            io.yo[b * m + T.var_boxrow[v]] = yv;
        }
        _Pragma("unroll") for (int s = 0; s < GS; s++) {
            if (!gok[s]) continue;
            double yv = has_sol2 ? (scaled ? (Eg[s] * y[s]) * cinv : y[s]) : kNan;
            io.yo[b * m + T.gen_row[NL * s + L]] = yv;
        }
        if (ps) {  // the workspace after osqp_solve: rho and the scaled iterates -- zero when the
                   // solve ended without a solution (store_solution's cold_start, auxil.c)
            if (!has_sol2) {
                _Pragma("unroll") for (int s = 0; s < VS; s++) x[s] = zb[s] = yb[s] = 0.0;
                _Pragma("unroll") for (int s = 0; s < GS; s++) z[s] = y[s] = 0.0;
            }
            write_persist(ps);
        }
        if (L == 0 && io.qpt) {
            io.qpt[2 * b] = t0;
            io.qpt[2 * b + 1] = device_clock();
        }
        if (L == 0) {
            out->iter = info_iter;
            out->status_val = status;
            out->rho_updates = rho_updates;
            out->setup_exitflag = 0;
            out->obj_val = obj;
            out->pri_res = inf.pri_res;
            out->dua_res = inf.dua_res;
            out->rho_estimate = rho_est;
        }
        wv.sync();
#if defined(IMPC_SECTION_PROF) && defined(__HIP_DEVICE_COMPILE__)
        IMPC_SEC(kSecOutput);
        if (L == 0 && io.sec) {
            sec_acc[kSecIters] = (uint64_t)info_iter;
            _Pragma("unroll") for (int i = 0; i < kSecCount; i++) atomicAdd(io.sec + i, (unsigned long long)sec_acc[i]);
        }
#endif
    }
};

}  // namespace impc
