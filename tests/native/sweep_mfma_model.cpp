// Host model of the stage recursions on v_mfma_f64_4x4x4_4b_f64 (csrc/mpc_wave.hpp sweep_mfma): the
// instruction and the two DPP controls modelled on 64 lanes with the operand layout measured on gfx950
// (csrc/sweep_mfma_map.hpp), driven by the kernel's own lane maps, stored F layout (-F_k, even
// stages transposed), 1/8 pre-scaled inputs and capture rule.  Both W-step sweeps on
// random F, t and e are compared with a plain double loop.  Stand-alone (own main), host only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../intent-mpc_amd/csrc/sweep_mfma_map.hpp"

namespace M = impc::mfmap;

// D = C + A B per block, products added in k-ascending fma order
static void mfma4(const double *A, const double *B, const double *C, double *D) {
    for (int b = 0; b < 4; b++)
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) {
                double d = C[j + 4 * b + 16 * i];
                for (int k = 0; k < 4; k++) d = std::fma(A[i + 4 * b + 16 * k], B[j + 4 * b + 16 * k], d);
                D[j + 4 * b + 16 * i] = d;
            }
}

template <bool FWD>
static double run(int W, uint64_t seed) {
    const int NS = W + 4;
    std::vector<double> F(64 * NS), Fm(64 * NS), c(13 * NS), cb(13 * NS), out(13 * NS, 0.0), ref(13 * NS, 0.0);
    auto rnd = [&]() {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(seed >> 11) / 9007199254740992.0 - 0.5;
    };
    for (double &f : F) f = 0.24 * rnd();
    for (double &v : c) v = rnd();
    for (int k = 0; k < NS; k++)
        for (int r = 0; r < 8; r++)
            for (int cc = 0; cc < 8; cc++) Fm[64 * k + M::f_slot(!(k & 1), r, cc)] = -F[64 * k + 8 * r + cc];
    for (int p = 0; p < 13 * NS; p++) cb[p] = 0.125 * c[p];

    // plain loop
    {
        double v[8], vn[8];
        for (int r = 0; r < 8; r++) v[r] = c[13 * (FWD ? 0 : W) + r];
        for (int m = 0; m < W; m++) {
            const int k = FWD ? m : W - 1 - m, st = FWD ? m + 1 : k;
            for (int r = 0; r < 8; r++) {
                double s = c[13 * st + r];
                for (int cc = 0; cc < 8; cc++) s -= (FWD ? F[64 * k + 8 * r + cc] : F[64 * k + 8 * cc + r]) * v[cc];
                vn[r] = s;
            }
            for (int r = 0; r < 8; r++) ref[13 * st + r] = v[r] = vn[r];
        }
    }
    // the kernel's form on 64 modelled lanes (the chain carries v / 4)
    double v[64], A[64], C[64], D[64], cap[2][2][64] = {};
    for (int l = 0; l < 64; l++) v[l] = 2.0 * cb[13 * (FWD ? 0 : W) + M::in_idx(l, false)];
    for (int m = 0; m < W; m++) {
        const bool odd = m & 1;
        const int k = FWD ? m : W - 1 - m, st = FWD ? m + 1 : k;
        for (int l = 0; l < 64; l++) {
            A[l] = Fm[64 * k + M::a_slot(l, odd, FWD, !(k & 1))];
            C[l] = cb[13 * st + M::out_idx(l, odd)];
        }
        mfma4(A, v, C, D);
        for (int l = 0; l < 64; l++) v[l] = D[l] + D[M::partner(l, odd)];
        const uint64_t keep = M::keep_mask((m >> 1) & 7, odd);
        for (int l = 0; l < 64; l++)
            if ((keep >> l) & 1) cap[odd][m >> 4][l] = v[l];
    }
    int stored = 0;
    for (int l = 0; l < 64; l++)
        for (int q = 0; q < 2; q++)
            for (int odd = 0; odd < 2; odd++) {
                const int m = 16 * q + 2 * M::other(l, odd) + odd;
                if (m >= W) continue;
                out[13 * (FWD ? m + 1 : W - 1 - m) + M::out_idx(l, odd)] = 4.0 * cap[odd][q][l];
                stored++;
            }
    if (stored != 8 * W) return INFINITY;  // every (step, element) kept by exactly one lane
    double mx = 0.0, df = 0.0;
    for (int p = 0; p < 13 * NS; p++) mx = std::fmax(mx, std::fabs(ref[p])), df = std::fmax(df, std::fabs(out[p] - ref[p]));
    return df / mx;
}

int main() {
    // every lane (x, b, q) <-> (other, out_idx) pair is distinct in both parities, and the keep masks
    // select exactly the lanes with that `other`
    for (int odd = 0; odd < 2; odd++) {
        uint64_t seen = 0;
        for (int l = 0; l < 64; l++) {
            seen |= 1ull << (8 * M::other(l, odd) + M::out_idx(l, odd));
            if (((M::keep_mask(M::other(l, odd), odd) >> l) & 1) == 0) return std::printf("keep mask, lane %d\n", l), 1;
            if (M::out_idx(M::partner(l, odd), odd) != M::out_idx(l, odd) || M::bcol(M::partner(l, odd), odd) == M::bcol(l, odd))
                return std::printf("partner, lane %d\n", l), 1;
            if (M::in_idx(l, !odd) != M::out_idx(l, odd)) return std::printf("chain, lane %d\n", l), 1;
        }
        if (~seen) return std::printf("capture lanes not distinct\n"), 1;
        for (int v = 0; v < 8; v++)
            if (__builtin_popcountll(M::keep_mask(v, odd)) != 8) return std::printf("keep mask %d\n", v), 1;
    }
    // bound: W steps of 8-term sums, |F| rows sum below 1, so the two associations differ by at most
    // about 8 W eps of the largest value; 1e-13 leaves a factor of 5 over that for W = 19
    int bad = 0;
    for (int W : {19, 18, 7})
        for (uint64_t seed = 1; seed <= 4; seed++) {
            const double f = run<true>(W, seed), b = run<false>(W, 77 * seed);
            std::printf("W %2d seed %llu: forward %.3e backward %.3e\n", W, (unsigned long long)seed, f, b);
            bad += !(f <= 1e-13) || !(b <= 1e-13);
        }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad != 0;
}
