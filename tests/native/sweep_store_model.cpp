// Host model of the capture registers of the unrolled stage sweeps (csrc/mpc_wave.hpp sweep_run) and of
// the stores that leave them: step m's result is kept under mfmap::keep_mask in register m >> 4 of the
// even- or odd-step array (the register's first step is a plain copy in every lane), and each register
// is stored behind the last step that writes it (mfmap::cap_final), by the lane that keeps the step
// mfmap::cap_step names, the other lanes to their discard slot.  Checked for a sweep of WC steps:
// cap_final is exact, and the early stores write every (stage, element) slot once, with the value of the
// step that owns the stage.  Stand-alone (own main), host only.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../intent-mpc_amd/csrc/sweep_mfma_map.hpp"

namespace M = impc::mfmap;

// the value step m leaves in a lane that holds element e of its result (never 0: 0 is "unwritten")
static int token(int m, int e) { return 8 * m + e + 1; }

template <bool FWD>
static int run(int WC) {
    const int CQ = WC / 16 + 1;
    std::vector<int> reg(2 * CQ * 64, 0);          // [odd][q][lane]
    std::vector<int> last(2 * CQ, -1);             // last step that wrote register (odd, q) in any lane
    std::vector<int> slot(13 * (WC + 1), 0), writes(13 * (WC + 1), 0);
    int junk = 0, stored_regs = 0;
    auto stage = [&](int m) { return FWD ? m + 1 : WC - 1 - m; };
    auto store = [&](int odd, int q, int after) {
        // no later step may write a register that has been stored
        for (int m = after + 1; m < WC; m++)
            if ((m >> 4) == q && (m & 1) == odd) return std::printf("WC %d: step %d writes a stored register\n", WC, m), 1;
        for (int l = 0; l < 64; l++) {
            const int m = M::cap_step(q, odd, M::other(l, odd));
            if (m >= WC) { junk++; continue; }
            const int p = 13 * stage(m) + M::out_idx(l, odd);
            slot[p] = reg[(odd * CQ + q) * 64 + l];
            writes[p]++;
        }
        stored_regs++;
        return 0;
    };
    for (int m = 0; m < WC; m++) {
        const int odd = m & 1, q = m >> 4;
        const uint64_t keep = (m & 14) == 0 ? ~0ull : M::keep_mask((m >> 1) & 7, odd);
        for (int l = 0; l < 64; l++)
            if ((keep >> l) & 1) reg[(odd * CQ + q) * 64 + l] = token(m, M::out_idx(l, odd));
        last[odd * CQ + q] = m;
        if (m == M::cap_final(WC, q, odd) && store(odd, q, m)) return 1;
    }
    for (int q = 0; q < CQ; q++)
        for (int odd = 0; odd < 2; odd++) {
            // exact: the step named is the last one that writes the register (-1: none does)
            if (M::cap_final(WC, q, odd) != last[odd * CQ + q])
                return std::printf("WC %d: cap_final(%d, %d) = %d, last write %d\n", WC, q, odd, M::cap_final(WC, q, odd),
                                   last[odd * CQ + q]), 1;
            if (M::cap_final(WC, q, odd) < 0) {  // stored after the sweep: owns no element
                for (int l = 0; l < 64; l++)
                    if (M::cap_step(q, odd, M::other(l, odd)) < WC) return std::printf("WC %d: unwritten register owns a step\n", WC), 1;
                junk += 64, stored_regs++;
            }
        }
    if (stored_regs != 2 * CQ) return std::printf("WC %d: %d of %d registers stored\n", WC, stored_regs, 2 * CQ), 1;
    // every stage the sweep produces: its 8 elements written once, by the step that owns the stage
    int covered = 0;
    for (int m = 0; m < WC; m++)
        for (int e = 0; e < 8; e++) {
            const int p = 13 * stage(m) + e;
            if (writes[p] != 1 || slot[p] != token(m, e))
                return std::printf("WC %d %s: stage %d element %d written %d times, value %d, want %d\n", WC,
                                   FWD ? "forward" : "backward", stage(m), e, writes[p], slot[p], token(m, e)), 1;
            covered++;
        }
    int total = 0;
    for (int w : writes) total += w;
    if (total != covered || total + junk != 2 * CQ * 64)
        return std::printf("WC %d: %d element stores, %d discarded, %d slots\n", WC, total, junk, covered), 1;
    return 0;
}

int main() {
    int bad = 0;
    for (int WC : {19, 1, 2, 16, 17, 18}) {
        const int f = run<true>(WC), b = run<false>(WC);
        std::printf("WC %2d: final steps c0 %d %d c1 %d %d  %s\n", WC, M::cap_final(WC, 0, false), M::cap_final(WC, 1, false),
                    M::cap_final(WC, 0, true), M::cap_final(WC, 1, true), f || b ? "FAILED" : "ok");
        bad += f || b;
    }
    static_assert(M::cap_final(19, 0, false) == 14 && M::cap_final(19, 0, true) == 15, "the default horizon's early stores");
    static_assert(M::cap_final(19, 1, false) == 18 && M::cap_final(19, 1, true) == 17, "");
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad != 0;
}
