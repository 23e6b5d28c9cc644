// Lane and block maps of the stage recursions on the four-block FP64 matrix instruction
// v_mfma_f64_4x4x4_4b_f64 (mpc_wave.hpp sweep_mfma).  Plain constexpr integer functions: the kernel
// uses them on the device, tests/native/sweep_mfma_model.cpp checks them on the host against a model
// of the instruction.
//
// Operand layout measured on gfx950 (tools/probe/recur_probe.hip k_layout), lane = x + 4 b + 16 q with
// b the block: A[i][k] of block b sits in lane i + 4 b + 16 k, B[k][j] in lane j + 4 b + 16 k, and
// C[i][j] / D[i][j] in lane j + 4 b + 16 i.  One f64 per lane for each operand; every block computes
// D = C + A B with the four products of an element added in k-ascending fma order.
//
// A step v' = c - M v (M 8x8 as 2x2 blocks of 4x4) is one instruction: block b carries -M's block
// (R, Cc) as A, B is v[4 Cc + k] in every column j, C is half of c[4 R + i] in every column, and
// v'[4 R + i] = D(R, 0) + D(R, 1): one sum over the partner block.
// Even steps number the blocks b = 2 R + Cc: the partner is lane ^ 4 (DPP row_half_mirror; D is the
// same in all four columns) and the sum leaves v'[4 (b >> 1) + q] in lane (x, b, q).  That is the B
// operand of an odd step, whose blocks are numbered b = R + 2 Cc (partner lane ^ 8, DPP row_ror:8)
// and which leaves v'[4 (b & 1) + q]: the even step's B again.  No transpose sits on the chain.
#pragma once
#include <stdint.h>

namespace impc {
namespace mfmap {

constexpr int lx(int l) { return l & 3; }
constexpr int lb(int l) { return (l >> 2) & 3; }
constexpr int lq(int l) { return (l >> 4) & 3; }
// block row R / block column Cc of lane l's block in an even / odd step
constexpr int brow(int l, bool odd) { return odd ? lb(l) & 1 : lb(l) >> 1; }
constexpr int bcol(int l, bool odd) { return odd ? lb(l) >> 1 : lb(l) & 1; }

// slot of F_k[r][c] in stage k's 64 doubles (the recursion layout: even stages transposed)
constexpr int f_slot(bool even_stage, int r, int c) { return even_stage ? 8 * c + r : 8 * r + c; }

// the slot lane l feeds to A: element [4 R + x][4 Cc + q] of F_k (forward) or of F_k' (backward)
constexpr int a_slot(int l, bool odd, bool fwd, bool even_stage) {
    const int row = 4 * brow(l, odd) + lx(l), col = 4 * bcol(l, odd) + lq(l);
    return fwd ? f_slot(even_stage, row, col) : f_slot(even_stage, col, row);
}
// element of v the lane feeds to B; element of c it feeds to C and of v' it holds after the pair sum
constexpr int in_idx(int l, bool odd) { return 4 * bcol(l, odd) + lq(l); }
constexpr int out_idx(int l, bool odd) { return 4 * brow(l, odd) + lq(l); }
// the 8 lanes that hold the same element of v' differ in this index; the lane whose index is
// (m / 2) % 8 keeps step m (the lane grid's capture rule)
constexpr int other(int l, bool odd) { return lx(l) + 4 * bcol(l, odd); }
constexpr uint64_t keep_mask(int v, bool odd) {
    return odd ? 0x0001000100010001ull * (0x11ull << ((v & 3) + 8 * (v >> 2))) : 0x0101010101010101ull << v;
}
// Capture registers of an unrolled sweep of wc steps: step m is kept in register m >> 4 of the even-
// (c0) or odd-step (c1) array, by the lane whose `other` index is (m / 2) % 8.
// cap_step: the step that lane keeps in register q; it exists when it is below wc.
constexpr int cap_step(int q, bool odd, int oth) { return 16 * q + 2 * oth + (odd ? 1 : 0); }
// cap_final: the last step of the sweep that writes register q (-1: none does).  After it the
// register is final in every lane and can be stored while the later steps run.
constexpr int cap_final(int wc, int q, bool odd) {
    const int first = 16 * q + (odd ? 1 : 0), top = first + 14;  // the register's steps: first, first + 2, .. top
    if (first >= wc) return -1;
    return top < wc ? top : wc - 1 - ((wc - 1 - first) & 1);
}
// partner lane of the pair sum
constexpr int partner(int l, bool odd) { return odd ? l ^ 8 : (l & ~7) | (7 - (l & 7)); }

}  // namespace mfmap
}  // namespace impc
