// k2s_tail16_map.h -- index maps of the 16-row form of the screening kernel's shared last row tile (k2s_round.h, fused pass):
// v_mfma_f32_16x16x32_f16 instead of v_mfma_f32_32x32x16_f16 when that tile holds at most 16 atoms.  Plain constexpr
// functions: the kernel and a host program (tests/test_k2s_tail16_host.py) read the same text.
//
// The KS k-steps of 16 measurement rows (MP = 16 KS) become (KS + 1) / 2 steps of 32.  Lane l = 16 g + c (g = l >> 4: lane
// group, c = l & 15) holds, in element j = 0..7 of its A and B fragments of step s, measurement row 32 s + 8 g + j: of atom c
// of the row tile (A), of atom 2 c + t of the 32-atom column tile in sub-tile t (B: one 16-byte table load brings the two
// adjacent atoms, the even one goes to sub-tile 0, the odd one to sub-tile 1).  An odd KS leaves the lane groups 2 and 3 of
// the last step beyond MP: they supply zeros and read no per-row constant.
#pragma once

constexpr int k2s_t16_steps(int KS) { return (KS + 1) / 2; }
// measurement row of element j of lane l in step s; -1: beyond MP = 16 KS (the lane supplies a zero)
constexpr int k2s_t16_row(int l, int j, int s, int KS) {
  const int m = 32 * s + 8 * (l >> 4) + j;
  return m < 16 * KS ? m : -1;
}
// atom of the row tile (0..15) in lane l's A fragment
constexpr int k2s_t16_arow(int l) { return l & 15; }
// atom of the 32-atom column tile in lane l's B fragment of sub-tile t (0: even atoms, 1: odd atoms)
constexpr int k2s_t16_atom(int l, int t) { return 2 * (l & 15) + t; }
// accumulator register r = 0..3 of lane l: row (atom of the row tile) and column (B lane's atom slot) of the 16 x 16 C tile
constexpr int k2s_t16_crow(int l, int r) { return 4 * (l >> 4) + r; }
constexpr int k2s_t16_ccol(int l) { return l & 15; }
