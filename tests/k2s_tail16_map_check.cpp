// Stand-alone check of csrc/k2s_tail16_map.h, the index maps of the screening kernel's 16-row form (host code only, its own
// main; tests/test_k2s_tail16_host.py builds it with -fsanitize=address,undefined and runs it).  For KS = 4, 8, 13, 16:
//   * every (measurement row < MP, atom < 32) of a column tile is produced exactly once over lanes, elements j, steps and
//     sub-tiles, and every (row < MP, atom < 16) of the row tile exactly once over lanes, j and steps;
//   * no row index >= MP is ever formed: a lane beyond MP answers -1, and the constants it then reads (the kernel takes
//     row 32 s + j instead) lie inside MP;
//   * A and B fragments of a lane carry the same measurement rows (the product sums over matching k);
//   * the C map is a bijection onto 16 x 16, rows as the A map's atoms, columns as the B map's lanes;
//   * even atoms land in sub-tile 0, odd atoms in sub-tile 1, adjacent atoms 2c, 2c+1 in the same lane.
#include <cstdio>
#include <vector>

#include "../microstructure_fingerprinting_amd/csrc/k2s_tail16_map.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

static void check(int KS) {
  const int MP = 16 * KS, NS = k2s_t16_steps(KS);
  CHECK(32 * NS >= MP && 32 * (NS - 1) < MP, "KS %d: %d steps", KS, NS);
  std::vector<int> seenB((size_t)MP * 32, 0), seenA((size_t)MP * 16, 0);   // indexed only after the range checks below
  for (int s = 0; s < NS; ++s)
    for (int l = 0; l < 64; ++l) {
      const int m0 = k2s_t16_row(l, 0, s, KS);
      // what the kernel does with the answer: all 8 rows of a lane are in range, or none is
      const int mb = m0 >= 0 ? m0 : 32 * s;
      CHECK(mb >= 0 && mb + 7 < MP, "KS %d step %d lane %d: constants read at rows %d..%d", KS, s, l, mb, mb + 7);
      for (int j = 0; j < 8; ++j) {
        const int m = k2s_t16_row(l, j, s, KS);
        CHECK(m == -1 || (m >= 0 && m < MP), "KS %d step %d lane %d j %d: row %d", KS, s, l, j, m);
        CHECK((m >= 0) == (m0 >= 0), "KS %d step %d lane %d: rows partly in range", KS, s, l);
        if (m >= 0) CHECK(m == m0 + j, "KS %d step %d lane %d j %d: rows not consecutive", KS, s, l, j);
        if (m < 0 || m >= MP) continue;
        const int ar = k2s_t16_arow(l);
        CHECK(ar >= 0 && ar < 16, "A atom %d", ar);
        if (ar >= 0 && ar < 16) ++seenA[(size_t)m * 16 + ar];
        for (int t = 0; t < 2; ++t) {
          const int at = k2s_t16_atom(l, t);
          CHECK(at >= 0 && at < 32, "B atom %d", at);
          CHECK((at & 1) == t, "lane %d sub-tile %d holds atom %d", l, t, at);
          if (at >= 0 && at < 32) ++seenB[(size_t)m * 32 + at];
        }
      }
      CHECK(k2s_t16_atom(l, 1) == k2s_t16_atom(l, 0) + 1 && (k2s_t16_atom(l, 0) & 1) == 0, "lane %d: atoms not an adjacent even/odd pair", l);
    }
  for (int m = 0; m < MP; ++m) {
    for (int n = 0; n < 32; ++n) CHECK(seenB[(size_t)m * 32 + n] == 1, "KS %d: B (row %d, atom %d) produced %d times", KS, m, n, seenB[(size_t)m * 32 + n]);
    for (int n = 0; n < 16; ++n) CHECK(seenA[(size_t)m * 16 + n] == 1, "KS %d: A (row %d, atom %d) produced %d times", KS, m, n, seenA[(size_t)m * 16 + n]);
  }
  // C: register r of lane l -> (row, column); rows are A atoms, columns the B lanes' slots
  int seenC[16][16] = {};
  for (int l = 0; l < 64; ++l)
    for (int r = 0; r < 4; ++r) {
      const int row = k2s_t16_crow(l, r), col = k2s_t16_ccol(l);
      CHECK(row >= 0 && row < 16 && col >= 0 && col < 16, "C (%d, %d)", row, col);
      if (row >= 0 && row < 16 && col >= 0 && col < 16) ++seenC[row][col];
      CHECK(col == (l & 15) && row == 4 * (l >> 4) + r, "C map of lane %d register %d", l, r);
      // the lane that owns column `col` of C owns atoms 2 col, 2 col + 1 of the column tile in B
      CHECK(k2s_t16_atom(l, 0) == 2 * col && k2s_t16_atom(l, 1) == 2 * col + 1, "lane %d: C column %d against B atoms", l, col);
    }
  for (int r = 0; r < 16; ++r)
    for (int c = 0; c < 16; ++c) CHECK(seenC[r][c] == 1, "C (%d, %d) held %d times", r, c, seenC[r][c]);
}

// the maps are usable in constant expressions (the kernel takes its step count from one)
static_assert(k2s_t16_steps(13) == 7 && k2s_t16_steps(4) == 2 && k2s_t16_steps(16) == 8, "step counts");
static_assert(k2s_t16_row(32, 0, 6, 13) == -1 && k2s_t16_row(31, 7, 6, 13) == 207, "KS = 13: the half-empty last step");

int main() {
  for (int KS : {4, 8, 13, 16}) check(KS);
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("ok\n");
  return 0;
}
