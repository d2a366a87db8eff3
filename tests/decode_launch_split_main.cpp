// Prints the decode launchers' work split for tests/test_decode_launch_split.py: one "ppw blocks" line per case, in the order that test walks.
// Host C++17 only: vg_decode_launch.h is what the launchers (vg_decode.hip, vg_decode_w4.hip) call.
#include <cstdio>

#include "../videoglamm_amd/csrc/vg_decode_launch.h"

int main() {
  const int NPAIR = 66000;
  const int caps[3] = {64 /* DEC_MAX_PPW */, 64 /* DEC4_MAX_PPW */, 8 /* a cap that binds */};
  for (int wg = 2; wg <= 4; wg += 2)
    for (int cap : caps)
      for (int n = 1; n <= NPAIR; ++n) {
        const DecSplit s = dec_pair_split(n, wg, cap);
        std::printf("%d %d\n", s.ppw, s.blocks);
      }
  for (int phased = 0; phased <= 1; ++phased)
    for (int n = 1; n <= NPAIR; ++n) {
      const DecSplit s = dec_rows_split(n, phased != 0, 8 /* DEC_ROWS_PPW = DEC4_ROWS_PPW */);
      std::printf("%d %d\n", s.ppw, s.blocks);
    }
  int ladder[17] = {0};
  for (int B = 1; B <= 16; ++B) {
    std::printf("%d\n", dec_bucket(B));
    ladder[B] = dec_with_bucket(B, [](auto br) { return decltype(br)::value; });
  }
  for (int B = 1; B <= 16; ++B)
    if (ladder[B] != dec_bucket(B) || !dec_rows_b_ok(B)) return 1;      // the compile-time ladder is the value ladder
  return dec_rows_b_ok(0) || dec_rows_b_ok(17) ? 1 : 0;
}
