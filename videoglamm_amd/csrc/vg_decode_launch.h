// Launch geometry of the decode step's GEMV launchers (vg_decode.hip, vg_decode_w4.hip, vg_decode_mfma.hip, vg_decode2.hip): how row pairs are
// split over waves and workgroups, and the B-row bucket ladder.  Host code only, plain C++17, no HIP types: tests/decode_launch_split_main.cpp
// builds it with the host compiler alone.  The B-row kernels are built so that which wave owns which pair does not enter the sums — a wrong split
// passes every bit-identity test and only costs time, so it is written once, here, and pinned by tests/test_decode_launch_split.py.
#pragma once
#include <type_traits>
#include <utility>

struct DecSplit { int ppw, blocks; };      // row pairs per wave; workgroups of four waves

// Single-row GEMVs.  The pairs are spread over at most wg_per_cu workgroups on each of the 256 CUs: 2 = what is resident of the bf16 / 13-bit /
// q|k|v-rope kernels and the chained roles (254 VGPRs; with 4 the q|k|v projection ran 768 workgroups in one and a half rounds, r03: 3.23 ->
// 3.205 ms per token on C2), 4 for the fp8 and MXFP4 kernels.  Preferred: a split of whole rounds of 256 workgroups (every CU the same number).
// max_ppw: the kernel's res[] rows (DEC_MAX_PPW / DEC4_MAX_PPW).
inline DecSplit dec_pair_split(int npair, int wg_per_cu, int max_ppw) {
  const int maxw = 256 * wg_per_cu * 4;
  int ppw = (npair + maxw - 1) / maxw;
  for (int c = ppw; c <= 2 * ppw; ++c)
    if (((npair + 4 * c - 1) / (4 * c)) % 256 == 0 && npair % (4 * c) == 0) { ppw = c; break; }
  if (ppw > max_ppw) ppw = max_ppw;
  return {ppw, (npair + 4 * ppw - 1) / (4 * ppw)};
}

// B-row GEMVs: ~2 workgroups per CU, as the single-row bf16 kernel; phased (the x rows are staged in phases of K): one pair per wave.
// max_ppw: DEC_ROWS_PPW / DEC4_ROWS_PPW.
inline DecSplit dec_rows_split(int npair, bool phased, int max_ppw) {
  int ppw = (npair + 2047) / 2048;
  ppw = phased ? 1 : (ppw < max_ppw ? ppw : max_ppw);
  return {ppw, (npair + 4 * ppw - 1) / (4 * ppw)};
}

// The B-row kernels are built for BR = 1, 2, 4, 8, 16 rows: B rows run on the smallest bucket that holds them (and stage that many rows of x).
inline bool dec_rows_b_ok(int B) { return B >= 1 && B <= 16; }
inline int dec_bucket(int B) { return B <= 1 ? 1 : B <= 2 ? 2 : B <= 4 ? 4 : B <= 8 ? 8 : 16; }

// f(std::integral_constant<int, dec_bucket(B)>{}): the bucket as a compile-time BR
template <typename F>
inline auto dec_with_bucket(int B, F&& f) {
  switch (dec_bucket(B)) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 16>{});
  }
}
