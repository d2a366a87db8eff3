// Operand layout probe for v_mfma_scale_f32_32x32x64_f8f6f4 with MIXED operands on gfx950: A = fp8 e4m3 (cbsz 0, 8 VGPRs), B = fp4 e2m1 (blgp 4,
// 4 VGPRs), B with an e8m0 block scale per lane.  It assumes nothing about the layout: the kernel takes the register image of every lane and returns
// the raw accumulator registers, and the host finds the maps with one-hot operands.
//   part 1  the C layout: which (lane, register) of the result belongs to A-lane La and to B-lane Lb
//   part 2  the pairing: byte q of A's 32 (lanes of half hA) meets nibble p of B's 32 (lanes of half hB) exactly where their k agree — the matrix of
//           (hA, q) x (hB, p) products is counted against the layout stated below and, where it differs, printed as the list of pairs (nibble p = 2 byte + (0 low | 1 high))
//   part 3  the scale: which byte of the lane's scale register op_sel = 0..3 picks, and whether the two k halves of a row take their own lane's
//           register (per lane = per 32-element block) or one lane's for both; what the scale byte 0 means to the hardware
//   part 4  with the answers of 1-3: random exact operands in the derived layout against a host reference (== on all 1024 results)
// Measured on an MI355X: C has the layout of the other 32x32 MFMAs (register i of lane l = C[A row (i&3) + 8 (i>>2) + 4 (l>>5)][B row l & 31]); the fp4 lane
// (row, h) holds the 32 consecutive k [32h, 32h + 32) — one MX block — element 2j in the low nibble of byte j; the fp8 lane (row, h) holds k [16h, 16h + 16)
// in VGPR 0-3 and k [32 + 16h, 32 + 16h + 16) in VGPR 4-7; op_sel = j picks byte j of the lane's scale register and the scale applies to that lane's own
// 32 nibbles; the scale byte 0 is 2^-127, not zero.
//   hipcc -O3 --offload-arch=gfx950 tools/f8f4_mfma_layout.hip -o f8f4l && ./f8f4l
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <cmath>
typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

__global__ void k(const uint32_t* RA, const uint32_t* RB, const uint32_t* S, float* out, int opsel) {
  const int lane = threadIdx.x;
  i32x8_t va, vb;
  for (int v = 0; v < 8; ++v) { va[v] = (int)RA[lane * 8 + v]; vb[v] = v < 4 ? (int)RB[lane * 4 + v] : 0; }
  f32x16_t acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int sb = (int)S[lane];
  switch (opsel) {
    case 0: acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, vb, acc, 0, 4, 0, 0x7f7f7f7f, 0, sb); break;
    case 1: acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, vb, acc, 0, 4, 0, 0x7f7f7f7f, 1, sb); break;
    case 2: acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, vb, acc, 0, 4, 0, 0x7f7f7f7f, 2, sb); break;
    default: acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(va, vb, acc, 0, 4, 0, 0x7f7f7f7f, 3, sb); break;
  }
  for (int i = 0; i < 16; ++i) out[lane * 16 + i] = acc[i];
}

static uint32_t hRA[64 * 8], hRB[64 * 4], hS[64];
static float hOut[64 * 16];
static uint32_t *dRA, *dRB, *dS;
static float* dOut;
static void run(int opsel = 0) {
  (void)hipMemcpy(dRA, hRA, sizeof(hRA), hipMemcpyHostToDevice);
  (void)hipMemcpy(dRB, hRB, sizeof(hRB), hipMemcpyHostToDevice);
  (void)hipMemcpy(dS, hS, sizeof(hS), hipMemcpyHostToDevice);
  k<<<1, 64>>>(dRA, dRB, dS, dOut, opsel);
  if (hipMemcpy(hOut, dOut, sizeof(hOut), hipMemcpyDeviceToHost) != hipSuccess) { printf("device error\n"); exit(1); }
}
static void unit_scales() { for (int i = 0; i < 64; ++i) hS[i] = 0x7f7f7f7fu; }

int main() {
  (void)hipMalloc(&dRA, sizeof(hRA)); (void)hipMalloc(&dRB, sizeof(hRB)); (void)hipMalloc(&dS, sizeof(hS)); (void)hipMalloc(&dOut, sizeof(hOut));
  uint8_t* bA = (uint8_t*)hRA;      // [64 lanes][32 bytes]
  uint8_t* bB = (uint8_t*)hRB;      // [64 lanes][16 bytes]
  // ---- part 1: C layout.  rowmap[lane][reg] = the A row (lane % 32 of the A-lane that reaches it), colmap likewise for B
  int rowmap[64][16], colmap[64][16];
  memset(rowmap, -1, sizeof(rowmap)); memset(colmap, -1, sizeof(colmap));
  unit_scales();
  int clash = 0;
  for (int L = 0; L < 64; ++L) {
    memset(hRA, 0, sizeof(hRA)); memset(hRB, 0x22, sizeof(hRB));      // B: 1.0 everywhere
    memset(bA + L * 32, 0x38, 32);                                     // A: 1.0 in lane L only
    run();
    for (int l = 0; l < 64; ++l) for (int i = 0; i < 16; ++i) if (hOut[l * 16 + i] != 0.f) { clash += rowmap[l][i] >= 0 && rowmap[l][i] != L % 32; rowmap[l][i] = L % 32; }
    memset(hRA, 0x38, sizeof(hRA)); memset(hRB, 0, sizeof(hRB));
    memset(bB + L * 16, 0x22, 16);
    run();
    for (int l = 0; l < 64; ++l) for (int i = 0; i < 16; ++i) if (hOut[l * 16 + i] != 0.f) { clash += colmap[l][i] >= 0 && colmap[l][i] != L % 32; colmap[l][i] = L % 32; }
  }
  int std_layout = 0;
  for (int l = 0; l < 64; ++l) for (int i = 0; i < 16; ++i) std_layout += rowmap[l][i] == (i & 3) + 8 * (i >> 2) + 4 * (l >> 5) && colmap[l][i] == (l & 31);
  printf("part 1: lanes L and L + 32 feed one row / column (clashes: %d); C register i of lane l = C[A row (i&3) + 8 (i>>2) + 4 (l>>5)][B row l & 31] holds at %d of 1024 places\n",
         clash, std_layout);
  printf("        lane 0: A rows"); for (int i = 0; i < 16; ++i) printf(" %d", rowmap[0][i]); printf(" | B row %d;   lane 33: A rows", colmap[0][0]);
  for (int i = 0; i < 16; ++i) printf(" %d", rowmap[33][i]); printf(" | B row %d\n", colmap[33][0]);

  // ---- part 2: pairing of A byte (hA, q) with B nibble (hB, p); nibble p = 2 * byte + (0 low, 1 high)
  int ident = 0, npairs = 0, bad_uniform = 0;
  static int partner[2][32][2];      // for B (hB, p): the (hA, q) it meets
  memset(partner, -1, sizeof(partner));
  for (int hB = 0; hB < 2; ++hB)
    for (int p = 0; p < 32; ++p) {
      memset(hRB, 0, sizeof(hRB));
      for (int l = 32 * hB; l < 32 * hB + 32; ++l) bB[l * 16 + p / 2] = (p & 1) ? 0x20 : 0x02;
      for (int hA = 0; hA < 2; ++hA)
        for (int q = 0; q < 32; ++q) {
          memset(hRA, 0, sizeof(hRA));
          for (int l = 32 * hA; l < 32 * hA + 32; ++l) bA[l * 32 + q] = 0x38;
          run();
          int nz = 0;
          for (int j = 0; j < 1024; ++j) nz += hOut[j] == 1.f;
          if (nz == 1024) { ++npairs; partner[hB][p][0] = hA; partner[hB][p][1] = q; ident += 32 * hB + p == (q < 16 ? 16 * hA + q : 32 + 16 * hA + q - 16); }
          else if (nz != 0) ++bad_uniform;
        }
    }
  printf("part 2: %d (A byte, B nibble) pairs meet (64 expected), %d of them where B's lane half hB holds k [32 hB, 32 hB + 32) (nibble p = k - 32 hB, element 2j in\n"
         "        the LOW nibble of byte j) and A's lane half hA holds k [16 hA, 16 hA + 16) in VGPR 0-3 and k [32 + 16 hA, 32 + 16 hA + 16) in VGPR 4-7;\n"
         "        launches with a partly non-zero C: %d\n", npairs, ident, bad_uniform);
  if (ident != 64)
    for (int hB = 0; hB < 2; ++hB) { printf("        B half %d nibble p -> A (half, byte):", hB); for (int p = 0; p < 32; ++p) printf(" %d:%d", partner[hB][p][0], partner[hB][p][1]); printf("\n"); }

  // ---- part 3: scales.  A, B = 1.0 everywhere; byte j of lane l's register = 127 + (j + l % 32) % 4 + 4 (l / 32): C = 32 (2^e_lo + 2^e_hi), e_lo in 0..3,
  // e_hi in 4..7 when each half takes its own lane's register
  memset(hRA, 0x38, sizeof(hRA)); memset(hRB, 0x22, sizeof(hRB));
  for (int l = 0; l < 64; ++l) { hS[l] = 0; for (int j = 0; j < 4; ++j) hS[l] |= (uint32_t)(127 + (j + l % 32) % 4 + 4 * (l / 32)) << (8 * j); }
  for (int opsel = 0; opsel < 4; ++opsel) {
    run(opsel);
    int per_lane[4] = {0, 0, 0, 0}, other = 0;
    for (int l = 0; l < 64; ++l)
      for (int i = 0; i < 16; ++i) {
        const int n = colmap[l][i] >= 0 ? colmap[l][i] : (l & 31);
        bool hit = false;
        for (int j = 0; j < 4; ++j)
          if (hOut[l * 16 + i] == 32.f * (ldexpf(1.f, (j + n) % 4) + ldexpf(1.f, (j + n) % 4 + 4))) { ++per_lane[j]; hit = true; }
        other += !hit;
      }
    printf("part 3: op_sel %d: C = 32 (2^s(lane n, byte j) + 2^s(lane n + 32, byte j)) at byte j = 0..3: %d %d %d %d of 1024; neither: %d (first value %g)\n", opsel,
           per_lane[0], per_lane[1], per_lane[2], per_lane[3], other, hOut[0]);
  }
  // whose scale does a nibble get: B = one nibble p of the lanes of half hB, A = 1.0 everywhere, the scale 2^(1 + l / 32) in lane l: C = 2 (own lane's) or 4
  for (int l = 0; l < 64; ++l) hS[l] = 128u + (uint32_t)(l / 32);
  int own = 0, all = 0;
  for (int hB = 0; hB < 2; ++hB)
    for (int p = 0; p < 32; ++p) {
      memset(hRB, 0, sizeof(hRB));
      for (int l = 32 * hB; l < 32 * hB + 32; ++l) bB[l * 16 + p / 2] = (p & 1) ? 0x20 : 0x02;
      run();
      for (int j = 0; j < 1024; ++j) { ++all; own += hOut[j] == (hB ? 4.f : 2.f); }
    }
  printf("part 3: a lane's scale applies to that lane's own 32 nibbles (one MX block of its row) at %d of %d results\n", own, all);
  memset(hRB, 0x22, sizeof(hRB));
  unit_scales();
  hS[0] = hS[32] = 0u;
  run();
  printf("part 3: scale byte 0 in lanes 0 and 32: C[.][B row 0] = %g (64 * 2^-127 = %g: the hardware reads e8m0, the packed rows want 0)\n", hOut[0], 64.0 * ldexp(1.0, -127));

  // ---- part 4: random exact operands in the layout of parts 2 and 3 (scale in byte 0, junk above), C by part 1's standard layout
  const uint8_t c8[4] = {0x38, 0x40, 0xB8, 0x48};      // 1, 2, -1, 4 in e4m3
  const float v8[4] = {1.f, 2.f, -1.f, 4.f};
  const uint8_t c4[4] = {0x2, 0x4, 0xA, 0x5};          // 1, 2, -1, 3 in e2m1
  const float v4[4] = {1.f, 2.f, -1.f, 3.f};
  static float fA[32][64], fB[32][64];
  srand(1);
  memset(hRB, 0, sizeof(hRB));
  for (int r = 0; r < 32; ++r)
    for (int kk = 0; kk < 64; ++kk) {
      const int a = rand() & 3, b = rand() & 3, l = r + 32 * (kk / 32), e = kk % 32;
      fA[r][kk] = v8[a]; bA[(r + 32 * ((kk / 16) & 1)) * 32 + 16 * (kk / 32) + kk % 16] = c8[a];
      fB[r][kk] = v4[b]; bB[l * 16 + e / 2] |= (uint8_t)(c4[b] << (4 * (e & 1)));
    }
  for (int l = 0; l < 64; ++l) hS[l] = 127u + (uint32_t)((l % 32 + 2 * (l / 32)) % 4) + 0x55443300u;      // byte 0 = the block's scale, junk above
  run(0);
  int bad = 0;
  for (int l = 0; l < 64; ++l)
    for (int i = 0; i < 16; ++i) {
      const int m = (i & 3) + 8 * (i >> 2) + 4 * (l >> 5), n = l & 31;
      double s = 0.0;
      for (int kk = 0; kk < 64; ++kk) s += (double)fA[m][kk] * fB[n][kk] * ldexp(1.0, (n + 2 * (kk / 32)) % 4);
      bad += !(hOut[l * 16 + i] == (float)s);
    }
  printf("part 4: random operands in that layout, a scale per (B row, 32-element block): %d mismatches of 1024\n", bad);
  return 0;
}
