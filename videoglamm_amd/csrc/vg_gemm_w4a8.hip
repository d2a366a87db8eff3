// vg_gemm_w4a8: C[m,n] = a_scale[m] * sum_k e4m3(A8[m,k]) * 2^(s[n, k/32] - 127) * e2m1(W4[n,k])  (+ R[m,n])   (include/vg_kernels.h)
// The prefill GEMM of cfg prefill_gemm = "mxfp4": per-token e4m3 activations (vg_quantize_fp8_rows) against the PACKED MXFP4 rows the decode step streams
// (ops.mxfp4_pack: a head of 64 * SPL scale bytes, then K / 2 code bytes), read in place: codes by LDS-DMA, scales by byte loads from the head.
//
// Built on the byte instantiation of gemm_tile_glds_kernel (vg_gemm.hip): 128x128 tile, 4 waves of 64x64, 16-byte LDS-DMA with the swizzle applied to the
// SOURCE chunk, two stages, one barrier per K step of 128 elements.  A stages 128 rows x 128 bytes exactly as there (slot = chunk ^ ((row >> 1) & 7)); W
// stages 128 rows x 64 code bytes: 16 rows per wave DMA instruction, slot = chunk ^ ((row >> 2) & 3) (the 64-byte-row swizzle of gemm_tile_k64b_kernel).
//
// v_mfma_scale_f32_32x32x64_f8f6f4 with A = e4m3 (cbsz 0, unit scale 0x7f) and B = e2m1 (blgp 4) — the lane map, measured with tools/f8f4_mfma_layout.hip:
//   C        the layout of every 32x32 MFMA: register i of lane l = C[A row (i & 3) + 8 (i >> 2) + 4 (l >> 5)][B row l & 31]
//   B (fp4)  lane (row n, half h = l >> 5) holds the 32 CONSECUTIVE k [32h, 32h + 32) of its row in 4 VGPRs = one MX block = one 16-byte chunk of the packed
//            row, element 2j in the low nibble of byte j: the packed rows' own order, no shuffle
//   A (fp8)  lane (row m, half h) holds k [16h, 16h + 16) in VGPR 0-3 and k [32 + 16h, 32 + 16h + 16) in VGPR 4-7: of the four 16-byte chunks of a 64-element
//            group G, chunks 4G + h and 4G + 2 + h (what vg_gemm_f8 loads, there for both operands)
//   scale    op_sel = j picks byte j of the lane's scale VGPR; the scale of lane (n, h) applies to that lane's own 32 nibbles, i.e. to block 2G + h of row n.
//            The kernel keeps each scale byte in a register of its own (a zero-extended byte load) and passes op_sel 0.
//   byte 0   the hardware reads it as 2^-127.  Every MXFP4 entry point of this library reads it as "the block is zero", so the fragment's four code
//            registers are replaced by zeros where the byte is 0 (one compare, four selects).
// The scales of K step kt + 1 are requested while step kt multiplies: 4 byte loads per lane and step (2 W rows x 2 groups) from the head, byte
// ((b & 63) * SPL + (b >> 6)) for block b = 4 kt + 2G + h.  No second copy of codes or scales exists.
// Epilogue: the wave's 64x64 fp32 tile through LDS (as gemm_epilogue128), then row-major: * a_scale[m], + R, or SwiGLU over the gate / up wave pair.
#include "vg_gemm_common.h"

struct W4A8Args {
  const uint8_t* A; const float* sa; const uint8_t* W; void* C; const void* R;
  int64_t lda, ldw, ldc, ldr;
  int M, N, K, a_op, gn, spl_sh;      // spl_sh = log2(SPL): the head is 64 << spl_sh bytes
};

__device__ __forceinline__ i32x8_t w4_operand(const u32x4_t& c, uint32_t sbyte) {
  const bool z = sbyte == 0u;
  i32x8_t v = {z ? 0 : (int)c[0], z ? 0 : (int)c[1], z ? 0 : (int)c[2], z ? 0 : (int)c[3], 0, 0, 0, 0};
  return v;
}

template <typename TO>
__global__ __launch_bounds__(256) void gemm_w4a8_kernel(W4A8Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILEA = 128 * 128, TILEW = 128 * 64, STAGE = TILEA + TILEW;
  constexpr int BM = 128, BN = 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, h = lane >> 5;
  const int nwg = gridDim.x * gridDim.y, lin = blockIdx.y * gridDim.x + blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = lin & 7;
  const int wgid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (lin >> 3);
  int bm, bn;
  gemm_tile_of(wgid, gridDim.y, gridDim.x, p.gn, bm, bn);
  const int M = p.M, N = p.N, K = p.K;
  const int head = 64 << p.spl_sh;
  // tile row (0..127) of W -> row of the packed matrix.  a_op 1: 64 gate rows then the 64 up rows of the SAME 64 outputs (W = [gate; up], 2N rows)
  auto wrow = [&](int row) -> int64_t {
    if (p.a_op == 1) {
      const int o = bn * 64 + (row & 63), oc = o < N ? o : N - 1;
      return row < 64 ? oc : N + oc;
    }
    const int gn = bn * BN + row;
    return gn < N ? gn : N - 1;
  };
  const uint8_t* asrc[4];
  const uint8_t* wsrc[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {        // wave w stages A rows [32w, 32w + 32): 4 DMA instructions of 8 rows x 128 bytes
    const int row = wave * 32 + i * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((row >> 1) & 7);
    int gm = bm * BM + row;
    gm = gm < M ? gm : M - 1;
    asrc[i] = p.A + (int64_t)gm * p.lda + chunk * 16;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {        // and W rows [32w, 32w + 32): 2 DMA instructions of 16 rows x 64 code bytes
    const int row = wave * 32 + i * 16 + (lane >> 2);
    const int chunk = (lane & 3) ^ ((row >> 2) & 3);
    wsrc[i] = p.W + wrow(row) * p.ldw + head + chunk * 16;
  }
  auto issue = [&](int kt, int buf) {
    char* sa = smem + buf * STAGE + wave * 32 * 128;
    char* sb = smem + buf * STAGE + TILEA + wave * 32 * 64;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[i] + (int64_t)kt * 128),
                                       (__attribute__((address_space(3))) void*)(sa + i * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc[i] + (int64_t)kt * 64),
                                       (__attribute__((address_space(3))) void*)(sb + i * 1024), 16, 0, 0);
  };
  // fragment rows: A rows ra, ra + 32 and W rows rb, rb + 32 of the tile (the swizzle keys of r and r + 32 agree)
  const int ra = wm * 64 + l31, rb = wn * 64 + l31;
  const int swa = (ra >> 1) & 7, swb = (rb >> 2) & 3;
  const uint8_t* srow[2] = {p.W + wrow(rb) * p.ldw, p.W + wrow(rb + 32) * p.ldw};
  auto load_scales = [&](int kt, uint32_t (&s)[2][2]) {
#pragma unroll
    for (int G = 0; G < 2; ++G) {
      const int b = 4 * kt + 2 * G + h;
      const int off = ((b & 63) << p.spl_sh) + (b >> 6);
      s[0][G] = srow[0][off];
      s[1][G] = srow[1][off];
    }
  };

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = K / 128;
  uint32_t sc[2][2], scn[2][2];
  issue(0, 0);
  load_scales(0, sc);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) {
      issue(kt + 1, buf ^ 1);
      load_scales(kt + 1, scn);
    }
    const char* sa = smem + buf * STAGE + ra * 128;
    const char* sb = smem + buf * STAGE + TILEA + rb * 64;
    u32x4_t fa0[4], fa1[4], fb0[2], fb1[2];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = 2 * g + h;
      fa0[g] = *(const u32x4_t*)(sa + ((c ^ swa) << 4));
      fa1[g] = *(const u32x4_t*)(sa + 32 * 128 + ((c ^ swa) << 4));
    }
#pragma unroll
    for (int G = 0; G < 2; ++G) {
      const int c = 2 * G + h;
      fb0[G] = *(const u32x4_t*)(sb + ((c ^ swb) << 4));
      fb1[G] = *(const u32x4_t*)(sb + 32 * 64 + ((c ^ swb) << 4));
    }
#pragma unroll
    for (int G = 0; G < 2; ++G) {
      const i32x8_t a0 = f8_operand(fa0[2 * G], fa0[2 * G + 1]), a1 = f8_operand(fa1[2 * G], fa1[2 * G + 1]);
      const i32x8_t b0 = w4_operand(fb0[G], sc[0][G]), b1 = w4_operand(fb1[G], sc[1][G]);
      acc[0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a0, b0, acc[0][0], 0, 4, 0, 0x7f7f7f7f, 0, (int)sc[0][G]);
      acc[0][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a0, b1, acc[0][1], 0, 4, 0, 0x7f7f7f7f, 0, (int)sc[1][G]);
      acc[1][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a1, b0, acc[1][0], 0, 4, 0, 0x7f7f7f7f, 0, (int)sc[0][G]);
      acc[1][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a1, b1, acc[1][1], 0, 4, 0, 0x7f7f7f7f, 0, (int)sc[1][G]);
    }
    if (kt + 1 < nk) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int G = 0; G < 2; ++G) sc[i][G] = scn[i][G];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- epilogue: the wave's raw 64x64 tile through LDS (the stages are done with), then every lane owns 8 consecutive columns of a row
  constexpr int ES = 68;
  float* ws = (float*)smem + wave * 64 * ES;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) ws[(i * 32 + mfma32_row(r, h)) * ES + j * 32 + l31] = acc[i][j][r];
  __syncthreads();
  TO* C = (TO*)p.C;
  const TO* R = (const TO*)p.R;
  const int cg = lane & 7, rsub = lane >> 3;
  const int m0w = bm * BM + wm * 64;
  const int n0 = (p.a_op == 1 ? bn * 64 : bn * BN + wn * 64) + cg * 8;
  if (n0 >= N) return;                               // N % 8 == 0: a lane's 8 columns are all inside or all outside
  auto store8 = [&](TO* cp, const float (&v)[8]) {
    if constexpr (sizeof(TO) == 2) {
      u32x4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f2bf2(v[2 * e], v[2 * e + 1]);
      *(u32x4_t*)cp = o;
    } else {
      const f32x4_t o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
      *(f32x4_t*)cp = o0;
      *(f32x4_t*)(cp + 4) = o1;
    }
  };
  if (p.a_op == 1) {
    // SwiGLU: waves (wm, 0) / (wm, 1) staged the gate / up halves of the same 64 outputs; each finishes 32 of the 64 rows:
    // y = round(silu(round(gate))) * round(up) in the output dtype — vg_gemm_f8's epilogue, the arithmetic of vg_swiglu on the rounded GEMM outputs
    const float* wg = (const float*)smem + (wm * 2) * 64 * ES;
    const float* wu = wg + 64 * ES;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int ml = wn * 32 + pass * 8 + rsub, m = m0w + ml;
      if (m >= M) continue;
      const float sr = p.sa[m];
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float g = wg[ml * ES + cg * 8 + e] * sr, u = wu[ml * ES + cg * 8 + e] * sr;
        if (sizeof(TO) == 2) { g = bf2f(f2bf(g)); u = bf2f(f2bf(u)); }
        g = vg_silu(g);
        if (sizeof(TO) == 2) g = bf2f(f2bf(g));
        v[e] = g * u;
      }
      store8(C + (int64_t)m * p.ldc + n0, v);
    }
    return;
  }
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    const int ml = pass * 8 + rsub, m = m0w + ml;
    if (m >= M) continue;
    const float sr = p.sa[m];
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = ws[ml * ES + cg * 8 + e] * sr;
    if (R) {
      const TO* rp = R + (int64_t)m * p.ldr + n0;
      if constexpr (sizeof(TO) == 2) {
        const u32x4_t rv = *(const u32x4_t*)rp;
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[2 * e] += __uint_as_float(rv[e] << 16); v[2 * e + 1] += __uint_as_float(rv[e] & 0xffff0000u); }
      } else {
        const f32x4_t r0 = *(const f32x4_t*)rp, r1 = *(const f32x4_t*)(rp + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] += r0[e]; v[4 + e] += r1[e]; }
      }
    }
    store8(C + (int64_t)m * p.ldc + n0, v);
  }
}

static int w4a8_spl_shift(int64_t K) { return (K == 3072 || K == 4096) ? 1 : K == 8192 ? 2 : K == 14336 ? 3 : -1; }

extern "C" int vg_gemm_w4a8_supported(int64_t N, int64_t K) { return w4a8_spl_shift(K) >= 0 && N > 0 && N % 8 == 0 && N <= (1 << 30); }

template <typename TO>
static int launch_w4a8(const W4A8Args& p, hipStream_t st) {
  const int lds = 4 * 64 * 68 * 4;      // the epilogue's staging (68 KB) covers the two 24 KB stages
  vg_raise_lds_cap<gemm_w4a8_kernel<TO>>(lds);
  W4A8Args q = p;
  const int nt = p.a_op == 1 ? (p.N + 63) / 64 : (p.N + 127) / 128, mt = (p.M + 127) / 128;
  q.gn = nt < 4 ? nt : 4;
  gemm_w4a8_kernel<TO><<<dim3(nt, mt, 1), 256, lds, st>>>(q);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_gemm_w4a8(const uint8_t* A8, int64_t lda, const float* a_scale, const uint8_t* W4, int64_t ldw_bytes, void* C, int64_t ldc,
                            const void* R, int64_t ldr, int64_t M, int64_t N, int64_t K, int out_dtype, int a_op, vg_stream_t stream) {
  VG_CHECK(A8 && W4 && C && a_scale && M > 0 && N > 0 && K > 0, VG_ERR_ARG, "vg_gemm_w4a8: bad args M=%lld N=%lld K=%lld", (long long)M, (long long)N,
           (long long)K);
  VG_CHECK(out_dtype == VG_BF16 || out_dtype == VG_F32, VG_ERR_ARG, "vg_gemm_w4a8: bad out_dtype %d", out_dtype);
  VG_CHECK(a_op == 0 || (a_op == 1 && !R), VG_ERR_ARG, "vg_gemm_w4a8: a_op %d (0, or 1 = SwiGLU without residual)", a_op);
  VG_CHECK(M > 16 && M <= (1 << 22) && vg_gemm_w4a8_supported(N, K), VG_ERR_UNSUPPORTED,
           "vg_gemm_w4a8: M=%lld N=%lld K=%lld (M > 16, N a multiple of 8, K one of 3072, 4096, 8192, 14336)", (long long)M, (long long)N, (long long)K);
  const int sh = w4a8_spl_shift(K);
  const int oes = out_dtype == VG_BF16 ? 2 : 4;
  VG_CHECK(lda % 16 == 0 && lda >= K && ldw_bytes % 16 == 0 && ldw_bytes >= (64 << sh) + K / 2 && (((uintptr_t)A8 | (uintptr_t)W4) & 15) == 0, VG_ERR_ARG,
           "vg_gemm_w4a8: lda / ldw_bytes must be multiples of 16 that cover a row, A8 and W4 16-byte aligned");
  VG_CHECK(ldc >= N && (ldc * oes) % 16 == 0 && ((uintptr_t)C & 15) == 0 && (!R || (ldr >= N && (ldr * oes) % 16 == 0 && ((uintptr_t)R & 15) == 0)), VG_ERR_ARG,
           "vg_gemm_w4a8: C / R rows must be 16-byte aligned");
  W4A8Args p{};
  p.A = A8; p.sa = a_scale; p.W = W4; p.C = C; p.R = R;
  p.lda = lda; p.ldw = ldw_bytes; p.ldc = ldc; p.ldr = ldr;
  p.M = (int)M; p.N = (int)N; p.K = (int)K; p.a_op = a_op; p.gn = 4; p.spl_sh = sh;
  if (out_dtype == VG_BF16) return launch_w4a8<bf16_t>(p, (hipStream_t)stream);
  return launch_w4a8<float>(p, (hipStream_t)stream);
}
