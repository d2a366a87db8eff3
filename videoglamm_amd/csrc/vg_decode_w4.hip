// Decode-step GEMV with MXFP4 weights (OCP Microscaling v1.0: e2m1 elements, one e8m0 scale per 32 consecutive K elements of a weight row):
// vg_decode_gemv_w4, the 4-bit sibling of vg_decode_gemv_w8 (vg_decode.hip).  The structure is decode_gemv_fast_kernel's — x staged once per workgroup
// in LDS (normalised on the way), row PAIRS per wave, every weight load of a pair issued before its first use and two pairs in flight (one at K = 14336), wave_sum on the
// VALU, results parked in LDS and written by a lane-per-pair epilogue — with the row walk cut to the format:
//   * a lane's 16-byte load is 32 codes = exactly one scale block, so a whole row is CPL = K / 2048 loads per lane (2, 2, 4, 7 at K = 3072 (the second
//     one on half the lanes), 4096, 8192, 14336) and ONE batch: a pair is 2 x CPL loads, reduced once;
//   * v_cvt_scalef32_pk_bf16_fp4 turns a byte (two codes) into two bf16 with the block scale applied (exact: two significant bits times a power of
//     two), v_dot2c_f32_bf16 multiplies them with the staged bf16 x pair and accumulates in fp32: one instruction per weight;
//   * x sits in LDS in four planes (x chunk 4 c + h of weight chunk c at plane h, index c): the four 16-byte reads a lane makes per weight chunk are
//     then 16 bytes apart from its neighbours' instead of 64 (no bank conflicts).
// vg_decode_gemv_w4_rows (below the single-row kernel) applies every weight byte to up to 16 rows of x, each row with the single-row kernel's bits.
// The scale bytes are 1/16 of the code bytes and come one of two ways (vg_kernels.h): a head of 64 x SPL bytes in front of every row's codes, ordered so
// that a lane's SPL scales are ONE 2 / 4 / 8-byte load (packed rows, scales == NULL), or a second array in the logical order read with one byte load per
// chunk (the 64 lanes of a wave cover one 64-byte line).
#include "vg_common.h"
#include "vg_decode_launch.h"
#include <type_traits>

struct DecW4Args {
  const void* x; const uint8_t* W; const uint8_t* sc; void* y; const float* nw; const void* R;
  int N, K; int64_t ldw; float eps; int ppw;
};

constexpr int DEC4_MAX_PPW = 64;

// the epilogue of dec_gemv_store (vg_decode.hip) for bf16 activations: gate / up materialise in bf16, silu rounded to bf16, residual in the output dtype
template <typename TO, bool GLU>
__device__ __forceinline__ void dec4_store(const DecW4Args& p, int pi, float a0, float a1) {
  const int n0 = GLU ? pi : 2 * pi, n1 = GLU ? p.N + pi : 2 * pi + 1;
  TO* y = (TO*)p.y;
  const TO* R = (const TO*)p.R;
  if constexpr (GLU) {
    const float g = bf2f(f2bf(vg_silu(bf2f(f2bf(a0))))), u = bf2f(f2bf(a1));
    float v = g * u;
    if (R) v += vg_elt<TO>::ld(R + n0);
    vg_elt<TO>::st(y + n0, v);
  } else {
    float v = a0;
    if (R) v += vg_elt<TO>::ld(R + n0);
    vg_elt<TO>::st(y + n0, v);
    if (n1 < p.N) {
      v = a1;
      if (R) v += vg_elt<TO>::ld(R + n1);
      vg_elt<TO>::st(y + n1, v);
    }
  }
}

// e8m0 scale byte -> the float 2^(b - 127) (b = 0 gives 0.0f, not 2^-127: a block that small contributes nothing)
__device__ __forceinline__ float dec4_scale(uint32_t b) { return __uint_as_float(b << 23); }

// a dword of two bf16 as the dot instruction's operand type (by value: a bit cast applied to a vector ELEMENT reads element 0 of the vector)
__device__ __forceinline__ vg_bf16x2_t dec4_bf2(uint32_t v) { return __builtin_bit_cast(vg_bf16x2_t, v); }

// 32 e2m1 codes of one chunk (element 2j in the low nibble of byte j) times the block scale against the 32 bf16 of four x chunks
__device__ __forceinline__ float dec4_dot(const u32x4_t& w, float sc, const u32x4_t (&x)[4], float s) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t we = w[e], x0 = x[e][0], x1 = x[e][1], x2 = x[e][2], x3 = x[e][3];
    s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(we, sc, 0), dec4_bf2(x0), s, false);
    s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(we, sc, 1), dec4_bf2(x1), s, false);
    s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(we, sc, 2), dec4_bf2(x2), s, false);
    s = __builtin_amdgcn_fdot2_f32_bf16(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(we, sc, 3), dec4_bf2(x3), s, false);
  }
  return s;
}

// NWC = K / 32 weight chunks per row (96, 128, 256, 448), CPL = ceil(NWC / 64) per lane, SPL = scale bytes per lane in a packed row's head (CPL rounded
// up to 2, 4 or 8).  SEP: the scales are a second array [rows, NWC] (p.sc) instead of the row heads.
template <int NWC> struct Dec4Shape {
  static constexpr int CPL = (NWC + 63) / 64;
  static constexpr int SPL = CPL <= 2 ? 2 : CPL <= 4 ? 4 : 8;
  typedef typename std::conditional<SPL == 2, uint16_t, typename std::conditional<SPL == 4, uint32_t, uint64_t>::type>::type sc_t;
};

template <typename TO, bool GLU, int NWC, bool SEP>
__global__ __launch_bounds__(256) void decode_gemv_w4_kernel(DecW4Args p) {
  typedef Dec4Shape<NWC> S;
  constexpr int CPL = S::CPL, SPL = S::SPL;
  constexpr bool PART = NWC % 64 != 0;            // the last chunk per lane exists on the low lanes only (K = 3072)
  constexpr int NCH = NWC * 4;                    // 16-byte chunks of x
  constexpr int XN = (NCH + 255) / 256;
  typedef typename S::sc_t sc_t;
  extern __shared__ __attribute__((aligned(16))) char dec4_smem[];
  __shared__ float red[4];
  __shared__ float res[4][DEC4_MAX_PPW][2];
  u32x4_t* xs = (u32x4_t*)dec4_smem;               // [4][NWC]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int npair = GLU ? p.N : (p.N + 1) / 2;
  const int p0 = (blockIdx.x * 4 + wave) * p.ppw;
  const int np = max(min(p0 + p.ppw, npair) - p0, 0);     // pairs of this wave

  // ---- 1. every load up front, oldest-needed first: x, the norm weights, two pairs of W
  u32x4_t xr[XN];
#pragma unroll
  for (int i = 0; i < XN; ++i) xr[i] = ((const u32x4_t*)p.x)[min(tid + 256 * i, NCH - 1)];
  f32x4_t nwr[XN][2];
  if (p.nw) {
#pragma unroll
    for (int i = 0; i < XN; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) nwr[i][j] = ((const f32x4_t*)p.nw)[min(tid + 256 * i, NCH - 1) * 2 + j];
  }
  struct Set { u32x4_t v0[CPL], v1[CPL]; sc_t s0, s1; uint8_t b0[SEP ? CPL : 1], b1[SEP ? CPL : 1]; };
  int ipi = p0;                    // issue cursor
  auto issue = [&](Set& t) {
    const int pc = min(ipi, npair - 1);                       // clamped: the two prologue issues are unconditional
    const int n0 = GLU ? pc : 2 * pc, n1 = GLU ? p.N + pc : min(2 * pc + 1, p.N - 1);
    const uint8_t* r0 = p.W + (int64_t)n0 * p.ldw;
    const uint8_t* r1 = p.W + (int64_t)n1 * p.ldw;
    if constexpr (SEP) {
#pragma unroll
      for (int u = 0; u < CPL; ++u) {
        const int c = min(u * 64 + lane, NWC - 1);
        t.b0[u] = __builtin_nontemporal_load(p.sc + (int64_t)n0 * NWC + c);
        t.b1[u] = __builtin_nontemporal_load(p.sc + (int64_t)n1 * NWC + c);
      }
    } else {
      t.s0 = __builtin_nontemporal_load((const sc_t*)r0 + lane);
      t.s1 = __builtin_nontemporal_load((const sc_t*)r1 + lane);
      r0 += 64 * SPL;
      r1 += 64 * SPL;
    }
#pragma unroll
    for (int u = 0; u < CPL; ++u) {
      const int c = PART ? min(u * 64 + lane, NWC - 1) : u * 64 + lane;
      t.v0[u] = __builtin_nontemporal_load((const u32x4_t*)r0 + c);
      t.v1[u] = __builtin_nontemporal_load((const u32x4_t*)r1 + c);
    }
    ++ipi;
  };
  // two pairs in flight per wave; K = 14336 (14 loads = 56 registers per pair) keeps one and leaves the overlap to the other waves of the CU: a second
  // set would not fit 256 registers.  A wave's first pair is clamped, so a wave without pairs loads (and drops) the last one.
  constexpr bool TWO = CPL <= 4;
  Set sa, sb;
  issue(sa);
  if (TWO && np > 1) issue(sb);

  // ---- 2. stage x (normalised, the arithmetic of decode_gemv_fast_kernel) into the four LDS planes
  {
    float rstd = 1.f;
    if (p.nw) {
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < XN; ++i) {
        if (tid + 256 * i < NCH) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = __uint_as_float(xr[i][e] << 16), hi = __uint_as_float(xr[i][e] & 0xffff0000u);
            ss += lo * lo;
            ss += hi * hi;
          }
        }
      }
      ss = wave_sum(ss);
      if (lane == 0) red[wave] = ss;
      __syncthreads();
      rstd = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)p.K + p.eps);
#pragma unroll
      for (int i = 0; i < XN; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = __uint_as_float(xr[i][e] << 16), hi = __uint_as_float(xr[i][e] & 0xffff0000u);
          xr[i][e] = f2bf2(bf2f(f2bf(lo * rstd)) * nwr[i][e / 2][2 * (e % 2)], bf2f(f2bf(hi * rstd)) * nwr[i][e / 2][2 * (e % 2) + 1]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < XN; ++i) {
      const int c = tid + 256 * i;
      if (c < NCH) xs[(c & 3) * NWC + (c >> 2)] = xr[i];
    }
    __syncthreads();
  }

  // ---- 3. the stream: no stores inside (a pending store makes every later vmcnt wait a full drain), results to LDS
  int cpl = 0;
  auto consume = [&](const Set& t) {
    float a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int u = 0; u < CPL; ++u) {
      const int c = u * 64 + lane;
      const int cx = PART ? min(c, NWC - 1) : c;
      const u32x4_t xv[4] = {xs[cx], xs[NWC + cx], xs[2 * NWC + cx], xs[3 * NWC + cx]};
      u32x4_t w0 = t.v0[u], w1 = t.v1[u];
      if (PART && u == CPL - 1 && c >= NWC) {      // no such chunk: +0 codes
        w0 = u32x4_t{0, 0, 0, 0};
        w1 = u32x4_t{0, 0, 0, 0};
      }
      const uint32_t e0 = SEP ? (uint32_t)t.b0[u] : (uint32_t)(t.s0 >> (8 * u)) & 0xffu;
      const uint32_t e1 = SEP ? (uint32_t)t.b1[u] : (uint32_t)(t.s1 >> (8 * u)) & 0xffu;
      a0 = dec4_dot(w0, dec4_scale(e0), xv, a0);
      a1 = dec4_dot(w1, dec4_scale(e1), xv, a1);
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    if (lane == 0) { res[wave][cpl][0] = a0; res[wave][cpl][1] = a1; }
    ++cpl;
  };
  if constexpr (TWO) {
    int b = 0;
    for (; b + 4 <= np; b += 2) {      // on entry: pair b in set a, pair b+1 in set b
      consume(sa);
      issue(sa);
      consume(sb);
      issue(sb);
    }
    const int rem = np - b;
    if (rem == 3) {
      consume(sa);
      issue(sa);
      consume(sb);
      consume(sa);
    } else if (rem == 2) {
      consume(sa);
      consume(sb);
    } else if (rem == 1) {
      consume(sa);
    }
  } else {
    for (int b = 0; b < np; ++b) {
      consume(sa);
      if (b + 1 < np) issue(sa);
    }
  }
  // ---- 4. epilogue: one lane per pair
  for (int i = lane; i < np; i += 64) dec4_store<TO, GLU>(p, p0 + i, res[wave][i][0], res[wave][i][1]);
}

static int dec4_spl(int K) { return K == 3072 || K == 4096 ? 2 : K == 8192 ? 4 : K == 14336 ? 8 : 0; }

static int64_t dec4_row_bytes(int K) { return 64 * dec4_spl(K) + K / 2; }     // a packed row: the scale head, then the codes

template <typename TO, bool GLU, bool SEP>
static int launch_decode_gemv_w4(DecW4Args p, hipStream_t st) {
  const auto [ppw, blocks] = dec_pair_split(GLU ? p.N : (p.N + 1) / 2, 4, DEC4_MAX_PPW);      // four workgroups per CU, as vg_decode_gemv_w8
  p.ppw = ppw;
  const size_t lds = (size_t)p.K * 2;
  switch (p.K) {
    case 3072: decode_gemv_w4_kernel<TO, GLU, 96, SEP><<<blocks, 256, lds, st>>>(p); break;
    case 4096: decode_gemv_w4_kernel<TO, GLU, 128, SEP><<<blocks, 256, lds, st>>>(p); break;
    case 8192: decode_gemv_w4_kernel<TO, GLU, 256, SEP><<<blocks, 256, lds, st>>>(p); break;
    default: decode_gemv_w4_kernel<TO, GLU, 448, SEP><<<blocks, 256, lds, st>>>(p); break;
  }
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_decode_gemv_w4(const void* x, const uint8_t* W4, int64_t ldw_bytes, const uint8_t* scales, void* y, const float* norm_w, float eps,
                                 const void* R, int N, int K, int glu, int out_dtype, vg_stream_t stream) {
  VG_CHECK(x && W4 && y && N > 0 && K > 0, VG_ERR_ARG, "vg_decode_gemv_w4: bad args N=%d K=%d", N, K);
  VG_CHECK(dec4_spl(K), VG_ERR_UNSUPPORTED, "vg_decode_gemv_w4: K=%d is not one of the supported row lengths (3072, 4096, 8192, 14336)", K);
  const int64_t need = scales ? K / 2 : dec4_row_bytes(K);
  VG_CHECK(ldw_bytes % 16 == 0 && ldw_bytes >= need, VG_ERR_ARG, "vg_decode_gemv_w4: ldw_bytes=%lld must be a multiple of 16 and at least %lld (K=%d, %s)",
           (long long)ldw_bytes, (long long)need, K, scales ? "separate scales" : "packed rows");
  VG_CHECK(((uintptr_t)x & 15) == 0 && ((uintptr_t)W4 & 15) == 0 && ((uintptr_t)norm_w & 15) == 0, VG_ERR_ARG,
           "vg_decode_gemv_w4: x/W4/norm_w must be 16-byte aligned");
  VG_CHECK(out_dtype == VG_BF16 || out_dtype == VG_F32, VG_ERR_ARG, "vg_decode_gemv_w4: bad out_dtype %d", out_dtype);
  DecW4Args p{x, W4, scales, y, norm_w, R, N, K, ldw_bytes, eps, 1};
  hipStream_t st = (hipStream_t)stream;
#define VG_DEC_W4(TOO, G) return scales ? launch_decode_gemv_w4<TOO, G, true>(p, st) : launch_decode_gemv_w4<TOO, G, false>(p, st)
  if (out_dtype == VG_BF16) {
    if (glu) VG_DEC_W4(bf16_t, true);
    VG_DEC_W4(bf16_t, false);
  }
  if (glu) VG_DEC_W4(float, true);
  VG_DEC_W4(float, false);
#undef VG_DEC_W4
}

// ---------------------------------------------------------------------------------------------------------------
// B-row form of vg_decode_gemv_w4 (packed rows only; the MLP of the batched multi-prompt step with MXFP4 decode weights): every weight
// byte is loaded once and applied to the BR rows of x, and row r of the result is bit-identical to vg_decode_gemv_w4 on row r alone.  In the single-row
// kernel only the ORDER of operations enters a sum, and it is kept per (weight row, x row): one fp32 accumulator, the lane's chunks u = 0 .. CPL-1
// ascending (chunk 64 u + lane), dec4_dot's 16 dot instructions per chunk in its order, then wave_sum; the K = 3072 last chunk with the x index
// clamped and zero codes on the lanes without one; decode_gemv_w4_kernel's norm prologue and dec4_store per row.  v_cvt_scalef32_pk_bf16_fp4
// depends on the weight byte and its scale only, so a chunk of the pair is converted ONCE (2 x 16 registers) and fed to the BR rows' dots.
// x is staged in the single-row kernel's four planes per row ([BR][4][chunks]).  UPP chunks per lane (a range of u) are staged and streamed per
// phase: UPP = CPL is the whole row (always with a norm; ppw pairs per wave, two in flight where CPL <= 4), UPP < CPL the phased form for rows that
// exceed the staging budget: one pair per wave, its accumulators (and its scale head) carried across the phases, a phase's loads that phase's
// chunks only and issued before the phase's x is staged.
struct DecW4RowsArgs {
  const void* x; int64_t ldx; const uint8_t* W; int64_t ldw; void* y; int64_t ldy; const float* nw; float eps; const void* R; int64_t ldr;
  int N, K, B, ppw, f32out;
};

constexpr int DEC4_ROWS_PPW = 8, DEC4_ROWS_LDS = 64 * 1024;      // as DEC_ROWS_PPW / DEC_ROWS_LDS of the bf16 and fp8 B-row kernels (vg_decode.hip)

// the output dtype is a run-time flag (it enters dec4_store alone, one lane per result): half the instantiations
template <bool GLU, int NWC, int BR, int UPP>
__global__ __launch_bounds__(256) void decode_gemv_w4_rows_kernel(DecW4RowsArgs p) {
  typedef Dec4Shape<NWC> S;
  constexpr int CPL = S::CPL, SPL = S::SPL;
  constexpr bool PART = NWC % 64 != 0;
  constexpr bool WHOLE = UPP == CPL;
  constexpr bool TWO = WHOLE && CPL <= 4;          // two pairs in flight, as the single-row kernel
  constexpr int NCH = NWC * 4, XN = (NCH + 255) / 256;
  constexpr int PCH = WHOLE ? NWC : UPP * 64;      // weight chunks per row per phase
  static_assert(UPP >= 1 && UPP <= CPL, "a phase is a range of u");
  typedef typename S::sc_t sc_t;
  extern __shared__ __attribute__((aligned(16))) char dec4_smem[];
  __shared__ float red[BR][4];
  __shared__ float res[4][DEC4_ROWS_PPW][BR][2];
  u32x4_t* xs = (u32x4_t*)dec4_smem;               // [BR][4][PCH]: x chunk 4 c + h of the phase's weight chunk c at plane h
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int npair = GLU ? p.N : (p.N + 1) / 2;
  const int p0 = (blockIdx.x * 4 + wave) * p.ppw;
  const int np = max(min(p0 + p.ppw, npair) - p0, 0);     // pairs of this wave (at most one in the phased form)

  struct Set { u32x4_t v0[UPP], v1[UPP]; sc_t s0, s1; };
  auto issue = [&](Set& t, int li, int u0) {
    const int pc = p0 + li;
    const int n0 = GLU ? pc : 2 * pc, n1 = GLU ? p.N + pc : min(2 * pc + 1, p.N - 1);
    const uint8_t* r0 = p.W + (int64_t)n0 * p.ldw;
    const uint8_t* r1 = p.W + (int64_t)n1 * p.ldw;
    if (WHOLE || u0 == 0) {                        // the scale head once per pair
      t.s0 = __builtin_nontemporal_load((const sc_t*)r0 + lane);
      t.s1 = __builtin_nontemporal_load((const sc_t*)r1 + lane);
    }
    r0 += 64 * SPL;
    r1 += 64 * SPL;
#pragma unroll
    for (int j = 0; j < UPP; ++j) {
      if (CPL % UPP == 0 || u0 + j < CPL) {
        const int c = PART ? min((u0 + j) * 64 + lane, NWC - 1) : (u0 + j) * 64 + lane;
        t.v0[j] = __builtin_nontemporal_load((const u32x4_t*)r0 + c);
        t.v1[j] = __builtin_nontemporal_load((const u32x4_t*)r1 + c);
      }
    }
  };

  float a0[BR], a1[BR];
#pragma unroll
  for (int r = 0; r < BR; ++r) { a0[r] = 0.f; a1[r] = 0.f; }
  auto consume = [&](const Set& t, int li, int u0) {
#pragma unroll
    for (int j = 0; j < UPP; ++j) {
      if (CPL % UPP == 0 || u0 + j < CPL) {
        const int u = u0 + j, c = u * 64 + lane;
        const int cl = (PART ? min(c, NWC - 1) : c) - (WHOLE ? 0 : u0 * 64);
        u32x4_t w0 = t.v0[j], w1 = t.v1[j];
        if (PART && c >= NWC) {                    // no such chunk: +0 codes
          w0 = u32x4_t{0, 0, 0, 0};
          w1 = u32x4_t{0, 0, 0, 0};
        }
        const float sc0 = dec4_scale((uint32_t)(t.s0 >> (8 * u)) & 0xffu), sc1 = dec4_scale((uint32_t)(t.s1 >> (8 * u)) & 0xffu);
        vg_bf16x2_t c0[16], c1[16];                // the chunk converted once for the BR rows
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          c0[4 * e + 0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w0[e], sc0, 0);
          c0[4 * e + 1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w0[e], sc0, 1);
          c0[4 * e + 2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w0[e], sc0, 2);
          c0[4 * e + 3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w0[e], sc0, 3);
          c1[4 * e + 0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w1[e], sc1, 0);
          c1[4 * e + 1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w1[e], sc1, 1);
          c1[4 * e + 2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w1[e], sc1, 2);
          c1[4 * e + 3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w1[e], sc1, 3);
        }
        // per row dec4_dot's order: planes e ascending, dwords ascending.  Row r + 1's x is read while row r's dots run.  The compiler is held to that
        // order by the empty asm statements, which make the reads of row r + 1 wait for the sums of row r - 1: left alone it gathers every row's LDS
        // reads at the top of the block (16 registers a row), defers the dots, and the 16-row bucket spills
        u32x4_t xc[4], xn[4];
        {
          int c0l = cl;
          asm volatile("" : "+v"(c0l), "+v"(a0[BR - 1]), "+v"(a1[BR - 1]));     // (after the previous chunk's last row)
#pragma unroll
          for (int e = 0; e < 4; ++e) xc[e] = xs[e * PCH + c0l];
        }
#pragma unroll
        for (int r = 0; r < BR; ++r) {
          if (r + 1 < BR) {
            int cn = cl;
            if (r > 0) asm volatile("" : "+v"(cn), "+v"(a0[r - 1]), "+v"(a1[r - 1]));
#pragma unroll
            for (int e = 0; e < 4; ++e) xn[e] = xs[(4 * (r + 1) + e) * PCH + cn];
          }
          float s0 = a0[r], s1 = a1[r];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s0 = __builtin_amdgcn_fdot2_f32_bf16(c0[4 * e + k], dec4_bf2(xc[e][k]), s0, false);
#pragma unroll
            for (int k = 0; k < 4; ++k) s1 = __builtin_amdgcn_fdot2_f32_bf16(c1[4 * e + k], dec4_bf2(xc[e][k]), s1, false);
          }
          a0[r] = s0;
          a1[r] = s1;
          if (r + 1 < BR) {
#pragma unroll
            for (int e = 0; e < 4; ++e) xc[e] = xn[e];
          }
        }
      }
    }
    if (u0 + UPP >= CPL) {                         // the pair's last chunks
#pragma unroll
      for (int r = 0; r < BR; ++r) {
        const float s0 = wave_sum(a0[r]), s1 = wave_sum(a1[r]);
        if (lane == 0) { res[wave][li][r][0] = s0; res[wave][li][r][1] = s1; }
        a0[r] = 0.f;
        a1[r] = 0.f;
      }
    }
  };

  Set sa, sb;
  for (int u0 = 0; u0 < CPL; u0 += UPP) {
    // ---- 1. the phase's first weight loads, ahead of the staging
    if (np > 0) issue(sa, 0, u0);
    if (TWO && np > 1) issue(sb, 1, u0);
    if (u0 > 0) __syncthreads();                   // every wave is done with the previous phase's x
    // ---- 2. stage the rows' x chunks under the phase's weight chunks [cs, ce) (with a norm: the whole row, the single-row kernel's arithmetic)
    float rstd[BR];
#pragma unroll
    for (int r = 0; r < BR; ++r) rstd[r] = 1.f;
    if (WHOLE && p.nw) {
#pragma unroll
      for (int r = 0; r < BR; ++r) {
        const u32x4_t* xg = (const u32x4_t*)((const bf16_t*)p.x + (int64_t)min(r, p.B - 1) * p.ldx);
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < XN; ++i) {
          if (tid + 256 * i < NCH) {
            const u32x4_t v = xg[tid + 256 * i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float lo = __uint_as_float(v[e] << 16), hi = __uint_as_float(v[e] & 0xffff0000u);
              ss += lo * lo;
              ss += hi * hi;
            }
          }
        }
        ss = wave_sum(ss);
        if (lane == 0) red[r][wave] = ss;
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < BR; ++r) rstd[r] = rsqrtf((red[r][0] + red[r][1] + red[r][2] + red[r][3]) / (float)p.K + p.eps);
    }
    const int cs = WHOLE ? 0 : u0 * 64, ce = WHOLE ? NWC : min((u0 + UPP) * 64, NWC);
#pragma unroll 1
    for (int i = tid; i < (ce - cs) * 4; i += 256) {     // (not unrolled: the rows' loads of one x chunk at a time)
      const int gx = cs * 4 + i;                   // x chunk of the row
      f32x4_t n0 = {1.f, 1.f, 1.f, 1.f}, n1 = n0;
      if (WHOLE && p.nw) {
        n0 = ((const f32x4_t*)p.nw)[gx * 2];
        n1 = ((const f32x4_t*)p.nw)[gx * 2 + 1];
      }
      const float nwf[8] = {n0[0], n0[1], n0[2], n0[3], n1[0], n1[1], n1[2], n1[3]};
#pragma unroll
      for (int r = 0; r < BR; ++r) {
        u32x4_t v = ((const u32x4_t*)((const bf16_t*)p.x + (int64_t)min(r, p.B - 1) * p.ldx))[gx];
        if (WHOLE && p.nw) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float lo = __uint_as_float(v[e] << 16), hi = __uint_as_float(v[e] & 0xffff0000u);
            v[e] = f2bf2(bf2f(f2bf(lo * rstd[r])) * nwf[2 * e], bf2f(f2bf(hi * rstd[r])) * nwf[2 * e + 1]);
          }
        }
        xs[(4 * r + (i & 3)) * PCH + (i >> 2)] = v;
      }
    }
    __syncthreads();
    // ---- 3. the stream: no stores inside, results to LDS
    if constexpr (TWO) {
      int li = 0;
      for (; li + 1 < np; li += 2) {               // on entry: pair li in set a, pair li + 1 in set b
        consume(sa, li, u0);
        if (li + 2 < np) issue(sa, li + 2, u0);
        consume(sb, li + 1, u0);
        if (li + 3 < np) issue(sb, li + 3, u0);
      }
      if (li < np) consume(sa, li, u0);
    } else {
      for (int li = 0; li < np; ++li) {
        consume(sa, li, u0);
        if (li + 1 < np) issue(sa, li + 1, u0);
      }
    }
  }
  // ---- 4. epilogue: one lane per (pair, row); the single-row kernel's stores
  for (int i = lane; i < np * BR; i += 64) {
    const int li = i / BR, r = i % BR;
    if (r >= p.B) continue;
    DecW4Args q{};
    q.N = p.N;
    if (p.f32out) {
      q.y = (float*)p.y + r * p.ldy;
      q.R = p.R ? (const void*)((const float*)p.R + r * p.ldr) : nullptr;
      dec4_store<float, GLU>(q, p0 + li, res[wave][li][r][0], res[wave][li][r][1]);
    } else {
      q.y = (bf16_t*)p.y + r * p.ldy;
      q.R = p.R ? (const void*)((const bf16_t*)p.R + r * p.ldr) : nullptr;
      dec4_store<bf16_t, GLU>(q, p0 + li, res[wave][li][r][0], res[wave][li][r][1]);
    }
  }
}

extern "C" int vg_decode_gemv_w4_rows_supported(int K) { return dec4_spl(K) != 0; }

template <bool GLU, int NWC, int BR, int UPP>
static int launch_w4_rows_u(DecW4RowsArgs p, hipStream_t st) {
  constexpr int CPL = Dec4Shape<NWC>::CPL;
  const auto [ppw, blocks] = dec_rows_split(GLU ? p.N : (p.N + 1) / 2, UPP < CPL, DEC4_ROWS_PPW);
  p.ppw = ppw;
  const size_t lds = (size_t)BR * 4 * (UPP == CPL ? NWC : UPP * 64) * 16;
  vg_raise_lds_cap<decode_gemv_w4_rows_kernel<GLU, NWC, BR, UPP>>(lds);
  decode_gemv_w4_rows_kernel<GLU, NWC, BR, UPP><<<blocks, 256, lds, st>>>(p);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

// x staging: the whole rows when they fit the budget (always with the norm: the entry point has refused what does not fit 152 KiB), else phases of
// UPP = budget / (BR x 4 KiB) chunks per lane with one pair per wave (16 rows at K = 14336, the decoder's `down`: 7 phases)
template <bool GLU, int NWC, int BR>
static int launch_w4_rows_b(DecW4RowsArgs p, hipStream_t st) {
  constexpr int CPL = Dec4Shape<NWC>::CPL;
  constexpr int64_t ROWS = (int64_t)BR * NWC * 64;                // bytes of the bucket's rows
  constexpr int UPP = DEC4_ROWS_LDS / (BR * 4096) < 1 ? 1 : DEC4_ROWS_LDS / (BR * 4096);
  if constexpr (ROWS <= DEC4_ROWS_LDS) {
    return launch_w4_rows_u<GLU, NWC, BR, CPL>(p, st);
  } else {
    static_assert(UPP < CPL, "rows past the budget take more than one phase");
    if constexpr (ROWS <= 152 * 1024) {
      if (p.nw) return launch_w4_rows_u<GLU, NWC, BR, CPL>(p, st);
    }
    return launch_w4_rows_u<GLU, NWC, BR, UPP>(p, st);
  }
}

template <bool GLU, int BR>
static int launch_w4_rows_k(DecW4RowsArgs p, hipStream_t st) {
  switch (p.K) {
    case 3072: return launch_w4_rows_b<GLU, 96, BR>(p, st);
    case 4096: return launch_w4_rows_b<GLU, 128, BR>(p, st);
    case 8192: return launch_w4_rows_b<GLU, 256, BR>(p, st);
    default: return launch_w4_rows_b<GLU, 448, BR>(p, st);
  }
}

template <bool GLU>
static int launch_w4_rows(DecW4RowsArgs p, hipStream_t st) {
  return dec_with_bucket(p.B, [&](auto br) { return launch_w4_rows_k<GLU, decltype(br)::value>(p, st); });
}

extern "C" int vg_decode_gemv_w4_rows(const void* x, int64_t ldx, const uint8_t* W4, int64_t ldw_bytes, void* y, int64_t ldy, const float* norm_w,
                                      float eps, const void* R, int64_t ldr, int N, int K, int B, int glu, int out_dtype, vg_stream_t stream) {
  VG_CHECK(x && W4 && y && N > 0 && dec_rows_b_ok(B), VG_ERR_ARG, "vg_decode_gemv_w4_rows: bad args N=%d B=%d", N, B);
  VG_CHECK(vg_decode_gemv_w4_rows_supported(K), VG_ERR_UNSUPPORTED,
           "vg_decode_gemv_w4_rows: K=%d is not one of the supported row lengths (3072, 4096, 8192, 14336)", K);
  VG_CHECK(out_dtype == VG_BF16 || out_dtype == VG_F32, VG_ERR_ARG, "vg_decode_gemv_w4_rows: bad out_dtype %d", out_dtype);
  VG_CHECK(ldw_bytes % 16 == 0 && ldw_bytes >= dec4_row_bytes(K), VG_ERR_ARG,
           "vg_decode_gemv_w4_rows: ldw_bytes=%lld must be a multiple of 16 and at least %lld (K=%d, packed rows)", (long long)ldw_bytes,
           (long long)dec4_row_bytes(K), K);
  VG_CHECK(ldx % 8 == 0 && ((((uintptr_t)x) | ((uintptr_t)W4) | ((uintptr_t)norm_w)) & 15) == 0, VG_ERR_ARG,
           "vg_decode_gemv_w4_rows: alignment (16 bytes; ldx a multiple of 8)");
  const int br = dec_bucket(B);      // the bucket the kernel stages
  VG_CHECK(!norm_w || (int64_t)br * K * 2 <= 160 * 1024 - 8 * 1024, VG_ERR_UNSUPPORTED,
           "vg_decode_gemv_w4_rows: the norm stages the whole rows of the %d-row bucket: B=%d K=%d do not fit", br, B, K);
  DecW4RowsArgs p{x, ldx, W4, ldw_bytes, y, ldy, norm_w, eps, R, ldr, N, K, B, 1, out_dtype == VG_F32};
  hipStream_t st = (hipStream_t)stream;
  return glu ? launch_w4_rows<true>(p, st) : launch_w4_rows<false>(p, st);
}
