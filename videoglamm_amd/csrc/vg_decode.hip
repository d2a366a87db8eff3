// Single-token decode step of the LLM: one new row against the KV cache and against every
// weight matrix.  The step is HBM-bound (all weights stream once per token) and latency-bound (a chain of ~9 dependent
// launches per layer, each paying ~4-5 us of ramp on top of its bytes), so the kernels here exist to cut launches:
//   decode_gemv_kernel  : [RMSNorm ->] x.W^T [-> SwiGLU] [+ residual]   (norm and GLU fused into the GEMV)
//   decode_attn_kernel  : RoPE(q,k) + KV-cache append + split-KV attention + merge of the splits by the last
//                         workgroup to finish (no separate rope / combine launches)
// Arithmetic mirrors the stand-alone kernels (vg_rmsnorm, vg_gemm skinny path, vg_rope_kv_append) step for step.
#include "vg_common.h"
#include "vg_decode_launch.h"
#include <type_traits>

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

template <typename T> __device__ __forceinline__ void dec_unpack(const u32x4_t& v, float* f);
template <> __device__ __forceinline__ void dec_unpack<float>(const u32x4_t& v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) f[e] = __uint_as_float(v[e]);
}
template <> __device__ __forceinline__ void dec_unpack<bf16_t>(const u32x4_t& v, float* f) {
#pragma unroll
  for (int e = 0; e < 4; ++e) { f[2 * e] = __uint_as_float(v[e] << 16); f[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u); }
}
template <typename T> __device__ __forceinline__ u32x4_t dec_pack(const float* f);
template <> __device__ __forceinline__ u32x4_t dec_pack<float>(const float* f) {
  u32x4_t v = {__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3])};
  return v;
}
template <> __device__ __forceinline__ u32x4_t dec_pack<bf16_t>(const float* f) {
  u32x4_t v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = f2bf2(f[2 * e], f[2 * e + 1]);
  return v;
}
template <typename T> __device__ __forceinline__ float dec_dot(const u32x4_t& a, const u32x4_t& b);
template <> __device__ __forceinline__ float dec_dot<float>(const u32x4_t& a, const u32x4_t& b) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) s = fmaf(__uint_as_float(a[e]), __uint_as_float(b[e]), s);
  return s;
}
template <> __device__ __forceinline__ float dec_dot<bf16_t>(const u32x4_t& a, const u32x4_t& b) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    s = fmaf(__uint_as_float(a[e] << 16), __uint_as_float(b[e] << 16), s);
    s = fmaf(__uint_as_float(a[e] & 0xffff0000u), __uint_as_float(b[e] & 0xffff0000u), s);
  }
  return s;
}
// 16 fp8 (OCP e4m3) weights of one 16-byte chunk against the 16 bf16 activations of two x chunks
__device__ __forceinline__ float dec_dot_w8(const u32x4_t& w, const u32x4_t& x0, const u32x4_t& x1) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[e], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[e], true);
    const uint32_t xa = e < 2 ? x0[2 * e] : x1[2 * e - 4], xb = e < 2 ? x0[2 * e + 1] : x1[2 * e - 3];
    s = fmaf(lo[0], __uint_as_float(xa << 16), s);
    s = fmaf(lo[1], __uint_as_float(xa & 0xffff0000u), s);
    s = fmaf(hi[0], __uint_as_float(xb << 16), s);
    s = fmaf(hi[1], __uint_as_float(xb & 0xffff0000u), s);
  }
  return s;
}
// 13-bit bf16 (vg_decode_pack13): one 16-byte x chunk against the lane's weights 8 U .. 8 U + 7 of a (row, batch) block.  H = the 8 dwords of
// high bytes [sign | e5 | m2] (weight i in byte i % 4 of H[i / 4]), L = the 160-bit string of low mantissa bits (weight i at bits 5 i .. 5 i + 4).
// v_cvt_pk_f32_bf8 makes the fp32 sign | code + 112 | m2 << 21 of two weights; the five low bits go under it at fp32 bits 20..16 with one
// (funnel) shift and one v_and_or.  The operand is the true weight times 2^(112 - base_row), and the fmaf chain is dec_dot<bf16_t>'s.
template <int U> __device__ __forceinline__ float dec_dot_p13(const uint32_t (&H)[8], const uint32_t (&L)[5], const u32x4_t& x) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  float s = 0.f;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)H[2 * U + h], false), hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)H[2 * U + h], true);
    const float f[4] = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = 4 * h + t, bit = 5 * (8 * U + j), d = bit >> 5, o = bit & 31;
      uint32_t m;          // the weight's five bits at 20..16 (other bits: neighbours, masked below)
      if (o <= 16) m = L[d] << (16 - o);
      else if (o <= 27) m = L[d] >> (o - 16);
      else m = __builtin_amdgcn_alignbit(L[d < 4 ? d + 1 : d], L[d], o - 16);
      const float w = __uint_as_float((m & 0x001f0000u) | __float_as_uint(f[t]));
      const uint32_t xe = x[j >> 1];
      s = fmaf(w, __uint_as_float((j & 1) ? (xe & 0xffff0000u) : (xe << 16)), s);
    }
  }
  return s;
}
template <typename T> __device__ __forceinline__ float dec_round(float v) { return v; }
template <> __device__ __forceinline__ float dec_round<bf16_t>(float v) { return bf2f(f2bf(v)); }

// ---------------------------------------------------------------------------------------------------------------
// GEMV.  x (one row, K elements) is staged once per workgroup into LDS — normalised on the way when norm_w is given
// (HF LlamaRMSNorm: fp32 mean of squares, x*rstd cast to the activation dtype, then * weight) — and every wave streams
// PAIRS of weight rows against it: rows (2i, 2i+1), or (i, N+i) = gate|up of output i when GLU.
struct DecGemvArgs {
  const void* x; const void* W; void* y; const float* nw; const void* R;
  int N, K; int64_t ldw; float eps; int ppw;
  const float* wscale;   // fp8 weights only: one fp32 scale per weight row
  // RoPE epilogue (vg_decode_qkv_rope): the rows are the fused q|k|v projection of the new token; pairs are (d, d + D/2) of one head, rotated in
  // registers with the CURRENT position's cos / sin row (rope_cs: [2][D/2] fp32 at a fixed address, refreshed by vg_decode_advance), q heads go to
  // y, the new key / value rows straight into the caches at *pos_dev
  const float* rope_cs; const int* pos_dev; void* kc; void* vc; int H, Hkv;
  // 13-bit bf16 weights (vg_decode_gemv_p13): Wp = the packed (row, batch) blocks that are streamed in place of W, wscale = 2^(base_row - 112)
  // per row (1 for a raw row), raw[nraw] = the rows that are recomputed from W itself
  const uint8_t* Wp; const int* raw; int nraw;
};

// Lossless 13-bit bf16 rows.  A weight keeps its sign, its 7 mantissa bits and a 5-bit exponent code c = E - base_row in 1..30 (E the
// biased bf16 exponent; c = 0 with a zero mantissa = +-0).  A row whose non-zero exponents span more than 30 binades, that holds a denormal, an
// inf or a NaN, or whose scale 2^(base_row - 112) is no normal fp32 is RAW: its block is not used and the GEMV recomputes it from the bf16 matrix.
// Layout: per (row, batch of 2048 K elements) one 3328-byte block of four lane-major planes, 64 x 16 B | 64 x 16 B | 64 x 16 B | 64 x 4 B = the
// dwords H[0..3] | H[4..7] | L[0..3] | L[4] of each lane (dec_dot_p13); the lane's 32 weights are those of its four 16-byte chunks of the bf16 walk,
// weight 8 u + j = element j of chunk (batch * 256 + u * 64 + lane).
constexpr int DEC_P13_BLOCK = 3328;

// The e4m3 code of a bf16 value held in fp32 (the fp8 K/V cache): clamp to +-448 in fp32, then round to nearest even — bit for bit
// x.float().clamp(-448, 448).to(torch.float8_e4m3fn).  A NaN keeps its sign and becomes the NaN code (0x7f / 0xff): the clamp must not eat it.
__device__ __forceinline__ float kv8_clamp(float v) { return v > 448.f ? 448.f : (v < -448.f ? -448.f : v); }
__device__ __forceinline__ uint32_t kv8_fix_nan(uint32_t w, float v, int byte) {
  if (v != v) w = (w & ~(0xffu << (8 * byte))) | ((0x7fu | ((__float_as_uint(v) >> 24) & 0x80u)) << (8 * byte));
  return w;
}
__device__ __forceinline__ uint32_t kv8_pack4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(a), kv8_clamp(b), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(kv8_clamp(c), kv8_clamp(d), w, true);
  uint32_t u = (uint32_t)w;
  u = kv8_fix_nan(u, a, 0); u = kv8_fix_nan(u, b, 1); u = kv8_fix_nan(u, c, 2); u = kv8_fix_nan(u, d, 3);
  return u;
}
// The rope epilogues' store of a rotate-half pair (d, d + RHD) of a key / value head into an e4m3 cache (KVO = kv8_t below; KVO = the activation
// type is the plain store): two byte stores of the codes of the bf16 values the bf16 cache would have held — the values are rounded to bf16
// first, as that cache's store rounds them — and no other byte of the row is read or written.
__device__ __forceinline__ void kv8_store_pair(kv8_t* dst, int hi, float o1, float o2) {
  const uint32_t w = kv8_pack4(bf2f(f2bf(o1)), bf2f(f2bf(o2)), 0.f, 0.f);
  dst[0].b = (uint8_t)(w & 0xffu);
  dst[hi].b = (uint8_t)((w >> 8) & 0xffu);
}

template <typename T, typename TO, bool GLU>
__device__ __forceinline__ void dec_gemv_store(const DecGemvArgs& p, int pi, float a0, float a1) {
  const int n0 = GLU ? pi : 2 * pi, n1 = GLU ? p.N + pi : 2 * pi + 1;
  if (p.wscale) {        // fp8 weights: the row scales leave the dot products
    a0 *= p.wscale[n0];
    a1 *= p.wscale[GLU ? n1 : min(n1, p.N - 1)];
  }
  TO* y = (TO*)p.y;
  const TO* R = (const TO*)p.R;
  if constexpr (GLU) {
    float g = a0, u = a1;
    if (sizeof(T) == 2) { g = bf2f(f2bf(g)); u = bf2f(f2bf(u)); }   // gate/up projections materialise in bf16 in HF
    g = vg_silu(g);
    if (sizeof(T) == 2) g = bf2f(f2bf(g));
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

// Fast path, K = a whole number of batches of chunks.  A wave owns `ppw` consecutive pairs and walks them as one flat sequence of
// batches (2 rows x 4 chunks per lane), software-pipelined two batches deep = 16 x 16-byte loads in flight per lane.
// Everything the kernel must wait for is requested up front, oldest-needed first (vmcnt retires in order): x, the norm
// weights, then both pipeline stages of W — the norm runs underneath the HBM round trip.  The loop body is branch-free
// and issues no stores: results go to LDS and are written out (with the residual / SwiGLU epilogue) once at the end,
// because on gfx9 a pending store makes every later vmcnt wait a full drain.
constexpr int DEC_MAX_PPW = 64;

// NB batches per row pair, CPB 16-byte chunks per lane per row per batch: K = NB * CPB * 64 chunks (CPB = 4 unless K only
// divides by 128 chunks, e.g. Phi-3's hidden 3072 = 3 x 2 x 64 x 8).
// W8: the weights are fp8 (OCP e4m3, one byte each) with a per-row scale; a weight chunk then covers 16 K elements = TWO
// x chunks, and NB x CPB x 64 counts weight chunks (K = 16 x that).
// RHD = D/2 > 0: the RoPE form above (pairs (d, d + RHD) of a head instead of adjacent rows)
// P13: the weights stream as 13-bit bf16 blocks (p.Wp, above): a batch of a row is 3 x 16 + 4 bytes per lane instead of 4 x 16, in the same four
// load instructions, and covers the same K elements in the same (chunk, element) order.  The result has the bits of the bf16 kernel's:
//   * the decoded operand is the true weight times 2^k, k = 112 - base_row fixed per row, and x is the same, so by induction every partial sum of
//     the fmaf chain, of the per-chunk adds and of wave_sum is the bf16 kernel's times 2^k: each operation rounds the same significand, as long
//     as no partial sum, with or without the factor 2^k, is a denormal or overflows;
//   * the order of operations is the bf16 kernel's: lane, batch, chunk and element walk, one fmaf per weight, one add per chunk, wave_sum;
//   * the multiplication by 2^-k (p.wscale, a normal fp32 power of two) after wave_sum is exact under the same condition.
// The condition is a premise on the data (|x| within 2^+-60 is ample); a raw row does not lean on it: it is recomputed (3b below)
// from the bf16 matrix with the bf16 kernel's own code, and its wscale is 1.
template <typename T, typename TO, bool GLU, int NB, int CPB = 4, bool W8 = false, int RHD = 0, bool P13 = false, typename KVO = TO>
__global__ __launch_bounds__(256) void decode_gemv_fast_kernel(DecGemvArgs p) {
  extern __shared__ __attribute__((aligned(16))) char dec_smem[];
  __shared__ float red[4];
  __shared__ float res[4][DEC_MAX_PPW][2];
  __shared__ float rope_lds[RHD > 0 ? 2 * RHD : 1];
  static_assert(RHD == 0 || (!GLU && !W8 && 2 * RHD <= 256), "RoPE form: plain bf16 / fp32 rows");
  constexpr int KPC = 16 / sizeof(T);
  constexpr int NWV = KPC / 4;     // float4 loads of norm weight per chunk
  static_assert(!W8 || sizeof(T) == 2, "fp8 weights pair with bf16 activations");
  static_assert(!P13 || (sizeof(T) == 2 && CPB == 4 && !W8 && RHD == 0), "13-bit weights: bf16 rows in batches of four chunks per lane");
  constexpr int NCH = NB * CPB * 64 * (W8 ? 2 : 1);  // 16-byte chunks of x (with W8 a weight row has half as many)
  constexpr int XN = (NCH + 255) / 256;          // chunks of x per thread (the last one may be partial: NCH % 256 == 128)
  typedef float f32x4_t __attribute__((ext_vector_type(4)));
  u32x4_t* xs = (u32x4_t*)dec_smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int npair = GLU ? p.N : (p.N + 1) / 2;
  const int gw = blockIdx.x * 4 + wave;
  typedef typename std::conditional<W8, uint8_t, T>::type WT;
  const WT* W = (const WT*)p.W;
  const int p0 = gw * p.ppw;
  const int np = max(min(p0 + p.ppw, npair) - p0, 0);     // pairs of this wave
  const int total = np * NB;

  // ---- 1. every load up front
  u32x4_t xr[XN];
#pragma unroll
  for (int i = 0; i < XN; ++i) xr[i] = ((const u32x4_t*)p.x)[min(tid + 256 * i, NCH - 1)];
  f32x4_t nwr[XN][NWV];
  if (p.nw) {
#pragma unroll
    for (int i = 0; i < XN; ++i)
#pragma unroll
      for (int j = 0; j < NWV; ++j) nwr[i][j] = ((const f32x4_t*)p.nw)[min(tid + 256 * i, NCH - 1) * NWV + j];
  }
  float ropev = 0.f;               // cos (tid < RHD) / sin (RHD <= tid < 2 RHD) of the current position: requested BEFORE the weights, so the wait below costs the stream nothing
  if constexpr (RHD > 0) ropev = p.rope_cs[min(tid, 2 * RHD - 1)];
  int ipi = p0, icb = 0;           // issue cursor (pair, batch within the pair)
  u32x4_t va0[CPB], va1[CPB], vb0[CPB], vb1[CPB];
  auto issue = [&](u32x4_t (&v0)[CPB], u32x4_t (&v1)[CPB]) {
    const int pc = min(ipi, npair - 1);                      // clamped: the two prologue issues are unconditional
    const int n0 = RHD > 0 ? (pc / max(RHD, 1)) * (2 * RHD) + pc % max(RHD, 1) : GLU ? pc : 2 * pc;
    const int n1 = RHD > 0 ? n0 + RHD : GLU ? p.N + pc : min(2 * pc + 1, p.N - 1);
    if constexpr (P13) {                                     // three planes of 16 bytes per lane and one of 4: v[0..2] and v[3][0]
      const uint8_t* b0 = p.Wp + ((int64_t)n0 * NB + icb) * DEC_P13_BLOCK;
      const uint8_t* b1 = p.Wp + ((int64_t)n1 * NB + icb) * DEC_P13_BLOCK;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        v0[u] = __builtin_nontemporal_load((const u32x4_t*)(b0 + u * 1024) + lane);
        v1[u] = __builtin_nontemporal_load((const u32x4_t*)(b1 + u * 1024) + lane);
      }
      v0[3][0] = __builtin_nontemporal_load((const uint32_t*)(b0 + 3072) + lane);
      v1[3][0] = __builtin_nontemporal_load((const uint32_t*)(b1 + 3072) + lane);
    } else {
      const u32x4_t* w0 = (const u32x4_t*)(W + (int64_t)n0 * p.ldw) + icb * (64 * CPB) + lane;
      const u32x4_t* w1 = (const u32x4_t*)(W + (int64_t)n1 * p.ldw) + icb * (64 * CPB) + lane;
#pragma unroll
      for (int u = 0; u < CPB; ++u) {
        v0[u] = __builtin_nontemporal_load(w0 + u * 64);
        v1[u] = __builtin_nontemporal_load(w1 + u * 64);
      }
    }
    if (++icb == NB) { icb = 0; ++ipi; }
  };
  issue(va0, va1);
  issue(vb0, vb1);

  // ---- 2. stage x (normalised) into LDS
  {
    float rstd = 1.f;
    if (p.nw) {
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < XN; ++i) {
        float f[KPC];
        dec_unpack<T>(xr[i], f);
        if (tid + 256 * i < NCH) {
#pragma unroll
          for (int e = 0; e < KPC; ++e) ss += f[e] * f[e];
        }
      }
      ss = wave_sum(ss);
      if (lane == 0) red[wave] = ss;
      __syncthreads();
      rstd = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)p.K + p.eps);
#pragma unroll
      for (int i = 0; i < XN; ++i) {
        float f[KPC];
        dec_unpack<T>(xr[i], f);
#pragma unroll
        for (int e = 0; e < KPC; ++e) f[e] = dec_round<T>(f[e] * rstd) * nwr[i][e / 4][e % 4];
        xr[i] = dec_pack<T>(f);
      }
    }
#pragma unroll
    for (int i = 0; i < XN; ++i)
      if (tid + 256 * i < NCH) xs[tid + 256 * i] = xr[i];
    if constexpr (RHD > 0) {
      if (tid < 2 * RHD) rope_lds[tid] = ropev;
    }
    __syncthreads();
  }

  // ---- 3. the stream
  float a0 = 0.f, a1 = 0.f;
  int cpl = 0, ccb = 0;            // consume cursor (local pair, batch within the pair)
  auto consume = [&](const u32x4_t (&v0)[CPB], const u32x4_t (&v1)[CPB]) {
    if constexpr (P13) {
      const uint32_t H0[8] = {v0[0][0], v0[0][1], v0[0][2], v0[0][3], v0[1][0], v0[1][1], v0[1][2], v0[1][3]};
      const uint32_t H1[8] = {v1[0][0], v1[0][1], v1[0][2], v1[0][3], v1[1][0], v1[1][1], v1[1][2], v1[1][3]};
      const uint32_t L0[5] = {v0[2][0], v0[2][1], v0[2][2], v0[2][3], v0[3][0]}, L1[5] = {v1[2][0], v1[2][1], v1[2][2], v1[2][3], v1[3][0]};
      const int wc = ccb * (64 * CPB) + lane;
      const u32x4_t x0 = xs[wc], x1 = xs[wc + 64], x2 = xs[wc + 128], x3 = xs[wc + 192];
      a0 += dec_dot_p13<0>(H0, L0, x0);
      a1 += dec_dot_p13<0>(H1, L1, x0);
      a0 += dec_dot_p13<1>(H0, L0, x1);
      a1 += dec_dot_p13<1>(H1, L1, x1);
      a0 += dec_dot_p13<2>(H0, L0, x2);
      a1 += dec_dot_p13<2>(H1, L1, x2);
      a0 += dec_dot_p13<3>(H0, L0, x3);
      a1 += dec_dot_p13<3>(H1, L1, x3);
    }
#pragma unroll
    for (int u = 0; u < (P13 ? 0 : CPB); ++u) {
      const int wc = ccb * (64 * CPB) + u * 64 + lane;
      if constexpr (W8) {
        const u32x4_t xa = xs[2 * wc], xb = xs[2 * wc + 1];
        a0 += dec_dot_w8(v0[u], xa, xb);
        a1 += dec_dot_w8(v1[u], xa, xb);
      } else {
        const u32x4_t xv = xs[wc];
        a0 += dec_dot<T>(v0[u], xv);
        a1 += dec_dot<T>(v1[u], xv);
      }
    }
    if (++ccb == NB) {
      a0 = wave_sum(a0);
      a1 = wave_sum(a1);
      if (lane == 0) { res[wave][cpl][0] = a0; res[wave][cpl][1] = a1; }
      a0 = 0.f;
      a1 = 0.f;
      ccb = 0;
      ++cpl;
    }
  };
  int b = 0;
  for (; b + 4 <= total; b += 2) {      // on entry: batch b in set a, batch b+1 in set b
    consume(va0, va1);
    issue(va0, va1);
    consume(vb0, vb1);
    issue(vb0, vb1);
  }
  const int rem = total - b;
  if (rem == 3) {
    consume(va0, va1);
    issue(va0, va1);
    consume(vb0, vb1);
    consume(va0, va1);
  } else if (rem == 2) {
    consume(va0, va1);
    consume(vb0, vb1);
  } else if (rem == 1) {
    consume(va0, va1);
  }
  // ---- 3b. 13-bit weights: the raw rows among this wave's pairs, recomputed from the bf16 matrix in the bf16 kernel's order
  if constexpr (P13) {
    for (int r = 0; r < p.nraw; ++r) {
      const int n = p.raw[r];
      const int pi = GLU ? (n < p.N ? n : n - p.N) : n >> 1, half = GLU ? (n >= p.N) : (n & 1);
      if (n < 0 || n >= (GLU ? 2 * p.N : p.N) || pi < p0 || pi >= p0 + np) continue;
      const u32x4_t* w =(const u32x4_t*)(W + (int64_t)n * p.ldw);
      float a = 0.f;
      for (int cb = 0; cb < NB; ++cb) {
#pragma unroll
        for (int u = 0; u < CPB; ++u) {
          const int wc = cb * (64 * CPB) + u * 64 + lane;
          a += dec_dot<T>(w[wc], xs[wc]);
        }
      }
      a = wave_sum(a);
      if (lane == 0) res[wave][pi - p0][half] = a;
    }
  }
  // ---- 4. epilogue: one lane per pair
  if constexpr (RHD > 0) {
    constexpr bool KV8O = std::is_same<KVO, kv8_t>::value;      // byte K/V destinations (vg_decode_qkv_rope_kv8)
    const int pos = *p.pos_dev;
    for (int i = lane; i < np; i += 64) {
      const int pi = p0 + i, hh = pi / RHD, d = pi % RHD;
      const float x1 = dec_round<TO>(res[wave][i][0]), x2 = dec_round<TO>(res[wave][i][1]);      // the projection materialises in the activation dtype (HF)
      float o1 = x1, o2 = x2;
      TO* dst;
      if (hh < p.H + p.Hkv) {      // q and k heads: rotate-half RoPE, the arithmetic of vg_rope_kv_append / decode_attn_kernel
        const float c = rope_lds[d], sv = rope_lds[RHD + d];
        if (sizeof(TO) == 2) {
          const float cb = bf2f(f2bf(c)), sb = bf2f(f2bf(sv));
          o1 = bf2f(f2bf(x1 * cb)) + bf2f(f2bf(-x2 * sb));
          o2 = bf2f(f2bf(x2 * cb)) + bf2f(f2bf(x1 * sb));
        } else {
          o1 = x1 * c - x2 * sv;
          o2 = x2 * c + x1 * sv;
        }
        if constexpr (KV8O) {
          if (hh >= p.H) { kv8_store_pair((KVO*)p.kc + ((int64_t)pos * p.Hkv + (hh - p.H)) * (2 * RHD) + d, RHD, o1, o2); continue; }
        }
        dst = hh < p.H ? (TO*)p.y + (int64_t)hh * (2 * RHD) : (TO*)p.kc + ((int64_t)pos * p.Hkv + (hh - p.H)) * (2 * RHD);
      } else {
        if constexpr (KV8O) { kv8_store_pair((KVO*)p.vc + ((int64_t)pos * p.Hkv + (hh - p.H - p.Hkv)) * (2 * RHD) + d, RHD, o1, o2); continue; }
        dst = (TO*)p.vc + ((int64_t)pos * p.Hkv + (hh - p.H - p.Hkv)) * (2 * RHD);
      }
      vg_elt<TO>::st(dst + d, o1);
      vg_elt<TO>::st(dst + d + RHD, o2);
    }
  } else {
    for (int i = lane; i < np; i += 64) dec_gemv_store<T, TO, GLU>(p, p0 + i, res[wave][i][0], res[wave][i][1]);
  }
}

template <typename T, typename TO, bool GLU>
__global__ __launch_bounds__(256) void decode_gemv_kernel(DecGemvArgs p) {
  extern __shared__ __attribute__((aligned(16))) char dec_smem[];
  __shared__ float red[4];
  constexpr int KPC = 16 / sizeof(T);
  u32x4_t* xs = (u32x4_t*)dec_smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nch = p.K / KPC;
  const int npair = GLU ? p.N : (p.N + 1) / 2;
  const int gw = blockIdx.x * 4 + wave;
  const T* W = (const T*)p.W;
  {
    const u32x4_t* xg = (const u32x4_t*)p.x;
    float ss = 0.f;
    for (int c = tid; c < nch; c += 256) {
      const u32x4_t v = xg[c];
      xs[c] = v;
      if (p.nw) {
        float f[KPC];
        dec_unpack<T>(v, f);
#pragma unroll
        for (int e = 0; e < KPC; ++e) ss += f[e] * f[e];
      }
    }
    if (p.nw) {
      ss = wave_sum(ss);
      if (lane == 0) red[wave] = ss;
      __syncthreads();
      const float rstd = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)p.K + p.eps);
      for (int c = tid; c < nch; c += 256) {   // each thread re-reads only the chunks it wrote itself
        float f[KPC];
        dec_unpack<T>(xs[c], f);
#pragma unroll
        for (int e = 0; e < KPC; ++e) f[e] = dec_round<T>(f[e] * rstd) * p.nw[c * KPC + e];
        xs[c] = dec_pack<T>(f);
      }
    }
    __syncthreads();
  }
  const int TW = gridDim.x * 4;
  for (int i = gw; i < npair; i += TW) {
    const int n0 = GLU ? i : 2 * i;
    const int n1 = GLU ? p.N + i : min(2 * i + 1, p.N - 1);
    const u32x4_t* w0 = (const u32x4_t*)(W + (int64_t)n0 * p.ldw);
    const u32x4_t* w1 = (const u32x4_t*)(W + (int64_t)n1 * p.ldw);
    float a0 = 0.f, a1 = 0.f;
    int c = lane;
    for (; c + 3 * 64 < nch; c += 4 * 64) {
      u32x4_t v0[4], v1[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { v0[u] = w0[c + u * 64]; v1[u] = w1[c + u * 64]; }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const u32x4_t xv = xs[c + u * 64];
        a0 += dec_dot<T>(v0[u], xv);
        a1 += dec_dot<T>(v1[u], xv);
      }
    }
    for (; c < nch; c += 64) {
      const u32x4_t xv = xs[c];
      a0 += dec_dot<T>(w0[c], xv);
      a1 += dec_dot<T>(w1[c], xv);
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    if (lane == 0) dec_gemv_store<T, TO, GLU>(p, i, a0, a1);
  }
}

template <typename T, typename TO, bool GLU>
static int launch_decode_gemv(DecGemvArgs p, hipStream_t st) {
  constexpr int KPC = 16 / sizeof(T);
  const auto [ppw, blocks] = dec_pair_split(GLU ? p.N : (p.N + 1) / 2, 2, DEC_MAX_PPW);
  p.ppw = ppw;
  const size_t lds = (size_t)p.K * sizeof(T);
  const int nch = p.K / KPC;
  if (nch == 384) {        // Phi-3-mini hidden size: three batches of two chunks per lane
    decode_gemv_fast_kernel<T, TO, GLU, 3, 2><<<blocks, 256, lds, st>>>(p);
    VG_LAUNCH_CHECK();
    return VG_OK;
  }
  const int nb = nch % 256 == 0 ? nch / 256 : 0;
  switch (nb) {
    case 1: decode_gemv_fast_kernel<T, TO, GLU, 1><<<blocks, 256, lds, st>>>(p); break;
    case 2: decode_gemv_fast_kernel<T, TO, GLU, 2><<<blocks, 256, lds, st>>>(p); break;
    case 4: decode_gemv_fast_kernel<T, TO, GLU, 4><<<blocks, 256, lds, st>>>(p); break;
    case 7: decode_gemv_fast_kernel<T, TO, GLU, 7><<<blocks, 256, lds, st>>>(p); break;
    case 8: decode_gemv_fast_kernel<T, TO, GLU, 8><<<blocks, 256, lds, st>>>(p); break;
    default: decode_gemv_kernel<T, TO, GLU><<<blocks, 256, lds, st>>>(p); break;
  }
  VG_LAUNCH_CHECK();
  return VG_OK;
}

template <typename TO, bool GLU>
static int launch_decode_gemv_w8(DecGemvArgs p, hipStream_t st) {
  const auto [ppw, blocks] = dec_pair_split(GLU ? p.N : (p.N + 1) / 2, 4, DEC_MAX_PPW);
  p.ppw = ppw;
  const size_t lds = (size_t)p.K * 2;
  const int nchw = p.K / 16;               // weight chunks per row
  if (nchw % 256 == 0 && nchw / 256 == 1) decode_gemv_fast_kernel<bf16_t, TO, GLU, 1, 4, true><<<blocks, 256, lds, st>>>(p);
  else if (nchw % 256 == 0 && nchw / 256 == 2) decode_gemv_fast_kernel<bf16_t, TO, GLU, 2, 4, true><<<blocks, 256, lds, st>>>(p);
  else if (nchw == 7 * 128) decode_gemv_fast_kernel<bf16_t, TO, GLU, 7, 2, true><<<blocks, 256, lds, st>>>(p);
  else if (nchw == 3 * 64) decode_gemv_fast_kernel<bf16_t, TO, GLU, 3, 1, true><<<blocks, 256, lds, st>>>(p);
  else {
    vg_set_error("vg_decode_gemv_w8: K=%d is not one of the supported row lengths (3072, 4096, 8192, 14336)", p.K);
    return VG_ERR_UNSUPPORTED;
  }
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_decode_gemv_w8(const void* x, const uint8_t* W8, int64_t ldw, const float* wscale, void* y, const float* norm_w,
                                 float eps, const void* R, int N, int K, int glu, int out_dtype, vg_stream_t stream) {
  VG_CHECK(x && W8 && wscale && y && N > 0 && K > 0, VG_ERR_ARG, "vg_decode_gemv_w8: bad args N=%d K=%d", N, K);
  VG_CHECK(K % 16 == 0 && ldw % 16 == 0, VG_ERR_ARG, "vg_decode_gemv_w8: K/ldw must be multiples of 16 (K=%d ldw=%lld)", K, (long long)ldw);
  VG_CHECK(((uintptr_t)x & 15) == 0 && ((uintptr_t)W8 & 15) == 0 && ((uintptr_t)norm_w & 15) == 0, VG_ERR_ARG,
           "vg_decode_gemv_w8: x/W/norm_w must be 16-byte aligned");
  VG_CHECK((int64_t)K * 2 <= 64 * 1024, VG_ERR_UNSUPPORTED, "vg_decode_gemv_w8: K=%d does not fit the LDS staging", K);
  VG_CHECK(out_dtype == VG_BF16 || out_dtype == VG_F32, VG_ERR_ARG, "vg_decode_gemv_w8: bad out_dtype %d", out_dtype);
  DecGemvArgs p{x, W8, y, norm_w, R, N, K, ldw, eps, 1, wscale};
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == VG_BF16) return glu ? launch_decode_gemv_w8<bf16_t, true>(p, st) : launch_decode_gemv_w8<bf16_t, false>(p, st);
  return glu ? launch_decode_gemv_w8<float, true>(p, st) : launch_decode_gemv_w8<float, false>(p, st);
}

extern "C" int vg_decode_gemv(const void* x, const void* W, int64_t ldw, void* y, const float* norm_w, float eps,
                              const void* R, int N, int K, int glu, int in_dtype, int out_dtype, vg_stream_t stream) {
  VG_CHECK(x && W && y && N > 0 && K > 0, VG_ERR_ARG, "vg_decode_gemv: bad args N=%d K=%d", N, K);
  VG_CHECK(in_dtype == VG_BF16 || in_dtype == VG_F32, VG_ERR_ARG, "vg_decode_gemv: bad in_dtype %d", in_dtype);
  const int kpc = in_dtype == VG_BF16 ? 8 : 4, es = in_dtype == VG_BF16 ? 2 : 4;
  VG_CHECK(K % kpc == 0 && ldw % kpc == 0, VG_ERR_ARG, "vg_decode_gemv: K/ldw must be multiples of %d (K=%d ldw=%lld)", kpc, K, (long long)ldw);
  VG_CHECK(((uintptr_t)x & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)norm_w & 15) == 0, VG_ERR_ARG,
           "vg_decode_gemv: x/W/norm_w must be 16-byte aligned");
  VG_CHECK((int64_t)K * es <= 64 * 1024, VG_ERR_UNSUPPORTED, "vg_decode_gemv: K=%d does not fit the LDS staging", K);
  DecGemvArgs p{x, W, y, norm_w, R, N, K, ldw, eps, 1, nullptr};
  hipStream_t st = (hipStream_t)stream;
#define VG_DEC_GEMV(TI, TOO) return glu ? launch_decode_gemv<TI, TOO, true>(p, st) : launch_decode_gemv<TI, TOO, false>(p, st)
  if (in_dtype == VG_BF16 && out_dtype == VG_BF16) VG_DEC_GEMV(bf16_t, bf16_t);
  if (in_dtype == VG_BF16 && out_dtype == VG_F32) VG_DEC_GEMV(bf16_t, float);
  if (in_dtype == VG_F32 && out_dtype == VG_F32) VG_DEC_GEMV(float, float);
#undef VG_DEC_GEMV
  vg_set_error("vg_decode_gemv: unsupported dtype combination %d -> %d", in_dtype, out_dtype);
  return VG_ERR_UNSUPPORTED;
}

// ---- 13-bit bf16 rows: packer, unpacker and the GEMV entry point
// One workgroup per row: the exponent range of the row decides base_row and raw (phase 1), then thread (batch, lane) gathers the lane's 32
// weights of that batch and writes its 13 dwords into the four planes (phase 2).  A raw row's block is written all the same (codes mod 32).
__global__ __launch_bounds__(256) void dec_pack13_kernel(const uint16_t* W, int64_t ldw, int K, uint8_t* packed, float* scale, uint8_t* rawflag) {
  __shared__ int s_min, s_max, s_bad;
  const int tid = threadIdx.x, row = blockIdx.x, nb = K / 2048;
  const uint16_t* w = W + (int64_t)row * ldw;
  if (tid == 0) { s_min = 255; s_max = 0; s_bad = 0; }
  __syncthreads();
  int emin = 255, emax = 0, bad = 0;
  for (int c = tid; c < K / 8; c += 256) {
    const u32x4_t v = ((const u32x4_t*)w)[c];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t b = (v[j >> 1] >> (16 * (j & 1))) & 0xffffu, E = (b >> 7) & 255u;
      if (E == 255u || (E == 0u && (b & 127u))) bad = 1;
      else if (E) { emin = min(emin, (int)E); emax = max(emax, (int)E); }
    }
  }
  atomicMin(&s_min, emin);
  atomicMax(&s_max, emax);
  if (bad) atomicOr(&s_bad, 1);
  __syncthreads();
  const int base = s_min <= s_max ? s_min - 1 : 112;        // the smallest non-zero exponent takes code 1; a row of zeros: scale 1
  const bool raw = s_bad || s_max - base > 30 || base > 239;      // 2^(base - 112) = the fp32 with exponent field base + 15: normal up to 254
  if (tid == 0) {
    scale[row] = raw ? 1.f : __uint_as_float((uint32_t)(base + 15) << 23);
    rawflag[row] = raw;
  }
  for (int t = tid; t < nb * 64; t += 256) {
    const int cb = t >> 6, lane = t & 63;
    uint32_t H[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t L[3] = {0, 0, 0};                               // the 160-bit string, 64 bits at a time
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const u32x4_t v = ((const u32x4_t*)w)[cb * 256 + u * 64 + lane];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = 8 * u + j, bit = 5 * i;
        const uint32_t b = (v[j >> 1] >> (16 * (j & 1))) & 0xffffu, E = (b >> 7) & 255u;
        const uint32_t code = E ? (E - (uint32_t)base) & 31u : 0u;
        H[i >> 2] |= (((b >> 15) << 7) | (code << 2) | ((b >> 5) & 3u)) << (8 * (i & 3));
        const uint64_t lo5 = b & 31u;
        L[bit >> 6] |= lo5 << (bit & 63);
        if ((bit & 63) > 59) L[(bit >> 6) + 1] |= lo5 >> (64 - (bit & 63));
      }
    }
    uint8_t* blk = packed + ((int64_t)row * nb + cb) * DEC_P13_BLOCK;
    const u32x4_t h0 = {H[0], H[1], H[2], H[3]}, h1 = {H[4], H[5], H[6], H[7]};
    const u32x4_t l0 = {(uint32_t)L[0], (uint32_t)(L[0] >> 32), (uint32_t)L[1], (uint32_t)(L[1] >> 32)};
    ((u32x4_t*)blk)[lane] = h0;
    ((u32x4_t*)(blk + 1024))[lane] = h1;
    ((u32x4_t*)(blk + 2048))[lane] = l0;
    ((uint32_t*)(blk + 3072))[lane] = (uint32_t)L[2];
  }
}

// packed + scales + raw list + the original -> bf16 rows (the tests' inverse): a listed row is copied from the original
__global__ __launch_bounds__(256) void dec_unpack13_kernel(const uint8_t* packed, const float* scale, const int* raw, int nraw, const uint16_t* W,
                                                           int64_t ldw, uint16_t* out, int64_t ldo, int K) {
  __shared__ int s_raw;
  const int tid = threadIdx.x, row = blockIdx.x, nb = K / 2048;
  if (tid == 0) s_raw = 0;
  __syncthreads();
  for (int r = tid; r < nraw; r += 256)
    if (raw[r] == row) s_raw = 1;
  __syncthreads();
  uint16_t* o = out + (int64_t)row * ldo;
  if (s_raw) {
    for (int c = tid; c < K / 8; c += 256) ((u32x4_t*)o)[c] = ((const u32x4_t*)(W + (int64_t)row * ldw))[c];
    return;
  }
  const uint32_t base = (__float_as_uint(scale[row]) >> 23) - 15u;
  for (int t = tid; t < nb * 64; t += 256) {
    const int cb = t >> 6, lane = t & 63;
    const uint8_t* blk = packed + ((int64_t)row * nb + cb) * DEC_P13_BLOCK;
    const u32x4_t h0 = ((const u32x4_t*)blk)[lane], h1 = ((const u32x4_t*)(blk + 1024))[lane], l0 = ((const u32x4_t*)(blk + 2048))[lane];
    const uint32_t H[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    const uint64_t L[3] = {l0[0] | ((uint64_t)l0[1] << 32), l0[2] | ((uint64_t)l0[3] << 32), ((const uint32_t*)(blk + 3072))[lane]};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      u32x4_t v = {0, 0, 0, 0};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = 8 * u + j, bit = 5 * i;
        const uint32_t hb = (H[i >> 2] >> (8 * (i & 3))) & 255u, code = (hb >> 2) & 31u;
        uint64_t lo5 = L[bit >> 6] >> (bit & 63);
        if ((bit & 63) > 59) lo5 |= L[(bit >> 6) + 1] << (64 - (bit & 63));
        const uint32_t b = ((hb >> 7) << 15) | ((code ? code + base : 0u) << 7) | ((hb & 3u) << 5) | ((uint32_t)lo5 & 31u);
        v[j >> 1] |= b << (16 * (j & 1));
      }
      ((u32x4_t*)o)[cb * 256 + u * 64 + lane] = v;
    }
  }
}

extern "C" int64_t vg_decode_pack13_row_bytes(int K) { return K > 0 && K % 2048 == 0 ? (int64_t)(K / 2048) * DEC_P13_BLOCK : 0; }

extern "C" int vg_decode_pack13(const void* W, int64_t ldw, int N, int K, uint8_t* packed, float* scale, uint8_t* rawflag, vg_stream_t stream) {
  VG_CHECK(W && packed && scale && rawflag && N > 0, VG_ERR_ARG, "vg_decode_pack13: bad args N=%d K=%d", N, K);
  VG_CHECK(vg_decode_pack13_row_bytes(K) && ldw % 8 == 0 && ldw >= K, VG_ERR_ARG, "vg_decode_pack13: K=%d must be a multiple of 2048, ldw=%lld of 8",
           K, (long long)ldw);
  VG_CHECK(((uintptr_t)W & 15) == 0 && ((uintptr_t)packed & 15) == 0, VG_ERR_ARG, "vg_decode_pack13: W/packed must be 16-byte aligned");
  dec_pack13_kernel<<<N, 256, 0, (hipStream_t)stream>>>((const uint16_t*)W, ldw, K, packed, scale, rawflag);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_decode_unpack13(const uint8_t* packed, const float* scale, const int* raw, int nraw, const void* W, int64_t ldw, void* out,
                                  int64_t ldo, int N, int K, vg_stream_t stream) {
  VG_CHECK(packed && scale && W && out && N > 0 && nraw >= 0 && (raw || !nraw), VG_ERR_ARG, "vg_decode_unpack13: bad args N=%d K=%d nraw=%d", N, K, nraw);
  VG_CHECK(vg_decode_pack13_row_bytes(K) && ldw % 8 == 0 && ldw >= K && ldo % 8 == 0 && ldo >= K, VG_ERR_ARG,
           "vg_decode_unpack13: K=%d must be a multiple of 2048, ldw=%lld / ldo=%lld of 8", K, (long long)ldw, (long long)ldo);
  VG_CHECK(((uintptr_t)W & 15) == 0 && ((uintptr_t)packed & 15) == 0 && ((uintptr_t)out & 15) == 0, VG_ERR_ARG,
           "vg_decode_unpack13: W/packed/out must be 16-byte aligned");
  dec_unpack13_kernel<<<N, 256, 0, (hipStream_t)stream>>>(packed, scale, raw, nraw, (const uint16_t*)W, ldw, (uint16_t*)out, ldo, K);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_decode_gemv_p13_supported(int K) { return K == 4096 || K == 14336; }

template <typename TO, bool GLU>
static int launch_decode_gemv_p13(DecGemvArgs p, hipStream_t st) {
  const auto [ppw, blocks] = dec_pair_split(GLU ? p.N : (p.N + 1) / 2, 2, DEC_MAX_PPW);
  p.ppw = ppw;
  const size_t lds = (size_t)p.K * 2;
  if (p.K == 4096) decode_gemv_fast_kernel<bf16_t, TO, GLU, 2, 4, false, 0, true><<<blocks, 256, lds, st>>>(p);
  else decode_gemv_fast_kernel<bf16_t, TO, GLU, 7, 4, false, 0, true><<<blocks, 256, lds, st>>>(p);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_decode_gemv_p13(const void* x, const void* W, int64_t ldw, const uint8_t* packed, const float* scale, const int* raw, int nraw,
                                  void* y, const float* norm_w, float eps, const void* R, int N, int K, int glu, int out_dtype, vg_stream_t stream) {
  VG_CHECK(x && W && packed && scale && y && N > 0 && nraw >= 0 && (raw || !nraw), VG_ERR_ARG, "vg_decode_gemv_p13: bad args N=%d K=%d nraw=%d", N, K, nraw);
  VG_CHECK(vg_decode_gemv_p13_supported(K), VG_ERR_UNSUPPORTED, "vg_decode_gemv_p13: K=%d is not one of the supported row lengths (4096, 14336)", K);
  VG_CHECK(ldw % 8 == 0 && ldw >= K, VG_ERR_ARG, "vg_decode_gemv_p13: ldw=%lld must be a multiple of 8 and at least K=%d", (long long)ldw, K);
  VG_CHECK(((uintptr_t)x & 15) == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)packed & 15) == 0 && ((uintptr_t)norm_w & 15) == 0, VG_ERR_ARG,
           "vg_decode_gemv_p13: x/W/packed/norm_w must be 16-byte aligned");
  VG_CHECK(out_dtype == VG_BF16 || out_dtype == VG_F32, VG_ERR_ARG, "vg_decode_gemv_p13: bad out_dtype %d", out_dtype);
  DecGemvArgs p{x, W, y, norm_w, R, N, K, ldw, eps, 1, scale};
  p.Wp = packed;
  p.raw = raw;
  p.nraw = nraw;
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == VG_BF16) return glu ? launch_decode_gemv_p13<bf16_t, true>(p, st) : launch_decode_gemv_p13<bf16_t, false>(p, st);
  return glu ? launch_decode_gemv_p13<float, true>(p, st) : launch_decode_gemv_p13<float, false>(p, st);
}

// q|k|v projection of the new token with RMSNorm in front and RoPE + KV-cache append behind it (r06): the rows of a rotate-half pair
// (d, d + D/2) go to ONE lane of the GEMV's epilogue, so the rotation is two fmas on values that are in registers anyway, the new key / value
// rows are written where the attention kernel reads them, and that kernel (vg_decode_attention2) starts on its K / V loads instead of on a
// RoPE phase.  rope_cs = [cos row | sin row] of position *pos_dev (vg_decode_advance keeps it current): a fixed address, no dependent load.
extern "C" int vg_decode_qkv_rope_supported(int H, int Hkv, int D, int K, int dtype) {
  if (H <= 0 || Hkv <= 0 || D != 128) return 0;
  if (dtype == VG_BF16) return K == 4096 || K == 2048;
  if (dtype == VG_F32) return K == 4096;
  return 0;
}

template <typename T, int NB, typename KVO = T>
static int launch_decode_qkv_rope(DecGemvArgs p, hipStream_t st) {
  const auto [ppw, blocks] = dec_pair_split(p.N / 2, 2, DEC_MAX_PPW);
  p.ppw = ppw;
  decode_gemv_fast_kernel<T, T, false, NB, 4, false, 64, false, KVO><<<blocks, 256, (size_t)p.K * sizeof(T), st>>>(p);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

// fn: the entry point's name for the messages.  KV: the caches' element type — void = the activation dtype, kv8_t = e4m3 codes (kv_cache =
// "fp8_rope", DESIGN 8c: bf16 activations only; the same kernel, the key / value pairs stored by kv8_store_pair, q_out with the bf16 cache's bits)
template <typename KV>
static int decode_qkv_rope(const char* fn, const void* x, const void* Wqkv, int64_t ldw, const float* norm_w, float eps, void* q_out, void* k_cache,
                           void* v_cache, const float* rope_cs, const int* pos_dev, int H, int Hkv, int D, int K, int dtype, vg_stream_t stream) {
  constexpr bool KV8 = std::is_same<KV, kv8_t>::value;
  VG_CHECK(x && Wqkv && q_out && k_cache && v_cache && rope_cs && pos_dev, VG_ERR_ARG, "%s: null pointer", fn);
  VG_CHECK((!KV8 || dtype == VG_BF16) && vg_decode_qkv_rope_supported(H, Hkv, D, K, dtype), VG_ERR_UNSUPPORTED,
           "%s: H=%d Hkv=%d D=%d K=%d dtype=%d not covered%s", fn, H, Hkv, D, K, dtype, KV8 ? " (bf16 only)" : "");
  const int kpc = dtype == VG_BF16 ? 8 : 4;
  VG_CHECK(ldw % kpc == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)Wqkv & 15) == 0 && ((uintptr_t)norm_w & 15) == 0, VG_ERR_ARG,
           "%s: alignment (16 bytes; ldw a multiple of %d)", fn, kpc);
  DecGemvArgs p{x, Wqkv, q_out, norm_w, nullptr, (H + 2 * Hkv) * D, K, ldw, eps, 1, nullptr, rope_cs, pos_dev, k_cache, v_cache, H, Hkv};
  hipStream_t st = (hipStream_t)stream;
  if constexpr (KV8) {
    return K == 4096 ? launch_decode_qkv_rope<bf16_t, 2, kv8_t>(p, st) : launch_decode_qkv_rope<bf16_t, 1, kv8_t>(p, st);
  } else {
    if (dtype == VG_BF16) return K == 4096 ? launch_decode_qkv_rope<bf16_t, 2>(p, st) : launch_decode_qkv_rope<bf16_t, 1>(p, st);
    return launch_decode_qkv_rope<float, 4>(p, st);
  }
}

extern "C" int vg_decode_qkv_rope(const void* x, const void* Wqkv, int64_t ldw, const float* norm_w, float eps, void* q_out, void* k_cache,
                                  void* v_cache, const float* rope_cs, const int* pos_dev, int H, int Hkv, int D, int K, int dtype,
                                  vg_stream_t stream) {
  return decode_qkv_rope<void>("vg_decode_qkv_rope", x, Wqkv, ldw, norm_w, eps, q_out, k_cache, v_cache, rope_cs, pos_dev, H, Hkv, D, K, dtype, stream);
}

extern "C" int vg_decode_qkv_rope_kv8(const void* x, const void* Wqkv, int64_t ldw, const float* norm_w, float eps, void* q_out, uint8_t* k_cache,
                                      uint8_t* v_cache, const float* rope_cs, const int* pos_dev, int H, int Hkv, int D, int K, int dtype,
                                      vg_stream_t stream) {
  return decode_qkv_rope<kv8_t>("vg_decode_qkv_rope_kv8", x, Wqkv, ldw, norm_w, eps, q_out, k_cache, v_cache, rope_cs, pos_dev, H, Hkv, D, K, dtype,
                                stream);
}

// ---------------------------------------------------------------------------------------------------------------
// B-row forms of vg_decode_gemv / vg_decode_qkv_rope (the batched multi-prompt decode step): one weight pair is loaded once and applied
// to the BR rows of x.  Every row sees exactly the single-row kernel's arithmetic: the same RMSNorm prologue (256 threads, XN chunks per thread, wave
// sums, the 4-wave total), the same lane -> chunk walk (batch cb, chunk u: lane + 64 u + 256 cb) with one fp32 accumulator per (row, pair row) fed
// dec_dot in that order, the same wave_sum and the same epilogue — so row r of the result is bit-identical to vg_decode_gemv on row r alone.
// Which wave owns which pair does not enter the sums (the split is free).  x is staged into LDS as bf16 rows; when B x K x 2 bytes exceed the
// budget the K batches are staged in phases and each wave owns one pair, its accumulators carried across the phases (the order stays).
// NB = 3, CPB = 2 (K = 3072, Phi-3-mini's hidden size): decode_gemv_fast_kernel<..., 3, 2>'s walk — batches of 128 chunks (chunk u: lane + 64 u + 128 cb)
// and a norm prologue whose second chunk per thread is partial (threads 0..127 only).
constexpr int DEC_ROWS_PPW = 8, DEC_ROWS_LDS = 64 * 1024;

struct DecRowsArgs {
  const void* x; int64_t ldx; const void* W; int64_t ldw; void* y; int64_t ldy; const float* nw; float eps; const void* R; int64_t ldr;
  int N, K, B, ppw, nph;
  // RoPE form: rope_cs [B][2][RHD] fp32, pos [B]; row r's key / value rows go to slot r: kc + r * slot_stride + (pos[r] - row0) * Hkv * 2 RHD
  const float* rope_cs; const int* pos; void* kc; void* vc; int64_t slot_stride; int row0, slot_rows, H, Hkv;
};

template <int NB> constexpr int dec_rows_cpb() { return NB == 3 ? 2 : 4; }     // chunks per lane per batch: 2 only at K = 3072

template <typename TO, bool GLU, int NB, int BR, int RHD, typename KVO = TO>
__global__ __launch_bounds__(256) void decode_gemv_rows_kernel(DecRowsArgs p) {
  typedef bf16_t T;
  constexpr int CPB = dec_rows_cpb<NB>(), KPC = 8, NWV = 2;
  constexpr int BC = CPB * 64;                     // chunks per batch
  constexpr int NCH = NB * BC, XN = (NCH + 255) / 256;     // the last chunk per thread may be partial (NCH % 256 == 128)
  extern __shared__ __attribute__((aligned(16))) char dec_smem[];
  __shared__ float red[BR][4];
  __shared__ float res[4][DEC_ROWS_PPW][BR][2];
  u32x4_t* xs = (u32x4_t*)dec_smem;                // [BR][nph * BC] chunks of the current phase
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int npair = RHD > 0 ? p.N / 2 : GLU ? p.N : (p.N + 1) / 2;
  const int p0 = (blockIdx.x * 4 + wave) * p.ppw;
  const int np = max(min(p0 + p.ppw, npair) - p0, 0);
  const T* W = (const T*)p.W;
  const int pch = p.nph * BC;                      // chunks per row per phase

  float rstd[BR];
#pragma unroll
  for (int r = 0; r < BR; ++r) rstd[r] = 1.f;
  if (p.nw) {                                      // the norm needs the whole row: the launcher keeps nph = NB
#pragma unroll
    for (int r = 0; r < BR; ++r) {
      const u32x4_t* xg = (const u32x4_t*)((const T*)p.x + (int64_t)min(r, p.B - 1) * p.ldx);
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < XN; ++i) {
        if (NCH % 256 == 0 || tid + 256 * i < NCH) {
          float f[KPC];
          dec_unpack<T>(xg[tid + 256 * i], f);
#pragma unroll
          for (int e = 0; e < KPC; ++e) ss += f[e] * f[e];
        }
      }
      ss = wave_sum(ss);
      if (lane == 0) red[r][wave] = ss;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < BR; ++r) rstd[r] = rsqrtf((red[r][0] + red[r][1] + red[r][2] + red[r][3]) / (float)p.K + p.eps);
  }

  float a0[BR], a1[BR];
#pragma unroll
  for (int r = 0; r < BR; ++r) { a0[r] = 0.f; a1[r] = 0.f; }
  for (int ph = 0; ph < NB; ph += p.nph) {
    const int nbp = min(p.nph, NB - ph);
    if (ph > 0) __syncthreads();                   // every wave is done with the previous phase's rows
    // ---- stage rows' chunks [ph * BC, (ph + nbp) * BC)
    for (int c = tid; c < nbp * BC; c += 256) {
      const int gc = ph * BC + c;
#pragma unroll
      for (int r = 0; r < BR; ++r) {
        u32x4_t v = ((const u32x4_t*)((const T*)p.x + (int64_t)min(r, p.B - 1) * p.ldx))[gc];
        if (p.nw) {
          float f[KPC];
          dec_unpack<T>(v, f);
          const f32x4_t* nw4 = (const f32x4_t*)p.nw + gc * NWV;
#pragma unroll
          for (int e = 0; e < KPC; ++e) f[e] = dec_round<T>(f[e] * rstd[r]) * nw4[e / 4][e % 4];
          v = dec_pack<T>(f);
        }
        xs[r * pch + c] = v;
      }
    }
    __syncthreads();
    // ---- the stream: flat (pair, batch-of-phase) sequence, two batches in flight
    const int total = np * nbp;
    auto issue = [&](u32x4_t (&v0)[CPB], u32x4_t (&v1)[CPB], int it) {
      const int pc = p0 + it / nbp, cb = ph + it % nbp;
      const int n0 = RHD > 0 ? (pc / max(RHD, 1)) * (2 * RHD) + pc % max(RHD, 1) : GLU ? pc : 2 * pc;
      const int n1 = RHD > 0 ? n0 + RHD : GLU ? p.N + pc : min(2 * pc + 1, p.N - 1);
      const u32x4_t* w0 = (const u32x4_t*)(W + (int64_t)n0 * p.ldw) + cb * (64 * CPB) + lane;
      const u32x4_t* w1 = (const u32x4_t*)(W + (int64_t)n1 * p.ldw) + cb * (64 * CPB) + lane;
#pragma unroll
      for (int u = 0; u < CPB; ++u) {
        v0[u] = __builtin_nontemporal_load(w0 + u * 64);
        v1[u] = __builtin_nontemporal_load(w1 + u * 64);
      }
    };
    auto consume = [&](const u32x4_t (&v0)[CPB], const u32x4_t (&v1)[CPB], int it) {
      const int li = it / nbp, cbl = it % nbp;
#pragma unroll
      for (int r = 0; r < BR; ++r) {               // row-outer keeps one row's x chunks live at a time; each row's sum order is the single-row one
#pragma unroll
        for (int u = 0; u < CPB; ++u) {
          const u32x4_t xv = xs[r * pch + cbl * (64 * CPB) + u * 64 + lane];
          a0[r] += dec_dot<T>(v0[u], xv);
          a1[r] += dec_dot<T>(v1[u], xv);
        }
      }
      if (cbl == nbp - 1 && ph + nbp == NB) {      // the pair's last batch
#pragma unroll
        for (int r = 0; r < BR; ++r) {
          const float s0 = wave_sum(a0[r]), s1 = wave_sum(a1[r]);
          if (lane == 0) { res[wave][li][r][0] = s0; res[wave][li][r][1] = s1; }
          a0[r] = 0.f;
          a1[r] = 0.f;
        }
      }
    };
    u32x4_t va0[CPB], va1[CPB], vb0[CPB], vb1[CPB];
    if (total > 0) issue(va0, va1, 0);
    if (total > 1) issue(vb0, vb1, 1);
    int it = 0;
    for (; it + 1 < total; it += 2) {
      consume(va0, va1, it);
      if (it + 2 < total) issue(va0, va1, it + 2);
      consume(vb0, vb1, it + 1);
      if (it + 3 < total) issue(vb0, vb1, it + 3);
    }
    if (it < total) consume(va0, va1, it);
  }
  // ---- epilogue: one lane per (pair, row); the single-row kernel's stores
  for (int i = lane; i < np * BR; i += 64) {
    const int li = i / BR, r = i % BR, pi = p0 + li;
    if (r >= p.B) continue;
    if constexpr (RHD > 0) {
      constexpr bool KV8O = std::is_same<KVO, kv8_t>::value;      // byte K/V slots (vg_decode_qkv_rope_rows_kv8)
      const int pos = p.pos[r];
      const int srow = min(max(pos - p.row0, 0), p.slot_rows - 1);    // a slot's rows only, whatever the position word holds
      const int hh = pi / RHD, d = pi % RHD;
      const float x1 = dec_round<TO>(res[wave][li][r][0]), x2 = dec_round<TO>(res[wave][li][r][1]);
      float o1 = x1, o2 = x2;
      TO* dst;
      if (hh < p.H + p.Hkv) {
        const float c = p.rope_cs[r * 2 * RHD + d], sv = p.rope_cs[r * 2 * RHD + RHD + d];
        const float cb = bf2f(f2bf(c)), sb = bf2f(f2bf(sv));
        o1 = bf2f(f2bf(x1 * cb)) + bf2f(f2bf(-x2 * sb));
        o2 = bf2f(f2bf(x2 * cb)) + bf2f(f2bf(x1 * sb));
        if constexpr (KV8O) {
          if (hh >= p.H) {
            kv8_store_pair((KVO*)p.kc + r * p.slot_stride + ((int64_t)srow * p.Hkv + (hh - p.H)) * (2 * RHD) + d, RHD, o1, o2);
            continue;
          }
        }
        dst = hh < p.H ? (TO*)p.y + r * p.ldy + (int64_t)hh * (2 * RHD)
                       : (TO*)p.kc + r * p.slot_stride + ((int64_t)srow * p.Hkv + (hh - p.H)) * (2 * RHD);
      } else {
        if constexpr (KV8O) {
          kv8_store_pair((KVO*)p.vc + r * p.slot_stride + ((int64_t)srow * p.Hkv + (hh - p.H - p.Hkv)) * (2 * RHD) + d, RHD, o1, o2);
          continue;
        }
        dst = (TO*)p.vc + r * p.slot_stride + ((int64_t)srow * p.Hkv + (hh - p.H - p.Hkv)) * (2 * RHD);
      }
      vg_elt<TO>::st(dst + d, o1);
      vg_elt<TO>::st(dst + d + RHD, o2);
    } else {
      DecGemvArgs q{};
      q.y = (TO*)p.y + r * p.ldy;
      q.R = p.R ? (const void*)((const TO*)p.R + r * p.ldr) : nullptr;
      q.N = p.N;
      dec_gemv_store<T, TO, GLU>(q, pi, res[wave][li][r][0], res[wave][li][r][1]);
    }
  }
}

// batches per row at K = 2048 x {1, 2, 4, 7, 8} (four chunks per lane per batch)
static int dec_rows_nb4(int K) {
  const int nch = K / 8;
  if (K % 2048) return 0;
  const int nb = nch / 256;
  return nb == 1 || nb == 2 || nb == 4 || nb == 7 || nb == 8 ? nb : 0;
}

static int dec_rows_nb(int K) {
  return K == 3072 ? 3 : dec_rows_nb4(K);         // 3072 (Phi-3-mini's hidden size): three batches of two chunks per lane (CPB = 2)
}

extern "C" int vg_decode_rows_supported(int H, int Hkv, int D, int hidden, int inter, int dtype) {
  return dtype == VG_BF16 && vg_decode_qkv_rope_supported(H, Hkv, D, hidden, dtype) && dec_rows_nb4(hidden) && dec_rows_nb4(inter) && (H * D) == hidden;
}

template <typename TO, bool GLU, int NB, int BR, int RHD, typename KVO = TO>
static int launch_rows_b(DecRowsArgs p, hipStream_t st) {
  const int npair = RHD > 0 ? p.N / 2 : GLU ? p.N : (p.N + 1) / 2;
  constexpr int BBYTES = dec_rows_cpb<NB>() * 64 * 16;     // bytes of one row's batch of chunks
  // x staging: the whole row when it fits the budget (always with the norm), else phases of batches with one pair per wave
  int nph = NB;
  if (!p.nw && (int64_t)BR * NB * BBYTES > DEC_ROWS_LDS) nph = max(1, DEC_ROWS_LDS / (BR * BBYTES));
  const auto [ppw, blocks] = dec_rows_split(npair, nph < NB, DEC_ROWS_PPW);
  p.nph = nph;
  p.ppw = ppw;
  const size_t lds = (size_t)BR * nph * BBYTES;
  vg_raise_lds_cap<decode_gemv_rows_kernel<TO, GLU, NB, BR, RHD, KVO>>(lds);
  decode_gemv_rows_kernel<TO, GLU, NB, BR, RHD, KVO><<<blocks, 256, lds, st>>>(p);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

template <typename TO, bool GLU, int NB, int RHD, typename KVO = TO>
static int launch_rows_nb(DecRowsArgs p, hipStream_t st) {
  return dec_with_bucket(p.B, [&](auto br) { return launch_rows_b<TO, GLU, NB, decltype(br)::value, RHD, KVO>(p, st); });
}

template <bool GLU>
static int launch_rows(DecRowsArgs p, hipStream_t st) {
  switch (dec_rows_nb(p.K)) {
    case 1: return launch_rows_nb<bf16_t, GLU, 1, 0>(p, st);
    case 3: return launch_rows_nb<bf16_t, GLU, 3, 0>(p, st);
    case 2: return launch_rows_nb<bf16_t, GLU, 2, 0>(p, st);
    case 4: return launch_rows_nb<bf16_t, GLU, 4, 0>(p, st);
    case 7: return launch_rows_nb<bf16_t, GLU, 7, 0>(p, st);
    default: return launch_rows_nb<bf16_t, GLU, 8, 0>(p, st);
  }
}

extern "C" int vg_decode_gemv_rows(const void* x, int64_t ldx, const void* W, int64_t ldw, void* y, int64_t ldy, const float* norm_w, float eps,
                                   const void* R, int64_t ldr, int N, int K, int B, int glu, int dtype, vg_stream_t stream) {
  VG_CHECK(x && W && y && N > 0 && dec_rows_b_ok(B), VG_ERR_ARG, "vg_decode_gemv_rows: bad args N=%d B=%d", N, B);
  VG_CHECK(dtype == VG_BF16 && dec_rows_nb(K), VG_ERR_UNSUPPORTED, "vg_decode_gemv_rows: bf16 rows of K = 3072 or 2048 x {1, 2, 4, 7, 8} only (K=%d dtype=%d)", K, dtype);
  VG_CHECK(ldw % 8 == 0 && ldx % 8 == 0 && ((((uintptr_t)x) | ((uintptr_t)W) | ((uintptr_t)norm_w)) & 15) == 0, VG_ERR_ARG,
           "vg_decode_gemv_rows: alignment (16 bytes; ldx / ldw multiples of 8)");
  const int br = dec_bucket(B);      // the bucket the kernel stages
  VG_CHECK(!norm_w || (int64_t)br * K * 2 <= 160 * 1024 - 8 * 1024, VG_ERR_UNSUPPORTED,
           "vg_decode_gemv_rows: the norm stages the whole rows of the %d-row bucket: B=%d K=%d do not fit", br, B, K);
  DecRowsArgs p{x, ldx, W, ldw, y, ldy, norm_w, eps, R, ldr, N, K, B, 1, 1};
  hipStream_t st = (hipStream_t)stream;
  return glu ? launch_rows<true>(p, st) : launch_rows<false>(p, st);
}

// fn: the entry point's name for the messages.  KV: the slots' element type — bf16, or kv8_t = e4m3 codes: slot_stride in elements = bytes
// (a multiple of 8, as the attention's loads need)
template <typename KV>
static int decode_qkv_rope_rows(const char* fn, const void* x, int64_t ldx, const void* Wqkv, int64_t ldw, const float* norm_w, float eps, void* q_out,
                                int64_t ldq, void* k_slots, void* v_slots, int64_t slot_stride, int row0, int slot_rows, const float* rope_cs,
                                const int* pos, int H, int Hkv, int D, int K, int B, int dtype, vg_stream_t stream) {
  VG_CHECK(x && Wqkv && q_out && k_slots && v_slots && rope_cs && pos && dec_rows_b_ok(B) && slot_rows > 0, VG_ERR_ARG,
           "%s: bad args B=%d slot_rows=%d", fn, B, slot_rows);
  VG_CHECK(dtype == VG_BF16 && vg_decode_qkv_rope_supported(H, Hkv, D, K, dtype), VG_ERR_UNSUPPORTED,
           "%s: H=%d Hkv=%d D=%d K=%d dtype=%d not covered", fn, H, Hkv, D, K, dtype);
  const bool aligned = ldw % 8 == 0 && ldx % 8 == 0 && ((((uintptr_t)x) | ((uintptr_t)Wqkv) | ((uintptr_t)norm_w)) & 15) == 0;
  if constexpr (std::is_same<KV, kv8_t>::value)
    VG_CHECK(aligned && slot_stride % 8 == 0 && slot_stride >= (int64_t)slot_rows * Hkv * D, VG_ERR_ARG,
             "%s: alignment (16 bytes; ldx / ldw / slot_stride multiples of 8; slots must not overlap)", fn);
  else
    VG_CHECK(aligned, VG_ERR_ARG, "%s: alignment (16 bytes; ldx / ldw multiples of 8)", fn);
  DecRowsArgs p{x, ldx, Wqkv, ldw, q_out, ldq, norm_w, eps, nullptr, 0, (H + 2 * Hkv) * D, K, B, 1, 1,
                rope_cs, pos, k_slots, v_slots, slot_stride, row0, slot_rows, H, Hkv};
  hipStream_t st = (hipStream_t)stream;
  return K == 4096 ? launch_rows_nb<bf16_t, false, 2, 64, KV>(p, st) : launch_rows_nb<bf16_t, false, 1, 64, KV>(p, st);
}

extern "C" int vg_decode_qkv_rope_rows(const void* x, int64_t ldx, const void* Wqkv, int64_t ldw, const float* norm_w, float eps, void* q_out,
                                       int64_t ldq, void* k_slots, void* v_slots, int64_t slot_stride, int row0, int slot_rows, const float* rope_cs,
                                       const int* pos, int H, int Hkv, int D, int K, int B, int dtype, vg_stream_t stream) {
  return decode_qkv_rope_rows<bf16_t>("vg_decode_qkv_rope_rows", x, ldx, Wqkv, ldw, norm_w, eps, q_out, ldq, k_slots, v_slots, slot_stride, row0,
                                      slot_rows, rope_cs, pos, H, Hkv, D, K, B, dtype, stream);
}

extern "C" int vg_decode_qkv_rope_rows_kv8(const void* x, int64_t ldx, const void* Wqkv, int64_t ldw, const float* norm_w, float eps, void* q_out,
                                           int64_t ldq, uint8_t* k_slots, uint8_t* v_slots, int64_t slot_stride, int row0, int slot_rows,
                                           const float* rope_cs, const int* pos, int H, int Hkv, int D, int K, int B, int dtype, vg_stream_t stream) {
  return decode_qkv_rope_rows<kv8_t>("vg_decode_qkv_rope_rows_kv8", x, ldx, Wqkv, ldw, norm_w, eps, q_out, ldq, k_slots, v_slots, slot_stride, row0,
                                     slot_rows, rope_cs, pos, H, Hkv, D, K, B, dtype, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// B-row form of vg_decode_gemv_w8 (fp8 e4m3 weights with per-row scales; the MLP and the lm_head of the batched step with fp8 decode weights,
// DESIGN 11): every weight chunk is loaded once and applied to the BR rows of x, and row r of the result is bit-identical to vg_decode_gemv_w8 on
// row r alone.  The single-row kernel walks a weight row as the flat sequence of 64-chunk steps s = cb * CPB + u (weight chunk wc = 64 s + lane
// against the x chunks 2 wc and 2 wc + 1), one fp32 accumulator per pair row fed dec_dot_w8 in that order — so only the ORDER of the steps enters
// the sums, and how they are grouped into load batches is free (launch_w8_rows_k picks two chunks per lane per batch where the single-row kernel
// has four).  The norm prologue is decode_gemv_fast_kernel's for that K (256 threads, the same x chunks per thread, wave sums, the 4-wave total, dec_round before the norm weight), the scale and the epilogue are
// dec_gemv_store's.  x is staged as bf16 rows with the even and the odd x chunks of a row in two planes ([BR][2][chunks]: a lane's two 16-byte
// reads per weight chunk are then 16 bytes apart from its neighbours' instead of 32); phases as in decode_gemv_rows_kernel when B x K x 2 bytes
// exceed the budget and there is no norm.
struct DecRowsW8Args {
  const void* x; int64_t ldx; const uint8_t* W; int64_t ldw; const float* wscale; void* y; int64_t ldy; const float* nw; float eps;
  const void* R; int64_t ldr; int N, K, B, ppw, nph;
};

template <typename TO, bool GLU, int NB, int CPB, int BR>
__global__ __launch_bounds__(256) void decode_gemv_w8_rows_kernel(DecRowsW8Args p) {
  typedef bf16_t T;
  constexpr int KPC = 8, NWV = 2;
  constexpr int BC = CPB * 64;                     // WEIGHT chunks per batch (16 K elements each = two x chunks)
  constexpr int NCH = NB * BC * 2, XN = (NCH + 255) / 256;     // x chunks per row; the last one per thread may be partial (K = 3072)
  extern __shared__ __attribute__((aligned(16))) char dec_smem[];
  __shared__ float red[BR][4];
  __shared__ float res[4][DEC_ROWS_PPW][BR][2];
  u32x4_t* xs = (u32x4_t*)dec_smem;                // [BR][2][nph * BC]: x chunk 2 wc + h of the phase at plane h, index wc
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int npair = GLU ? p.N : (p.N + 1) / 2;
  const int p0 = (blockIdx.x * 4 + wave) * p.ppw;
  const int np = max(min(p0 + p.ppw, npair) - p0, 0);
  const uint8_t* W = p.W;
  const int pch = p.nph * BC;                      // weight chunks per row per phase

  float rstd[BR];
#pragma unroll
  for (int r = 0; r < BR; ++r) rstd[r] = 1.f;
  if (p.nw) {                                      // the launcher keeps nph = NB with a norm (whole rows)
#pragma unroll
    for (int r = 0; r < BR; ++r) {
      const u32x4_t* xg = (const u32x4_t*)((const T*)p.x + (int64_t)min(r, p.B - 1) * p.ldx);
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < XN; ++i) {
        if (NCH % 256 == 0 || tid + 256 * i < NCH) {
          float f[KPC];
          dec_unpack<T>(xg[tid + 256 * i], f);
#pragma unroll
          for (int e = 0; e < KPC; ++e) ss += f[e] * f[e];
        }
      }
      ss = wave_sum(ss);
      if (lane == 0) red[r][wave] = ss;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < BR; ++r) rstd[r] = rsqrtf((red[r][0] + red[r][1] + red[r][2] + red[r][3]) / (float)p.K + p.eps);
  }

  float a0[BR], a1[BR];
#pragma unroll
  for (int r = 0; r < BR; ++r) { a0[r] = 0.f; a1[r] = 0.f; }
  for (int ph = 0; ph < NB; ph += p.nph) {
    const int nbp = min(p.nph, NB - ph);
    if (ph > 0) __syncthreads();                   // every wave is done with the previous phase's rows
    // ---- stage the rows' x chunks [2 ph BC, 2 (ph + nbp) BC)
    for (int c = tid; c < nbp * BC * 2; c += 256) {
      const int gc = ph * BC * 2 + c;
#pragma unroll
      for (int r = 0; r < BR; ++r) {
        u32x4_t v = ((const u32x4_t*)((const T*)p.x + (int64_t)min(r, p.B - 1) * p.ldx))[gc];
        if (p.nw) {
          float f[KPC];
          dec_unpack<T>(v, f);
          const f32x4_t* nw4 = (const f32x4_t*)p.nw + gc * NWV;
#pragma unroll
          for (int e = 0; e < KPC; ++e) f[e] = dec_round<T>(f[e] * rstd[r]) * nw4[e / 4][e % 4];
          v = dec_pack<T>(f);
        }
        xs[(2 * r + (c & 1)) * pch + (c >> 1)] = v;
      }
    }
    __syncthreads();
    // ---- the stream: flat (pair, batch-of-phase) sequence, two batches in flight
    const int total = np * nbp;
    auto issue = [&](u32x4_t (&v0)[CPB], u32x4_t (&v1)[CPB], int it) {
      const int pc = p0 + it / nbp, cb = ph + it % nbp;
      const int n0 = GLU ? pc : 2 * pc;
      const int n1 = GLU ? p.N + pc : min(2 * pc + 1, p.N - 1);
      const u32x4_t* w0 = (const u32x4_t*)(W + (int64_t)n0 * p.ldw) + cb * BC + lane;
      const u32x4_t* w1 = (const u32x4_t*)(W + (int64_t)n1 * p.ldw) + cb * BC + lane;
#pragma unroll
      for (int u = 0; u < CPB; ++u) {
        v0[u] = __builtin_nontemporal_load(w0 + u * 64);
        v1[u] = __builtin_nontemporal_load(w1 + u * 64);
      }
    };
    auto consume = [&](const u32x4_t (&v0)[CPB], const u32x4_t (&v1)[CPB], int it) {
      const int li = it / nbp, cbl = it % nbp;
#pragma unroll
      for (int r = 0; r < BR; ++r) {               // row-outer: one row's x chunks live at a time; each row's sum order is the single-row one
#pragma unroll
        for (int u = 0; u < CPB; ++u) {
          const int wcl = cbl * BC + u * 64 + lane;
          const u32x4_t xa = xs[(2 * r) * pch + wcl], xb = xs[(2 * r + 1) * pch + wcl];
          a0[r] += dec_dot_w8(v0[u], xa, xb);
          a1[r] += dec_dot_w8(v1[u], xa, xb);
        }
      }
      if (cbl == nbp - 1 && ph + nbp == NB) {      // the pair's last batch
#pragma unroll
        for (int r = 0; r < BR; ++r) {
          const float s0 = wave_sum(a0[r]), s1 = wave_sum(a1[r]);
          if (lane == 0) { res[wave][li][r][0] = s0; res[wave][li][r][1] = s1; }
          a0[r] = 0.f;
          a1[r] = 0.f;
        }
      }
    };
    u32x4_t va0[CPB], va1[CPB], vb0[CPB], vb1[CPB];
    if (total > 0) issue(va0, va1, 0);
    if (total > 1) issue(vb0, vb1, 1);
    int it = 0;
    for (; it + 1 < total; it += 2) {
      consume(va0, va1, it);
      if (it + 2 < total) issue(va0, va1, it + 2);
      consume(vb0, vb1, it + 1);
      if (it + 3 < total) issue(vb0, vb1, it + 3);
    }
    if (it < total) consume(va0, va1, it);
  }
  // ---- epilogue: one lane per (pair, row); the single-row kernel's scale and stores
  for (int i = lane; i < np * BR; i += 64) {
    const int li = i / BR, r = i % BR;
    if (r >= p.B) continue;
    DecGemvArgs q{};
    q.y = (TO*)p.y + r * p.ldy;
    q.R = p.R ? (const void*)((const TO*)p.R + r * p.ldr) : nullptr;
    q.N = p.N;
    q.wscale = p.wscale;
    dec_gemv_store<T, TO, GLU>(q, p0 + li, res[wave][li][r][0], res[wave][li][r][1]);
  }
}

// the row lengths of vg_decode_gemv_w8's fast walk
extern "C" int vg_decode_gemv_w8_rows_supported(int K) { return K == 3072 || K == 4096 || K == 8192 || K == 14336; }

template <typename TO, bool GLU, int NB, int CPB, int BR>
static int launch_w8_rows_b(DecRowsW8Args p, hipStream_t st) {
  const int npair = GLU ? p.N : (p.N + 1) / 2;
  constexpr int BBYTES = CPB * 64 * 32;            // bytes of x under one row's batch of weight chunks
  // x staging: the whole row when it fits the budget (always with the norm), else phases of batches with one pair per wave
  int nph = NB;
  if (!p.nw && (int64_t)BR * NB * BBYTES > DEC_ROWS_LDS) nph = max(1, DEC_ROWS_LDS / (BR * BBYTES));
  const auto [ppw, blocks] = dec_rows_split(npair, nph < NB, DEC_ROWS_PPW);
  p.nph = nph;
  p.ppw = ppw;
  const size_t lds = (size_t)BR * nph * BBYTES;
  vg_raise_lds_cap<decode_gemv_w8_rows_kernel<TO, GLU, NB, CPB, BR>>(lds);
  decode_gemv_w8_rows_kernel<TO, GLU, NB, CPB, BR><<<blocks, 256, lds, st>>>(p);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

// Load batches per K: vg_decode_gemv_w8's (3, 1) and (7, 2) at K = 3072 and 14336; its batches of four chunks per lane at K = 4096 and 8192 are
// split in two — (2, 2) and (4, 2): the same steps in the same order, so every sum keeps its bits — because the fp8 -> fp32 conversions of a batch
// are shared by the B rows and four chunks of two weight rows converted (128 registers) leave no room for the rows' accumulators, and because one
// batch of a 16-row bucket then fits the staging budget
template <typename TO, bool GLU, int BR>
static int launch_w8_rows_k(DecRowsW8Args p, hipStream_t st) {
  switch (p.K) {
    case 3072: return launch_w8_rows_b<TO, GLU, 3, 1, BR>(p, st);
    case 4096: return launch_w8_rows_b<TO, GLU, 2, 2, BR>(p, st);
    case 8192: return launch_w8_rows_b<TO, GLU, 4, 2, BR>(p, st);
    default: return launch_w8_rows_b<TO, GLU, 7, 2, BR>(p, st);
  }
}

template <typename TO, bool GLU>
static int launch_w8_rows(DecRowsW8Args p, hipStream_t st) {
  return dec_with_bucket(p.B, [&](auto br) { return launch_w8_rows_k<TO, GLU, decltype(br)::value>(p, st); });
}

extern "C" int vg_decode_gemv_w8_rows(const void* x, int64_t ldx, const uint8_t* W8, int64_t ldw, const float* wscale, void* y, int64_t ldy,
                                      const float* norm_w, float eps, const void* R, int64_t ldr, int N, int K, int B, int glu, int out_dtype,
                                      vg_stream_t stream) {
  VG_CHECK(x && W8 && wscale && y && N > 0 && dec_rows_b_ok(B), VG_ERR_ARG, "vg_decode_gemv_w8_rows: bad args N=%d B=%d", N, B);
  VG_CHECK(vg_decode_gemv_w8_rows_supported(K), VG_ERR_UNSUPPORTED,
           "vg_decode_gemv_w8_rows: K=%d is not one of the supported row lengths (3072, 4096, 8192, 14336)", K);
  VG_CHECK(out_dtype == VG_BF16 || out_dtype == VG_F32, VG_ERR_ARG, "vg_decode_gemv_w8_rows: bad out_dtype %d", out_dtype);
  VG_CHECK(ldw % 16 == 0 && ldx % 8 == 0 && ((((uintptr_t)x) | ((uintptr_t)W8) | ((uintptr_t)norm_w)) & 15) == 0, VG_ERR_ARG,
           "vg_decode_gemv_w8_rows: alignment (16 bytes; ldx a multiple of 8, ldw of 16)");
  const int br = dec_bucket(B);      // the bucket the kernel stages
  VG_CHECK(!norm_w || (int64_t)br * K * 2 <= 160 * 1024 - 8 * 1024, VG_ERR_UNSUPPORTED,
           "vg_decode_gemv_w8_rows: the norm stages the whole rows of the %d-row bucket: B=%d K=%d do not fit", br, B, K);
  DecRowsW8Args p{x, ldx, W8, ldw, wscale, y, ldy, norm_w, eps, R, ldr, N, K, B, 1, 1};
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == VG_BF16) return glu ? launch_w8_rows<bf16_t, true>(p, st) : launch_w8_rows<bf16_t, false>(p, st);
  return glu ? launch_w8_rows<float, true>(p, st) : launch_w8_rows<float, false>(p, st);
}

// ---------------------------------------------------------------------------------------------------------------
// Attention of the one new token.  grid = (ceil(max_len/64) splits, Hkv): a workgroup owns 64 keys of one KV head and
// the G = H/Hkv query heads that share it.  All K and V bytes of the split are requested up front (one HBM round
// trip), RoPE of q and of the new k runs while they are in flight, the workgroup that owns position `pos` appends the
// new k/v rows to the cache, and the last workgroup of a KV head to finish merges the per-split (max, sum, acc)
// partials — ordering by an agent-scope arrival counter that resets itself, so the launch is graph-replayable.
// vg_decode_layer's flag region (ints; 32-int = 128-byte lines so that no two hot words share one): line 0 = [0] KV heads merged, [1] a wait gave up;
// lines 4 + 16 r + s = arrival stripe s of GEMV role r; lines 36 + r = the stripes of role r completed; lines 40 + 64 b + i = go flag i of boundary b
constexpr int DEC_LINE = 32, DEC_STRIPES = 16, DEC_GO = 64;
constexpr int DEC_CHAIN_INTS = (40 + 3 * DEC_GO) * DEC_LINE;
struct DecAttnArgs {
  const void* qkv; void* kc; void* vc; const float* cs; const float* sn; void* o;
  float* ws; int* cnt; const int* pos_dev;
  int H, Hkv, D, nsplit; float scale;
  int window;   // > 0: only the last `window` positions (the new one included) are attended (sliding-window LLMs); 0: all
};

__device__ __forceinline__ float ld_agent(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // global_load_dword sc1
}
__device__ __forceinline__ void st_agent(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        // global_store_dword sc1 (write-through)
}

template <typename TO> __device__ __forceinline__ float ld_agent_elt(const TO* p);
template <> __device__ __forceinline__ float ld_agent_elt<float>(const float* p) { return ld_agent(p); }
template <> __device__ __forceinline__ float ld_agent_elt<bf16_t>(const bf16_t* p) {
  return bf2f(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));       // global_load_ushort sc1
}
template <typename TO> __device__ __forceinline__ void st_agent_elt(TO* p, float v);
template <> __device__ __forceinline__ void st_agent_elt<float>(float* p, float v) { st_agent(p, v); }
template <> __device__ __forceinline__ void st_agent_elt<bf16_t>(bf16_t* p, float v) {
  __hip_atomic_store(p, f2bf(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // global_store_short sc1
}

// K/V storage of the attention body.  KV = T: the cache holds the activation dtype, a lane's chunk is 16 bytes.  KV = kv8_t (bf16 activations only):
// the cache holds OCP e4m3 codes, one byte per element and no scale, in the same [max_len, Hkv, D] layout; a chunk is still KPC = 8 elements, so
// 8 bytes, and every (wave, chunk, lane) assignment, fmaf chain and reduction below is the bf16 body's.  e4m3 -> fp32 is exact and every e4m3
// value is a bf16 value, so the body computes bit for bit what the bf16 body computes on the dequantised cache.
// (kv8_t, kv8_unpack8: vg_common.h; the quantiser kv8_pack4: above, beside the rope epilogues that append such rows)
template <typename KV> struct dec_kv { typedef u32x4_t reg_t; };
template <> struct dec_kv<kv8_t> { typedef u32x2_t reg_t; };
template <typename KV> __device__ __forceinline__ void dec_kv_unpack(const typename dec_kv<KV>::reg_t& v, float* f) { dec_unpack<KV>(v, f); }
template <> __device__ __forceinline__ void dec_kv_unpack<kv8_t>(const u32x2_t& v, float* f) { kv8_unpack8(v, f); }

// DT = compile-time head_dim (0 = run-time p.D): with it every load loop below has a constant trip count, so the
// kernel is straight-line up to the first wait and the compiler's vmcnt bookkeeping stays exact.
// AG (decode_layer_kernel): the merged output row leaves write-through (sc1) and *done is bumped once per KV head after it — the
// o_proj workgroups of the same launch wait on that counter and read the row with sc1 loads.
// LB = 64-key blocks per workgroup (2 at long caches: half as many partials to publish, arrive and merge — the merge then takes ONE pass of <= 32)
template <typename T, int G, int DT, bool AG, int LB = 1, typename KV = T>
__device__ __forceinline__ void dec_attn_body(const DecAttnArgs& p, const int s, const int kvh, char* dec_smem, int& ticket, int* done) {
  constexpr int KPC = 16 / sizeof(T);
  constexpr bool KV8 = std::is_same<KV, kv8_t>::value;
  static_assert(!KV8 || sizeof(T) == 2, "the e4m3 cache goes with bf16 activations");
  typedef typename dec_kv<KV>::reg_t kvreg_t;
  constexpr int L = 64 * LB;
  const int pos = *p.pos_dev;
  const int active = pos / L + 1;
  const int lo = p.window > 0 ? max(0, pos + 1 - p.window) : 0;     // first visible position
  const int first = lo / L;                                         // first split with a visible key
  if (s >= active || s < first) return;
  const int nact = active - first;
  const int D = DT ? DT : p.D;
  const int CH = D / KPC, hd = D / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = s * L;
  const int nk = min(L, pos + 1 - j0);
  const int KP = 256 / CH, cidx = tid % CH, kslot = min(tid / CH, KP - 1);
  const bool vlive = tid / CH < KP;
  const int NKI = DT ? (DT / KPC + 3) / 4 : 8;                 // K chunks per lane (wave w takes chunks w, w+4, ...)
  const int NVI = DT ? (64 + 256 / (DT / KPC) - 1) / (256 / (DT / KPC)) : 8;   // V rows per thread
  const int NRI = DT ? ((G + 1) * (DT / 2) + 255) / 256 : ((G + 1) * hd + 255) / 256;   // rope pairs per thread
  float* qs = (float*)dec_smem;       // [G][D] roped q
  float* knew = qs + G * D;           // [D] roped new k
  float* vnew = knew + D;             // [D]
  float* sp = vnew + D;               // [4 waves][G][64] partial scores
  float* sc = sp + LB * 4 * G * 64;   // [G][LB][64] exp(score - max)      (sp: [LB][4 waves][G][64])
  float* ms = sc + LB * G * 64;       // [G] max | [G] sum
  float* po = ms + 2 * G + ((4 - ((2 * G) & 3)) & 3);   // [KP][G][D] partial outputs

  // ---- 1. every global load up front, the early-needed (L2-resident) ones first: vmcnt retires in order
  const T* qkv = (const T*)p.qkv;
  const float* cs = p.cs + (int64_t)pos * hd;
  const float* sn = p.sn + (int64_t)pos * hd;
  float rx1[5], rx2[5], rc[5], rs_[5];
#pragma unroll
  for (int it = 0; it < 5; ++it) {
    if (it < NRI) {
      const int idx = min(tid + 256 * it, (G + 1) * hd - 1);
      const int gh = idx / hd, d = idx % hd;
      const T* src = gh < G ? qkv + (int64_t)(kvh * G + gh) * D : qkv + (int64_t)(p.H + kvh) * D;
      rx1[it] = vg_elt<T>::ld(src + d);
      rx2[it] = vg_elt<T>::ld(src + d + hd);
      rc[it] = cs[d];
      rs_[it] = sn[d];
    }
  }
  const float vn = vg_elt<T>::ld(qkv + (int64_t)(p.H + p.Hkv + kvh) * D + min(tid, D - 1));
  const int64_t rs = (int64_t)p.Hkv * D;
  const KV* kb = (const KV*)p.kc + ((int64_t)j0 * p.Hkv + kvh) * D;
  const KV* vb = (const KV*)p.vc + ((int64_t)j0 * p.Hkv + kvh) * D;
  kvreg_t kreg[LB][8], vreg[LB][8];
#pragma unroll
  for (int sub = 0; sub < LB; ++sub) {
    const int jl = min(sub * 64 + lane, nk - 1);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < NKI) kreg[sub][i] = *(const kvreg_t*)(kb + jl * rs + min(wave + 4 * i, CH - 1) * KPC);
  }
#pragma unroll
  for (int sub = 0; sub < LB; ++sub) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < NVI) vreg[sub][i] = *(const kvreg_t*)(vb + min(sub * 64 + kslot + KP * i, nk - 1) * rs + cidx * KPC);
  }
  // ---- 2. RoPE of the G query heads and of the new key; the new value row (vg_rope_kv_append arithmetic)
#pragma unroll
  for (int it = 0; it < 5; ++it) {
    if (it < NRI) {
      const int idx = tid + 256 * it;
      const int gh = idx / hd, d = idx % hd;
      const float x1 = rx1[it], x2 = rx2[it], c = rc[it], sv = rs_[it];
      float o1, o2;
      if (sizeof(T) == 2) {
        const float cb = bf2f(f2bf(c)), sb = bf2f(f2bf(sv));
        o1 = bf2f(f2bf(x1 * cb)) + bf2f(f2bf(-x2 * sb));
        o2 = bf2f(f2bf(x2 * cb)) + bf2f(f2bf(x1 * sb));
      } else {
        o1 = x1 * c - x2 * sv;
        o2 = x2 * c + x1 * sv;
      }
      o1 = dec_round<T>(o1);
      o2 = dec_round<T>(o2);
      if (idx < (G + 1) * hd) {
        float* dst = gh < G ? qs + gh * D : knew;
        dst[d] = o1;
        dst[d + hd] = o2;
      }
    }
  }
  if (tid < D) vnew[tid] = vn;
  __syncthreads();
  if (s == active - 1) {   // this split holds position `pos`: append the new rows to the cache
    KV* kdst = (KV*)p.kc + ((int64_t)pos * p.Hkv + kvh) * D;
    KV* vdst = (KV*)p.vc + ((int64_t)pos * p.Hkv + kvh) * D;
    if constexpr (KV8) {       // the appended row is the quantised form of the bf16 row; this step itself attends to knew / vnew unquantised (isnew below)
      if (tid < D / 4) {
        const int d = 4 * tid;
        *(uint32_t*)(kdst + d) = kv8_pack4(knew[d], knew[d + 1], knew[d + 2], knew[d + 3]);
        *(uint32_t*)(vdst + d) = kv8_pack4(vnew[d], vnew[d + 1], vnew[d + 2], vnew[d + 3]);
      }
    } else if (tid < D) {
      vg_elt<T>::st((T*)kdst + tid, knew[tid]);
      vg_elt<T>::st((T*)vdst + tid, vnew[tid]);
    }
  }
  // ---- 3. q.k: lane = key, wave w covers 16-byte chunks w, w+4, ... of the head dimension
#pragma unroll
  for (int sub = 0; sub < LB; ++sub) {
    const bool isnew = (j0 + sub * 64 + lane == pos);
    float part[G];
#pragma unroll
    for (int g = 0; g < G; ++g) part[g] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = wave + 4 * i;
      if (i < NKI && c < CH) {
        float kf[KPC];
        dec_kv_unpack<KV>(kreg[sub][i], kf);
        if (isnew) {
#pragma unroll
          for (int e = 0; e < KPC; ++e) kf[e] = knew[c * KPC + e];
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int e = 0; e < KPC; ++e) part[g] = fmaf(kf[e], qs[g * D + c * KPC + e], part[g]);
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) sp[((sub * 4 + wave) * G + g) * 64 + lane] = part[g];
  }
  __syncthreads();
  for (int g = wave; g < G; g += 4) {
    float v[LB];
    bool seen[LB];
    float mx = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < LB; ++sub) {
      const float* q4 = sp + (sub * 4 * G + g) * 64 + lane;
      v[sub] = (q4[0] + q4[G * 64] + q4[2 * G * 64] + q4[3 * G * 64]) * p.scale;
      seen[sub] = sub * 64 + lane < nk && j0 + sub * 64 + lane >= lo;
      if (!seen[sub]) v[sub] = -INFINITY;
      mx = fmaxf(mx, v[sub]);
    }
    const float m = wave_max(mx);
    float es = 0.f;
#pragma unroll
    for (int sub = 0; sub < LB; ++sub) {
      const float e = seen[sub] ? __expf(v[sub] - m) : 0.f;
      sc[(g * LB + sub) * 64 + lane] = e;
      es += e;
    }
    const float l = wave_sum(es);
    if (lane == 0) { ms[g] = m; ms[G + g] = l; }
  }
  __syncthreads();
  // ---- 4. p.v: thread = (key slot, 16-byte chunk of the head dimension)
  {
    float acc[G][KPC];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < KPC; ++e) acc[g][e] = 0.f;
#pragma unroll
    for (int sub = 0; sub < LB; ++sub)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = sub * 64 + kslot + KP * i;
      if (i < NVI && vlive && kslot + KP * i < 64 && j < nk) {      // (KP does not divide 64 at head dim 96: the last row round overshoots the block)
        float vf[KPC];
        dec_kv_unpack<KV>(vreg[sub][i], vf);
        if (j0 + j == pos) {
#pragma unroll
          for (int e = 0; e < KPC; ++e) vf[e] = vnew[cidx * KPC + e];
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float pj = sc[g * LB * 64 + j];
#pragma unroll
          for (int e = 0; e < KPC; ++e) acc[g][e] = fmaf(pj, vf[e], acc[g][e]);
        }
      }
    }
    if (vlive) {
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < KPC; ++e) po[(kslot * G + g) * D + cidx * KPC + e] = acc[g][e];
    }
  }
  __syncthreads();
  // ---- 5. publish the split's partials write-through (sc1): the merging workgroup reads them with sc1 loads, so the
  //         hand-off needs no cache write-back / invalidate fences (MI355X_MICROARCH.md, valid hand-off forms)
  float* wsp = p.ws + ((int64_t)kvh * p.nsplit + s) * G * (D + 2);
  for (int o = tid; o < G * D; o += 256) {
    const int g = o / D, d = o % D;
    float sum = 0.f;
    for (int k = 0; k < KP; ++k) sum += po[(k * G + g) * D + d];
    st_agent(wsp + g * (D + 2) + d, sum);
  }
  if (tid < G) { st_agent(wsp + tid * (D + 2) + D, ms[tid]); st_agent(wsp + tid * (D + 2) + D + 1, ms[G + tid]); }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) ticket = __hip_atomic_fetch_add(&p.cnt[kvh], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (ticket != nact - 1) return;
  // ---- 6. merge by the last workgroup of this KV head to arrive.  All loads of a pass (the (max, sum) of every
  //         split and two accumulator columns per thread) are requested together: one fabric round trip per pass.
  const float* wbase = p.ws + ((int64_t)kvh * p.nsplit + first) * G * (D + 2);   // the visible splits [first, active)
  float* cw = sp;                    // [nact][G] max -> weight      (sp is free again; nsplit*G*2 <= 4*G*64)
  float* cl = sp + p.nsplit * G;     // [nact][G] sum
  T* out = (T*)p.o;
  const int nml = nact * G;
  for (int o0 = 0; o0 < G * D; o0 += 512) {
    int oo[2], og[2], od[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      oo[k] = o0 + tid + 256 * k;
      const int oc = min(oo[k], G * D - 1);
      og[k] = oc / D;
      od[k] = oc % D;
    }
    float num[2] = {0.f, 0.f};
    for (int sb = 0; sb < nact; sb += 32) {
      float mv[2], lv[2];
      if (o0 == 0 && sb == 0) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {       // nml <= 128 * 8: two slots per thread cover 512, the rest loops below
          const float* w = wbase + (int64_t)min(tid + 256 * k, nml - 1) * (D + 2);
          mv[k] = ld_agent(w + D);
          lv[k] = ld_agent(w + D + 1);
        }
      }
      float v[2][32];
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int u = 0; u < 32; ++u)
          v[k][u] = ld_agent(wbase + ((int64_t)min(sb + u, nact - 1) * G + og[k]) * (D + 2) + od[k]);
      if (o0 == 0 && sb == 0) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (tid + 256 * k < nml) { cw[tid + 256 * k] = mv[k]; cl[tid + 256 * k] = lv[k]; }
        for (int t = tid + 512; t < nml; t += 256) {
          const float* w = wbase + (int64_t)t * (D + 2);
          cw[t] = ld_agent(w + D);
          cl[t] = ld_agent(w + D + 1);
        }
        __syncthreads();
        for (int gg = wave; gg < G; gg += 4) {
          float M = -INFINITY;
          for (int s2 = lane; s2 < nact; s2 += 64) M = fmaxf(M, cw[s2 * G + gg]);
          M = wave_max(M);
          float den = 0.f;
          for (int s2 = lane; s2 < nact; s2 += 64) {
            const float wgt = __expf(cw[s2 * G + gg] - M);
            cw[s2 * G + gg] = wgt;
            den = fmaf(wgt, cl[s2 * G + gg], den);
          }
          den = wave_sum(den);
          if (lane == 0) ms[gg] = 1.0f / den;
        }
        __syncthreads();
      }
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int u = 0; u < 32; ++u)
          if (sb + u < nact) num[k] = fmaf(cw[(sb + u) * G + og[k]], v[k][u], num[k]);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (oo[k] < G * D) {
        if constexpr (AG) st_agent_elt<T>(out + (int64_t)(kvh * G + og[k]) * D + od[k], num[k] * ms[og[k]]);
        else vg_elt<T>::st(out + (int64_t)(kvh * G + og[k]) * D + od[k], num[k] * ms[og[k]]);
      }
  }
  if (tid == 0) __hip_atomic_store(&p.cnt[kvh], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if constexpr (AG) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) ticket = __hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (ticket == p.Hkv - 1 && tid < DEC_GO)        // every head's row is in memory: release the o_proj workgroups (64 flags, 8 pollers each)
      __hip_atomic_store(done + (40 + tid) * DEC_LINE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <typename T, int G, int DT, int LB = 1, typename KV = T>
__global__ __launch_bounds__(256) void decode_attn_kernel(DecAttnArgs p) {
  extern __shared__ __attribute__((aligned(16))) char dec_smem[];
  __shared__ int ticket;
  dec_attn_body<T, G, DT, false, LB, KV>(p, blockIdx.x, blockIdx.y, dec_smem, ticket, nullptr);
}

template <typename T, int G, int DT, int LB = 1, typename KV = T>
static void launch_decode_attn_gd(const DecAttnArgs& p, dim3 grid, size_t lds, hipStream_t st) {
  vg_raise_lds_cap<decode_attn_kernel<T, G, DT, LB, KV>>(lds);
  decode_attn_kernel<T, G, DT, LB, KV><<<grid, 256, lds, st>>>(p);
}

template <typename T, int G, typename KV = T>
static void launch_decode_attn_g(const DecAttnArgs& p, dim3 grid, size_t lds, hipStream_t st) {
  if (p.D == 128) launch_decode_attn_gd<T, G, 128, 1, KV>(p, grid, lds, st);
  else if (p.D == 96) launch_decode_attn_gd<T, G, 96, 1, KV>(p, grid, lds, st);      // Phi-3-mini: the released checkpoint's LLM
  else launch_decode_attn_gd<T, G, 0, 1, KV>(p, grid, lds, st);
}

template <typename T, typename KV = T>
static int launch_decode_attn(const DecAttnArgs& p, int G, int keys_per_wg, hipStream_t st) {
  constexpr int KPC = 16 / sizeof(T);
  const int KP = 256 / (p.D / KPC);
  size_t lds = sizeof(float) * ((size_t)G * p.D + 2 * p.D + 4 * G * 64 + G * 64 + 2 * G + 4 + (size_t)KP * G * p.D);
  dim3 grid(p.nsplit, p.Hkv);
  if constexpr (sizeof(T) == 2) {
    // 128 keys per workgroup (the caller's hint for long caches): the two shapes the pipeline decodes with — Llama-3 (G = 4, d = 128), Phi-3 (MHA, d = 96)
    if (keys_per_wg == 128 && ((G == 4 && p.D == 128) || (G == 1 && p.D == 96))) {
      lds += sizeof(float) * (4 * G * 64 + G * 64);
      if (G == 4) launch_decode_attn_gd<T, 4, 128, 2, KV>(p, grid, lds, st);
      else launch_decode_attn_gd<T, 1, 96, 2, KV>(p, grid, lds, st);
      VG_LAUNCH_CHECK();
      return VG_OK;
    }
  }
  switch (G) {
    case 1: launch_decode_attn_g<T, 1, KV>(p, grid, lds, st); break;
    case 2: launch_decode_attn_g<T, 2, KV>(p, grid, lds, st); break;
    case 4: launch_decode_attn_g<T, 4, KV>(p, grid, lds, st); break;
    case 8: launch_decode_attn_g<T, 8, KV>(p, grid, lds, st); break;
    default:
      vg_set_error("vg_decode_attention: H/Hkv = %d not in {1,2,4,8}", G);
      return VG_ERR_UNSUPPORTED;
  }
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int64_t vg_decode_attention_ws_floats(int H, int Hkv, int D, int max_len) {
  if (H <= 0 || Hkv <= 0 || D <= 0 || max_len <= 0 || H % Hkv) return -1;
  const int64_t nsplit = (max_len + 63) / 64;
  return (int64_t)Hkv * nsplit * (H / Hkv) * (D + 2) + Hkv;
}

// vg_decode_attention on e4m3 caches (kv8_t above): bf16 qkv / out, the same workspace, the same shapes
extern "C" int vg_decode_attention_kv8_supported(int H, int Hkv, int D, int dtype) {
  if (dtype != VG_BF16 || H <= 0 || Hkv <= 0 || H % Hkv || D <= 0 || D % 8 || D > 256) return 0;
  const int G = H / Hkv;
  return G == 1 || G == 2 || G == 4 || G == 8;
}

// fn: the entry point's name for the messages.  KV: the caches' element type — void = the activation dtype, kv8_t = e4m3 codes.  The caches'
// alignment is one chunk of that type (16 bytes, 8 bytes of e4m3 codes); what each entry point covers is checked in its own words
template <typename KV>
static int decode_attention(const char* fn, const void* qkv, void* k_cache, void* v_cache, const float* cos, const float* sin, void* out, int H, int Hkv,
                            int D, int max_len, int window, float scale, const int* pos_dev, float* workspace, int64_t ws_floats, int keys_per_wg,
                            int dtype, vg_stream_t stream) {
  constexpr bool KV8 = std::is_same<KV, kv8_t>::value;
  constexpr int KVA = KV8 ? 8 : 16;
  VG_CHECK(qkv && k_cache && v_cache && cos && sin && out && pos_dev && workspace, VG_ERR_ARG, "%s: null pointer", fn);
  VG_CHECK(keys_per_wg == 0 || keys_per_wg == 64 || keys_per_wg == 128, VG_ERR_ARG, "%s: keys_per_wg %d not in {0, 64, 128}", fn, keys_per_wg);
  if constexpr (KV8) {
    VG_CHECK(max_len > 0 && window >= 0, VG_ERR_ARG, "%s: bad max_len %d / window %d", fn, max_len, window);
    VG_CHECK(vg_decode_attention_kv8_supported(H, Hkv, D, dtype), VG_ERR_UNSUPPORTED,
             "%s: H=%d Hkv=%d D=%d dtype=%d not covered (bf16, H/Hkv in {1,2,4,8}, head_dim a multiple of 8, <= 256)", fn, H, Hkv, D, dtype);
  } else {
    VG_CHECK(H > 0 && Hkv > 0 && H % Hkv == 0 && D > 0 && D % 2 == 0 && max_len > 0, VG_ERR_ARG, "%s: bad shape H=%d Hkv=%d D=%d max_len=%d", fn, H, Hkv,
             D, max_len);
    VG_CHECK(dtype == VG_BF16 || dtype == VG_F32, VG_ERR_ARG, "%s: bad dtype %d", fn, dtype);
    VG_CHECK(window >= 0, VG_ERR_ARG, "%s: window %d < 0", fn, window);
    const int kpc = dtype == VG_BF16 ? 8 : 4, es = dtype == VG_BF16 ? 2 : 4;
    VG_CHECK(D % kpc == 0 && D * es <= 512, VG_ERR_UNSUPPORTED, "%s: head_dim %d unsupported (multiple of %d, <= %d)", fn, D, kpc, 512 / es);
  }
  VG_CHECK((((uintptr_t)k_cache | (uintptr_t)v_cache) & (KVA - 1)) == 0, VG_ERR_ARG, "%s: caches must be %d-byte aligned", fn, KVA);
  const int64_t need = vg_decode_attention_ws_floats(H, Hkv, D, max_len);
  VG_CHECK(ws_floats >= need, VG_ERR_ARG, "%s: workspace %lld < %lld floats", fn, (long long)ws_floats, (long long)need);
  const int nsplit = (max_len + 63) / 64;
  VG_CHECK(nsplit <= 128, VG_ERR_UNSUPPORTED, "%s: max_len %d > 8192", fn, max_len);
  DecAttnArgs p{qkv, k_cache, v_cache, cos, sin, out, workspace, (int*)(workspace + (need - Hkv)), pos_dev, H, Hkv, D, nsplit, scale, window};
  if constexpr (KV8) {
    return launch_decode_attn<bf16_t, kv8_t>(p, H / Hkv, keys_per_wg, (hipStream_t)stream);
  } else {
    if (dtype == VG_BF16) return launch_decode_attn<bf16_t>(p, H / Hkv, keys_per_wg, (hipStream_t)stream);
    return launch_decode_attn<float>(p, H / Hkv, keys_per_wg, (hipStream_t)stream);
  }
}

extern "C" int vg_decode_attention(const void* qkv, void* k_cache, void* v_cache, const float* cos, const float* sin,
                                   void* out, int H, int Hkv, int D, int max_len, int window, float scale, const int* pos_dev,
                                   float* workspace, int64_t ws_floats, int keys_per_wg, int dtype, vg_stream_t stream) {
  return decode_attention<void>("vg_decode_attention", qkv, k_cache, v_cache, cos, sin, out, H, Hkv, D, max_len, window, scale, pos_dev, workspace,
                                ws_floats, keys_per_wg, dtype, stream);
}

extern "C" int vg_decode_attention_kv8(const void* qkv, void* k_cache, void* v_cache, const float* cos, const float* sin, void* out, int H, int Hkv,
                                       int D, int max_len, int window, float scale, const int* pos_dev, float* workspace, int64_t ws_floats,
                                       int keys_per_wg, int dtype, vg_stream_t stream) {
  return decode_attention<kv8_t>("vg_decode_attention_kv8", qkv, k_cache, v_cache, cos, sin, out, H, Hkv, D, max_len, window, scale, pos_dev, workspace,
                                 ws_floats, keys_per_wg, dtype, stream);
}

// dst[i] = e4m3(src[i]) (kv8_pack4: clamp, round to nearest even, no scale) for n elements: a prefill's bf16 K / V rows -> the e4m3 cache
__global__ __launch_bounds__(256) void kv_quantize_fp8_kernel(const bf16_t* src, uint8_t* dst, int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 4 <= n) {
    const uint32_t a = *(const uint32_t*)(src + i), b = *(const uint32_t*)(src + i + 2);
    *(uint32_t*)(dst + i) = kv8_pack4(__uint_as_float(a << 16), __uint_as_float(a & 0xffff0000u), __uint_as_float(b << 16),
                                      __uint_as_float(b & 0xffff0000u));
  } else {
    for (int64_t k = i; k < n; ++k) dst[k] = (uint8_t)(kv8_pack4(bf2f(src[k]), 0.f, 0.f, 0.f) & 0xffu);
  }
}

extern "C" int vg_kv_quantize_fp8(const void* src, uint8_t* dst, int64_t n, vg_stream_t stream) {
  VG_CHECK(src && dst && n > 0, VG_ERR_ARG, "vg_kv_quantize_fp8: bad args n=%lld", (long long)n);
  VG_CHECK((((uintptr_t)src | (uintptr_t)dst) & 3) == 0, VG_ERR_ARG, "vg_kv_quantize_fp8: src and dst must be 4-byte aligned");
  const int64_t nb = (n + 1023) / 1024;
  VG_CHECK(nb <= 0x7fffffff, VG_ERR_UNSUPPORTED, "vg_kv_quantize_fp8: n %lld too large", (long long)n);
  kv_quantize_fp8_kernel<<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>((const bf16_t*)src, dst, n);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// B query rows of vg_decode_attention at once (the batched multi-prompt decode step of the decode_attention path): grid z = row.
// Row b is decode_attn_kernel on row b alone — its q|k|v row (qkv + b * ldqkv), RoPE at pos[b] from the shared cos / sin tables, the append of
// its new key / value row, its own partials, arrival counters and output row — so it is bit-identical to vg_decode_attention on that row with the
// whole cache in one array.  Key blocks below row0 come from the shared caches (the prefix); blocks from row0 on are slot b's (ks / vs +
// b * slot_stride, sequence row j at j - row0), and the new rows are appended there.  row0 is a multiple of 128, so every 64- or 128-key split is
// wholly shared or wholly per slot.  Keys per workgroup: 128 (LB = 2) when pos[b] >= kpw_min, else 64 — the single-row step's choice, made per
// row on the device, so rows on both sides of the threshold share one launch and one captured graph.  A row whose position lies outside
// [row0, n_bound) does nothing (no append, no counter touched; RowsDecode refuses such a step on the host).
struct DecAttnRowsArgs {
  void* ks; void* vs; int64_t slot_stride, ldqkv, ws_row; const int* pos; int row0, n_bound, kpw_min;
};

template <int G, int DT, typename KV = bf16_t>
__global__ __launch_bounds__(256) void decode_attn_rows_kernel(DecAttnArgs p, DecAttnRowsArgs r) {
  extern __shared__ __attribute__((aligned(16))) char dec_smem[];
  __shared__ int ticket;
  const int b = blockIdx.z, s = blockIdx.x, kvh = blockIdx.y;
  const int pos = r.pos[b];
  if (pos < r.row0 || pos >= r.n_bound) return;
  const bool wide = pos >= r.kpw_min;              // uniform across the workgroup
  DecAttnArgs q = p;
  q.qkv = (const bf16_t*)p.qkv + b * r.ldqkv;
  q.o = (bf16_t*)p.o + (int64_t)b * p.H * DT;
  q.ws = p.ws + b * r.ws_row;
  q.cnt = p.cnt + b * p.Hkv;
  q.pos_dev = r.pos + b;
  if (s * (wide ? 128 : 64) >= r.row0) {           // a per-slot split: the body's row j lands on slot row j - row0 (j >= row0 only)
    const int64_t off = b * r.slot_stride - (int64_t)r.row0 * p.Hkv * DT;
    q.kc = (KV*)r.ks + off;
    q.vc = (KV*)r.vs + off;
  }
  if (wide) dec_attn_body<bf16_t, G, DT, false, 2, KV>(q, s, kvh, dec_smem, ticket, nullptr);
  else dec_attn_body<bf16_t, G, DT, false, 1, KV>(q, s, kvh, dec_smem, ticket, nullptr);
}

extern "C" int vg_decode_attention_rows_supported(int H, int Hkv, int D, int dtype) {
  return dtype == VG_BF16 && H > 0 && H == Hkv && D == 96;       // Phi-3-mini: MHA, head_dim 96
}

extern "C" int vg_decode_step_rows_supported(int H, int Hkv, int D, int hidden, int inter, int dtype) {
  // the decode_attention step's layer on the B-row kernels: the attention above, the q|k|v / o / gate|up GEMVs at K = hidden (the norm stages the
  // 16-row bucket's whole rows) and down at K = inter
  return vg_decode_attention_rows_supported(H, Hkv, D, dtype) && H * D == hidden && dec_rows_nb(hidden) && dec_rows_nb(inter) &&
         16 * hidden * 2 <= 160 * 1024 - 8 * 1024;
}

extern "C" int64_t vg_decode_attention_rows_ws_floats(int H, int Hkv, int D, int n_bound, int B) {
  if (H <= 0 || Hkv <= 0 || D <= 0 || n_bound <= 0 || B <= 0 || H % Hkv) return -1;
  const int64_t nsplit = (n_bound + 63) / 64;
  return (int64_t)B * Hkv * nsplit * (H / Hkv) * (D + 2) + (int64_t)B * Hkv;
}

// kv8: the shared caches and the slots hold e4m3 codes (vg_decode_attention_rows_kv8; slot_stride in elements = bytes)
static int decode_attention_rows_impl(const void* qkv, int64_t ldqkv, const void* k_cache, const void* v_cache, int max_len, void* k_slots,
                                      void* v_slots, int64_t slot_stride, int row0, int slot_rows, const float* cos, const float* sin, void* out,
                                      int H, int Hkv, int D, int n_bound, int window, float scale, const int* pos, int kpw_min, float* workspace,
                                      int64_t ws_floats, int B, int dtype, bool kv8, vg_stream_t stream) {
  VG_CHECK(qkv && k_cache && v_cache && k_slots && v_slots && cos && sin && out && pos && workspace && dec_rows_b_ok(B), VG_ERR_ARG,
           "vg_decode_attention_rows: bad args B=%d", B);
  VG_CHECK(vg_decode_attention_rows_supported(H, Hkv, D, dtype), VG_ERR_UNSUPPORTED, "vg_decode_attention_rows: H=%d Hkv=%d D=%d dtype=%d not covered",
           H, Hkv, D, dtype);
  VG_CHECK(row0 >= 0 && row0 % 128 == 0 && slot_rows > 0 && n_bound > row0 && n_bound <= row0 + slot_rows && n_bound <= max_len && window >= 0 &&
               ldqkv >= (int64_t)(H + 2 * Hkv) * D, VG_ERR_ARG,
           "vg_decode_attention_rows: row0=%d (a multiple of 128), slot_rows=%d, n_bound=%d in (row0, min(row0 + slot_rows, max_len %d)]", row0,
           slot_rows, n_bound, max_len);
  VG_CHECK((((uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)k_slots | (uintptr_t)v_slots) & 15) == 0 && slot_stride % 8 == 0 &&
               slot_stride >= (int64_t)slot_rows * Hkv * D, VG_ERR_ARG, "vg_decode_attention_rows: 16-byte alignment; slots must not overlap");
  const int64_t need = vg_decode_attention_rows_ws_floats(H, Hkv, D, n_bound, B);
  VG_CHECK(ws_floats >= need, VG_ERR_ARG, "vg_decode_attention_rows: workspace %lld < %lld floats", (long long)ws_floats, (long long)need);
  const int nsplit = (n_bound + 63) / 64;
  VG_CHECK(nsplit <= 128, VG_ERR_UNSUPPORTED, "vg_decode_attention_rows: n_bound %d > 8192", n_bound);
  const int G = H / Hkv;
  const int64_t ws_row = (int64_t)Hkv * nsplit * G * (D + 2);
  DecAttnArgs p{qkv, (void*)k_cache, (void*)v_cache, cos, sin, out, workspace, (int*)(workspace + (ws_floats - (int64_t)B * Hkv)), pos, H, Hkv, D,
                nsplit, scale, window};
  DecAttnRowsArgs r{k_slots, v_slots, slot_stride, ldqkv, ws_row, pos, row0, n_bound, kpw_min};
  // the LB = 2 layout (launch_decode_attn's, plus the second block's scores): LB = 1 rows use a prefix of it
  const int KP = 256 / (D / 8);
  const size_t lds = sizeof(float) * ((size_t)G * D + 2 * D + 4 * G * 64 + G * 64 + 2 * G + 4 + (size_t)KP * G * D + 4 * G * 64 + G * 64);
  if (kv8) decode_attn_rows_kernel<1, 96, kv8_t><<<dim3(nsplit, Hkv, B), 256, lds, (hipStream_t)stream>>>(p, r);
  else decode_attn_rows_kernel<1, 96><<<dim3(nsplit, Hkv, B), 256, lds, (hipStream_t)stream>>>(p, r);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_decode_attention_rows(const void* qkv, int64_t ldqkv, const void* k_cache, const void* v_cache, int max_len, void* k_slots,
                                        void* v_slots, int64_t slot_stride, int row0, int slot_rows, const float* cos, const float* sin, void* out,
                                        int H, int Hkv, int D, int n_bound, int window, float scale, const int* pos, int kpw_min, float* workspace,
                                        int64_t ws_floats, int B, int dtype, vg_stream_t stream) {
  return decode_attention_rows_impl(qkv, ldqkv, k_cache, v_cache, max_len, k_slots, v_slots, slot_stride, row0, slot_rows, cos, sin, out, H, Hkv, D,
                                    n_bound, window, scale, pos, kpw_min, workspace, ws_floats, B, dtype, false, stream);
}

extern "C" int vg_decode_attention_rows_kv8_supported(int H, int Hkv, int D, int dtype) {
  return vg_decode_attention_rows_supported(H, Hkv, D, dtype);
}

extern "C" int vg_decode_attention_rows_kv8(const void* qkv, int64_t ldqkv, const void* k_cache, const void* v_cache, int max_len, void* k_slots,
                                            void* v_slots, int64_t slot_stride, int row0, int slot_rows, const float* cos, const float* sin,
                                            void* out, int H, int Hkv, int D, int n_bound, int window, float scale, const int* pos, int kpw_min,
                                            float* workspace, int64_t ws_floats, int B, int dtype, vg_stream_t stream) {
  return decode_attention_rows_impl(qkv, ldqkv, k_cache, v_cache, max_len, k_slots, v_slots, slot_stride, row0, slot_rows, cos, sin, out, H, Hkv, D,
                                    n_bound, window, scale, pos, kpw_min, workspace, ws_floats, B, dtype, true, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// One launch per decoder layer behind the q|k|v projection (r03): attention, o_proj (+ residual), and — bf16 Llama
// widths — RMSNorm + gate|up + SwiGLU and down_proj (+ residual) as ROLES of one grid.  A workgroup's role follows
// from its index, roles are laid out in dependency order, and the dispatcher hands out workgroups in index order, so
// every workgroup a waiting one depends on is already running: a GEMV workgroup requests its first two batches of
// weight rows (16 x 16 bytes per lane — all of its rows for o_proj / down_proj), THEN waits for the producer role,
// then reads the input row with sc1 loads.  What the separate launches serialised — the weight stream's ramp behind
// the latency-bound attention, and each GEMV's ramp behind the previous one's tail — now overlaps.  Arithmetic
// (order of every sum) is the separate kernels': results are bit-identical.
// Hand-off: a producer workgroup stores sc1 (write-through) -> s_waitcnt vmcnt(0) -> barrier -> relaxed agent-scope
// add on one of 16 arrival stripes (own 128-byte lines: 512 simultaneous arrivals on ONE word serialise at the
// memory side); who completes a stripe adds to the role's counter, who completes that raises 64 go flags (own lines);
// a consumer workgroup polls go flag (index % 64) with one lane, s_sleep between polls (first version: every waiting
// workgroup polled the word next to the attention tickets — the pollers starved the tickets, +17 us per layer), then
// barrier -> sc1 loads (MI355X_MICROARCH.md, valid hand-off forms: the one the split merge above uses).  The wait is
// bounded: after ~0.5 s a workgroup sets the gave-up word and carries on (wrong numbers the host reports, not a hung
// queue).  The caller zero-fills the flag region before every launch (one memset per token for all layers).
struct DecRoleArgs {
  DecGemvArgs g;
  int nblocks;
};
struct DecLayerArgs {
  DecAttnArgs a;
  DecRoleArgs r[3];     // o_proj, gate|up, down
  int nroles;           // 1: attention + o_proj; 3: + the MLP
  int* flags;
};

__device__ __forceinline__ void dec_chain_wait(int* flags, const int boundary, const int wg) {
  if (threadIdx.x == 0) {
    const int* go = flags + (40 + boundary * DEC_GO + (wg & (DEC_GO - 1))) * DEC_LINE;
    int spins = 0;
    while (__hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
      __builtin_amdgcn_s_sleep(16);
      if (++spins > (1 << 20)) {
        __hip_atomic_store(flags + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
  }
  __syncthreads();
  asm volatile("" ::: "memory");
}

// thread 0 of a finished workgroup of role r (n workgroups): true for the one arrival that completes the role
__device__ __forceinline__ bool dec_chain_arrive(int* flags, const int r, const int wg, const int n) {
  const int st = wg & (DEC_STRIPES - 1);
  const int in_stripe = (n - st + DEC_STRIPES - 1) / DEC_STRIPES;
  if (__hip_atomic_fetch_add(flags + (4 + DEC_STRIPES * r + st) * DEC_LINE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != in_stripe - 1) return false;
  const int nst = min(n, DEC_STRIPES);
  return __hip_atomic_fetch_add(flags + (36 + r) * DEC_LINE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nst - 1;
}

// dec_gemv_store for a role: the residual row was written by another role of this launch (sc1 loads: this XCD's L2 may hold the line from an earlier
// launch); AGST: somebody in this launch reads y (sc1 stores)
template <typename T, typename TO, bool GLU, bool AGST>
__device__ __forceinline__ void dec_gemv_store_ag(const DecGemvArgs& p, int pi, float a0, float a1) {
  const int n0 = GLU ? pi : 2 * pi, n1 = GLU ? p.N + pi : 2 * pi + 1;
  TO* y = (TO*)p.y;
  const TO* R = (const TO*)p.R;
  auto put = [&](int n, float v) {
    if (R) v += ld_agent_elt<TO>(R + n);
    if constexpr (AGST) st_agent_elt<TO>(y + n, v);
    else vg_elt<TO>::st(y + n, v);
  };
  if constexpr (GLU) {
    float g = a0, u = a1;
    if (sizeof(T) == 2) { g = bf2f(f2bf(g)); u = bf2f(f2bf(u)); }
    g = vg_silu(g);
    if (sizeof(T) == 2) g = bf2f(f2bf(g));
    put(n0, g * u);
  } else {
    put(n0, a0);
    if (n1 < p.N) put(n1, a1);
  }
}

// decode_gemv_fast_kernel's body as role `role` (0..2): weights first, wait on boundary `role`, x by sc1 loads; `release`: raise boundary role + 1
template <typename T, typename TO, bool GLU, bool NORM, int NB, int CPB>
__device__ __forceinline__ void dec_gemv_role(const DecGemvArgs& p, const int wg, const int nwg, char* dec_smem, float* red, float (*res)[DEC_MAX_PPW][2],
                                               int* flags, const int role, const bool release, int& bcast) {
  constexpr int KPC = 16 / sizeof(T);
  constexpr int NWV = KPC / 4;
  constexpr int NCH = NB * CPB * 64;
  constexpr int XN = (NCH + 255) / 256;
  typedef float f32x4_t __attribute__((ext_vector_type(4)));
  u32x4_t* xs = (u32x4_t*)dec_smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int npair = GLU ? p.N : (p.N + 1) / 2;
  const int gw = wg * 4 + wave;
  const T* W = (const T*)p.W;
  const int p0 = gw * p.ppw;
  const int np = max(min(p0 + p.ppw, npair) - p0, 0);
  const int total = np * NB;

  // ---- 1. the weights (and the norm weights: constants of the layer) before the input row exists
  int ipi = p0, icb = 0;
  u32x4_t va0[CPB], va1[CPB], vb0[CPB], vb1[CPB];
  auto issue = [&](u32x4_t (&v0)[CPB], u32x4_t (&v1)[CPB]) {
    const int pc = min(ipi, npair - 1);
    const int n0 = GLU ? pc : 2 * pc;
    const int n1 = GLU ? p.N + pc : min(2 * pc + 1, p.N - 1);
    const u32x4_t* w0 = (const u32x4_t*)(W + (int64_t)n0 * p.ldw) + icb * (64 * CPB) + lane;
    const u32x4_t* w1 = (const u32x4_t*)(W + (int64_t)n1 * p.ldw) + icb * (64 * CPB) + lane;
#pragma unroll
    for (int u = 0; u < CPB; ++u) {
      v0[u] = __builtin_nontemporal_load(w0 + u * 64);
      v1[u] = __builtin_nontemporal_load(w1 + u * 64);
    }
    if (++icb == NB) { icb = 0; ++ipi; }
  };
  issue(va0, va1);
  issue(vb0, vb1);
  f32x4_t nwr[NORM ? XN : 1][NWV];
  if constexpr (NORM) {
#pragma unroll
    for (int i = 0; i < XN; ++i)
#pragma unroll
      for (int j = 0; j < NWV; ++j) nwr[i][j] = ((const f32x4_t*)p.nw)[min(tid + 256 * i, NCH - 1) * NWV + j];
  }

  // ---- 2. the producer role's row
  dec_chain_wait(flags, role, wg);
  u32x4_t xr[XN];
#pragma unroll
  for (int i = 0; i < XN; ++i) {
    const uint32_t* src = (const uint32_t*)p.x + (int64_t)min(tid + 256 * i, NCH - 1) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) xr[i][j] = __hip_atomic_load(src + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  {
    float rstd = 1.f;
    if constexpr (NORM) {
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < XN; ++i) {
        float f[KPC];
        dec_unpack<T>(xr[i], f);
        if (tid + 256 * i < NCH) {
#pragma unroll
          for (int e = 0; e < KPC; ++e) ss += f[e] * f[e];
        }
      }
      ss = wave_sum(ss);
      if (lane == 0) red[wave] = ss;
      __syncthreads();
      rstd = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)p.K + p.eps);
#pragma unroll
      for (int i = 0; i < XN; ++i) {
        float f[KPC];
        dec_unpack<T>(xr[i], f);
#pragma unroll
        for (int e = 0; e < KPC; ++e) f[e] = dec_round<T>(f[e] * rstd) * nwr[i][e / 4][e % 4];
        xr[i] = dec_pack<T>(f);
      }
    }
#pragma unroll
    for (int i = 0; i < XN; ++i)
      if (tid + 256 * i < NCH) xs[tid + 256 * i] = xr[i];
    __syncthreads();
  }

  // ---- 3. the stream (decode_gemv_fast_kernel's)
  float a0 = 0.f, a1 = 0.f;
  int cpl = 0, ccb = 0;
  auto consume = [&](const u32x4_t (&v0)[CPB], const u32x4_t (&v1)[CPB]) {
#pragma unroll
    for (int u = 0; u < CPB; ++u) {
      const u32x4_t xv = xs[ccb * (64 * CPB) + u * 64 + lane];
      a0 += dec_dot<T>(v0[u], xv);
      a1 += dec_dot<T>(v1[u], xv);
    }
    if (++ccb == NB) {
      a0 = wave_sum(a0);
      a1 = wave_sum(a1);
      if (lane == 0) { res[wave][cpl][0] = a0; res[wave][cpl][1] = a1; }
      a0 = 0.f;
      a1 = 0.f;
      ccb = 0;
      ++cpl;
    }
  };
  int b = 0;
  for (; b + 4 <= total; b += 2) {
    consume(va0, va1);
    issue(va0, va1);
    consume(vb0, vb1);
    issue(vb0, vb1);
  }
  const int rem = total - b;
  if (rem == 3) {
    consume(va0, va1);
    issue(va0, va1);
    consume(vb0, vb1);
    consume(va0, va1);
  } else if (rem == 2) {
    consume(va0, va1);
    consume(vb0, vb1);
  } else if (rem == 1) {
    consume(va0, va1);
  }
  // ---- 4. epilogue; a role somebody waits for leaves write-through and arrives
  if (!release) {
    for (int i = lane; i < np; i += 64) dec_gemv_store_ag<T, TO, GLU, false>(p, p0 + i, res[wave][i][0], res[wave][i][1]);
    return;
  }
  for (int i = lane; i < np; i += 64) dec_gemv_store_ag<T, TO, GLU, true>(p, p0 + i, res[wave][i][0], res[wave][i][1]);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) bcast = dec_chain_arrive(flags, role, wg, nwg) ? 1 : 0;
  __syncthreads();
  if (bcast && tid < DEC_GO) __hip_atomic_store(flags + (40 + (role + 1) * DEC_GO + tid) * DEC_LINE, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// NBH / CPBH: batches x chunks of a hidden-size row (o_proj, gate|up); NBI: batches of an intermediate-size row (down_proj), 0 = no MLP roles
template <typename T, int G, int DT, int NBH, int CPBH, int NBI>
__global__ __launch_bounds__(256, 2) void decode_layer_kernel(DecLayerArgs q) {
  extern __shared__ __attribute__((aligned(16))) char dec_smem[];
  __shared__ int ticket;
  __shared__ float red[4];
  __shared__ float res[4][DEC_MAX_PPW][2];
  int w = blockIdx.x;
  const int nattn = q.a.nsplit * q.a.Hkv;
  if (w < nattn) {
    dec_attn_body<T, G, DT, true>(q.a, w % q.a.nsplit, w / q.a.nsplit, dec_smem, ticket, q.flags);
    return;
  }
  w -= nattn;
  if (w < q.r[0].nblocks) {
    dec_gemv_role<T, T, false, false, NBH, CPBH>(q.r[0].g, w, q.r[0].nblocks, dec_smem, red, res, q.flags, 0, q.nroles > 1, ticket);
    return;
  }
  if constexpr (NBI > 0) {
    w -= q.r[0].nblocks;
    if (w < q.r[1].nblocks) {
      dec_gemv_role<T, T, true, true, NBH, CPBH>(q.r[1].g, w, q.r[1].nblocks, dec_smem, red, res, q.flags, 1, true, ticket);
      return;
    }
    w -= q.r[1].nblocks;
    dec_gemv_role<T, T, false, false, NBI, 4>(q.r[2].g, w, q.r[2].nblocks, dec_smem, red, res, q.flags, 2, false, ticket);
  }
}

// 0: not available for this shape; 1: attention + o_proj; 3: + the MLP roles
extern "C" int vg_decode_layer_roles(int H, int Hkv, int D, int hidden, int inter, int dtype) {
  if (H <= 0 || Hkv <= 0 || H % Hkv || (int64_t)H * D != hidden) return 0;
  if (dtype == VG_BF16 && H / Hkv == 4 && D == 128 && hidden == 4096) return inter == 14336 ? 3 : 1;   // Llama-3-8B widths
  if (dtype == VG_F32 && H / Hkv == 4 && D == 128 && hidden == 4096) return 1;                          // fp32 mode of the same
  if (dtype == VG_BF16 && H == Hkv && D == 96 && hidden == 3072) return 1;                              // Phi-3-mini
  return 0;
}
extern "C" int64_t vg_decode_layer_flag_ints(void) { return DEC_CHAIN_INTS; }

template <typename T, int G, int DT, int NBH, int CPBH, int NBI>
static int launch_decode_layer(const DecLayerArgs& q, int blocks, size_t lds, hipStream_t st) {
  vg_raise_lds_cap<decode_layer_kernel<T, G, DT, NBH, CPBH, NBI>>(lds);
  decode_layer_kernel<T, G, DT, NBH, CPBH, NBI><<<blocks, 256, lds, st>>>(q);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_decode_layer(const void* qkv, void* k_cache, void* v_cache, const float* cos, const float* sin, void* attn_out,
                               int H, int Hkv, int D, int max_len, int window, float scale, const int* pos_dev,
                               float* workspace, int64_t ws_floats, int32_t* flags,
                               const void* Wo, int64_t ldo, const void* resid, void* y_o,
                               const float* norm_w, float eps, const void* Wgu, int64_t ldgu, void* act,
                               const void* Wdown, int64_t lddown, void* y, int hidden, int inter, int dtype, vg_stream_t stream) {
  VG_CHECK(qkv && k_cache && v_cache && cos && sin && attn_out && pos_dev && workspace && flags && Wo && resid && y_o, VG_ERR_ARG, "vg_decode_layer: null pointer");
  const int roles = vg_decode_layer_roles(H, Hkv, D, hidden, inter, dtype);
  const int want = Wgu ? 3 : 1;
  VG_CHECK(roles >= want, VG_ERR_UNSUPPORTED, "vg_decode_layer: H=%d Hkv=%d D=%d hidden=%d inter=%d dtype=%d: %d role(s) available, %d asked for",
           H, Hkv, D, hidden, inter, dtype, roles, want);
  VG_CHECK(want == 1 || (norm_w && Wdown && act && y), VG_ERR_ARG, "vg_decode_layer: the MLP roles need norm_w, Wgu, Wdown, act, y");
  VG_CHECK(window >= 0 && max_len > 0, VG_ERR_ARG, "vg_decode_layer: bad window / max_len");
  const int es = dtype == VG_BF16 ? 2 : 4, kpc = 16 / es;
  VG_CHECK(ldo % kpc == 0 && (!Wgu || (ldgu % kpc == 0 && lddown % kpc == 0)), VG_ERR_ARG, "vg_decode_layer: weight row strides must be multiples of %d", kpc);
  VG_CHECK((((uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)Wo | (uintptr_t)Wgu | (uintptr_t)Wdown | (uintptr_t)norm_w | (uintptr_t)attn_out |
             (uintptr_t)y_o | (uintptr_t)act) & 15) == 0 && ((uintptr_t)flags & 127) == 0, VG_ERR_ARG, "vg_decode_layer: alignment (16 bytes; flags 128)");
  const int64_t need = vg_decode_attention_ws_floats(H, Hkv, D, max_len);
  VG_CHECK(ws_floats >= need, VG_ERR_ARG, "vg_decode_layer: workspace %lld < %lld floats", (long long)ws_floats, (long long)need);
  const int nsplit = (max_len + 63) / 64;
  VG_CHECK(nsplit <= 128, VG_ERR_UNSUPPORTED, "vg_decode_layer: max_len %d > 8192", max_len);
  DecLayerArgs q{};
  q.a = DecAttnArgs{qkv, k_cache, v_cache, cos, sin, attn_out, workspace, (int*)(workspace + (need - Hkv)), pos_dev, H, Hkv, D, nsplit, scale, window};
  q.flags = flags;
  q.nroles = want;
  const DecSplit so = dec_pair_split((hidden + 1) / 2, 2, DEC_MAX_PPW);      // o and down: N = hidden
  q.r[0].nblocks = so.blocks;
  q.r[0].g = DecGemvArgs{attn_out, Wo, y_o, nullptr, resid, hidden, hidden, ldo, 0.f, so.ppw, nullptr};
  int blocks = nsplit * Hkv + q.r[0].nblocks;
  if (want == 3) {
    const DecSplit sgu = dec_pair_split(inter, 2, DEC_MAX_PPW);              // gate|up (GLU): inter pairs
    q.r[1].nblocks = sgu.blocks;
    q.r[1].g = DecGemvArgs{y_o, Wgu, act, norm_w, nullptr, inter, hidden, ldgu, eps, sgu.ppw, nullptr};
    q.r[2].nblocks = so.blocks;
    q.r[2].g = DecGemvArgs{act, Wdown, y, nullptr, y_o, hidden, inter, lddown, 0.f, so.ppw, nullptr};
    blocks += q.r[1].nblocks + q.r[2].nblocks;
  }
  const int G = H / Hkv, KP = 256 / (D / kpc);
  size_t lds = sizeof(float) * ((size_t)G * D + 2 * D + 4 * G * 64 + G * 64 + 2 * G + 4 + (size_t)KP * G * D);
  const size_t xbytes = (size_t)(want == 3 ? inter : hidden) * es;
  if (xbytes > lds) lds = xbytes;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == VG_BF16 && D == 128) {
    if (want == 3) return launch_decode_layer<bf16_t, 4, 128, 2, 4, 7>(q, blocks, lds, st);
    return launch_decode_layer<bf16_t, 4, 128, 2, 4, 0>(q, blocks, lds, st);
  }
  if (dtype == VG_BF16) return launch_decode_layer<bf16_t, 1, 96, 3, 2, 0>(q, blocks, lds, st);
  return launch_decode_layer<float, 4, 128, 4, 4, 0>(q, blocks, lds, st);
}
