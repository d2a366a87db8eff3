// B-row decode projections on the matrix pipe (the decode mode decode_gemv = "mfma"): y[b] = f(x[b]) . W^T (+ R[b]) for B <= 16 rows.
// The batch is ALWAYS one 16-row operand of v_mfma_f32_16x16x32_bf16 (A = x: row l & 15 = batch row, k = 8 (l >> 4) + j; B = 16 weight rows, column
// l & 15 = weight row, the same k), rows >= B are zeros, so a weight tile costs the same whatever B is and the accumulators are four registers per 16
// weight rows.  Row b of the result depends on x[b] and W alone: the walk below never looks at B, and an MFMA output element is the dot product of its
// own A row and B column — row b of a B-row launch IS the one-row launch on that row, bit for bit, whatever the other rows hold.
//
// Walk.  A workgroup (4 waves) owns TPW consecutive 16-row weight tiles (x 2 matrices when GLU: gate rows | up rows; the last tile may be ragged:
// a vocabulary with added tokens is no multiple of 16).  The K axis is split four ways:
// wave w owns k in [w K/4, (w + 1) K/4) of every tile of its workgroup and walks it in phases of PK = 256 UPT elements; inside a phase it goes tile by
// tile, a tile-phase being UPT units of eight MFMAs (256 k).  A lane's eight 16-byte weight loads of a unit are 64 bytes apart in ONE weight row: two
// consecutive loads of the wave finish 16 whole 128-byte lines.  Weights go global -> VGPR (non-temporal), two units in flight; x goes through a
// wave-private LDS slab [16][PK] (row pitch PK x 2 + 16 bytes: the 16 rows of a ds_read_b128 fall into distinct banks), staged per phase, the next
// phase's rows requested one phase ahead.  No workgroup barrier inside the walk, and none between workgroups at all.
// Sums.  fp32 on the MFMA, one accumulator per tile, in k order inside the wave's slice; the four slices are added in LDS as ((w0 + w1) + w2) + w3.
// Roundings.  RMSNorm prologue with the decode GEMVs' arithmetic (256 threads x chunks tid + 256 i, wave sums, the 4-wave total; x rstd -> bf16,
// x weight -> bf16); SwiGLU / residual epilogue = dec_gemv_store's; one rounding of the output.
#include <type_traits>

#include "vg_common.h"
#include "vg_decode_launch.h"

namespace {

struct GemmRowsArgs {
  const bf16_t* x; int64_t ldx; const void* W; int64_t ldw; void* y; int64_t ldy; const float* nw; float eps; const void* R; int64_t ldr;
  int N, K, B, ntile;
  // (ldw: bf16 elements for bf16 weights, bytes for e4m3 and packed e2m1 rows)
  const float* wscale;     // e4m3: one fp32 scale per weight row
  int head;                // e2m1: bytes of a packed row's scale head (64 SPL), the codes follow it
};

constexpr int GR_UNIT = 8;     // MFMAs (of 32 k) per unit

enum { GR_BF16 = 0, GR_E4M3 = 1, GR_E2M1 = 2 };
// MPL: MFMAs a 16-byte load feeds (an element is 2 / MPL bytes); DMAX: units in flight at most (8 / MPL loads of 16 bytes each)
template <int F> struct gr_fmt {
  typedef typename std::conditional<F == GR_BF16, bf16_t, char>::type WT;      // what a weight pointer steps over: k elements are wk(k) of them
  template <typename T> static constexpr T wk(T k) { return F == GR_E2M1 ? k / 2 : k; }
  static constexpr int MPL = F == GR_BF16 ? 1 : F == GR_E4M3 ? 2 : 4, DMAX = F == GR_BF16 ? 2 : F == GR_E4M3 ? 4 : 8;
};

// units in flight: with more than one phase (UPT == 2) the ring must divide the NU units of a phase, so that a unit's buffer is known at compile time
constexpr int gr_depth(int dmax, int NU, int UPT) {
  if (UPT == 3) return NU < dmax ? NU : dmax;
  int d = 2;
  while (d * 2 <= dmax && NU % (d * 2) == 0) d *= 2;
  return d;
}

// MFMA m's B operand (8 bf16) out of a lane's 16-byte load
template <int F>
__device__ __forceinline__ bf16x8_t gr_operand(const u32x4_t& w, int m, float sc) {
  if constexpr (F == GR_BF16) {
    return __builtin_bit_cast(bf16x8_t, w);
  } else if constexpr (F == GR_E4M3) {
    const uint32_t a = w[2 * m], b = w[2 * m + 1];
    const u32x4_t r{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, false)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, true)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, false)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, true))};
    return __builtin_bit_cast(bf16x8_t, r);
  } else {
    const uint32_t a = w[m];
    const u32x4_t r{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 0)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 1)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 2)),
                    __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, sc, 3))};
    return __builtin_bit_cast(bf16x8_t, r);
  }
}

// e2m1: LDS bytes of the staged scales per tile (x MT): [4 waves][16 rows][4 lg][SLG], SLG = the slice's loads per lane rounded up to 4
__host__ __device__ constexpr int gr_slg(int K) { return (K / 512 + 3) & ~3; }

template <int UPT> constexpr int gr_pitch() { return 256 * UPT * 2 + 16; }       // bytes between the rows of a wave's x slab
template <int UPT> constexpr int gr_lds() { return 4 * 16 * gr_pitch<UPT>(); }

template <int F, typename TO, bool GLU, int TPW, int UPT>
__global__ __launch_bounds__(256) void decode_gemm_rows_kernel(GemmRowsArgs p) {
  constexpr int PK = 256 * UPT, PITCH = gr_pitch<UPT>(), MT = TPW * (GLU ? 2 : 1), NU = MT * UPT;
  constexpr int MPL = gr_fmt<F>::MPL, LPU = GR_UNIT / MPL, D = gr_depth(gr_fmt<F>::DMAX, NU, UPT);
  static_assert(D <= NU && (UPT == 3 || NU % D == 0), "a unit's ring buffer is a compile-time index");
  constexpr int XC = (PK / 8 + 63) / 64;           // 16-byte chunks of a slab row per lane
  static_assert(4 * MT * 1024 <= gr_lds<UPT>(), "the partial sums reuse the x slabs");
  extern __shared__ __attribute__((aligned(16))) char gr_smem[];
  __shared__ float red[16][4];
  __shared__ float rstd_s[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int slice = p.K / 4, nph = slice / PK;
  char* xs = gr_smem + wave * (16 * PITCH);

  // ---- RMSNorm statistics: per row the single-row kernel's sum (thread tid: chunks tid + 256 i; wave_sum; the four waves in order)
  if (p.nw) {
    const int nch = p.K / 8;
    for (int r = 0; r < p.B; ++r) {
      const u32x4_t* xg = (const u32x4_t*)(p.x + (int64_t)r * p.ldx);
      float ss = 0.f;
      for (int c = tid; c < nch; c += 256) {
        const u32x4_t v = xg[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float f0 = __uint_as_float(v[e] << 16), f1 = __uint_as_float(v[e] & 0xffff0000u);
          ss += f0 * f0;
          ss += f1 * f1;
        }
      }
      ss = wave_sum(ss);
      if (lane == 0) red[r][wave] = ss;
    }
    __syncthreads();
    if (tid < 16) rstd_s[tid] = tid < p.B ? rsqrtf((red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3]) / (float)p.K + p.eps) : 0.f;
    __syncthreads();
  }

  // ---- weight cursor: lane (lr, lg) reads weight row lr of every tile, 16 bytes at byte 16 lg + 64 j of a unit (k = 8 MPL lg + 32 MPL j)
  typedef typename gr_fmt<F>::WT WT;
  constexpr int W16 = 16 / sizeof(WT);                                 // 16 bytes in WT
  const WT* wrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int gt = min(blockIdx.x * TPW + mt % TPW, p.ntile - 1);      // a tile past the end re-reads the last one; nothing of it is stored
    const int64_t n = (int64_t)min(gt * 16 + lr, p.N - 1) + (GLU && mt >= TPW ? p.N : 0);      // ... as a row past N (a ragged last tile) re-reads row N - 1
    wrow[mt] = (const WT*)p.W + n * p.ldw + (F == GR_E2M1 ? p.head : 0) + gr_fmt<F>::wk((int64_t)wave * slice) + W16 * lg;
  }
  auto issue = [&](u32x4_t (&wb)[LPU], int ph, int i) {                // i may run past the phase: units NU .. NU + D - 1 are the next phase's first
    const int phc = i >= NU ? min(ph + 1, nph - 1) : ph;               // past the last phase: a valid address again, never consumed
    const int ii = i >= NU ? i - NU : i;
    const int mt = ii / UPT, uu = ii % UPT;
    const WT* w = wrow[mt] + gr_fmt<F>::wk(phc * PK + uu * 256);
#pragma unroll
    for (int j = 0; j < LPU; ++j) wb[j] = __builtin_nontemporal_load((const u32x4_t*)(w + 4 * W16 * j));
  };

  // ---- e2m1: the scale heads of the workgroup's 16 MT rows, once, into LDS in walk order.  Head byte h = lane SPL + u holds block b = 64 u + lane;
  // block b belongs to wave b / S (S = blocks per slice), and block 4 t + g of a slice is read by lane group g at load t = 2 (UPT ph + unit) + j
  const int slg = gr_slg(p.K);
  unsigned char* ssc = (unsigned char*)gr_smem + gr_lds<UPT>();
  if constexpr (F == GR_E2M1) {
    const int S = slice / 32, nb = p.K / 32, magic = 65536 / S + 1;    // b / S = (b magic) >> 16 for b < 512 and S of 24, 32, 64, 112
    const int hsh = 31 - __builtin_clz(p.head / 16), ssh = 31 - __builtin_clz(p.head / 64);      // chunks per head, SPL: powers of two
    for (int c = tid; c < (MT * 16) << hsh; c += 256) {
      const int r = c >> hsh, hc = c & ((1 << hsh) - 1), mt = r >> 4, row = r & 15;
      const int64_t n = (int64_t)min(min(blockIdx.x * TPW + mt % TPW, p.ntile - 1) * 16 + row, p.N - 1) + (GLU && mt >= TPW ? p.N : 0);      // the rows of wrow[]
      const u32x4_t v = *(const u32x4_t*)((const char*)p.W + n * p.ldw + hc * 16);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int h = hc * 16 + e, b = (h >> ssh) + 64 * (h & ((1 << ssh) - 1));
        if (b < nb) {
          const int w = (b * magic) >> 16, bs = b - w * S;
          ssc[(((w * MT + mt) * 16 + row) * 4 + (bs & 3)) * slg + (bs >> 2)] = (unsigned char)(v[e >> 2] >> (8 * (e & 3)));
        }
      }
    }
    __syncthreads();
  }

  f32x4_t acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  auto consume = [&](const u32x4_t (&wb)[LPU], int ph, int i) {
    const int mt = i / UPT, uu = i % UPT;
    const char* xrow = xs + lr * PITCH + (uu * 256 + 8 * MPL * lg) * 2;
    uint32_t s2 = 0;                                                   // e2m1: the scale bytes of this unit's two loads
    if constexpr (F == GR_E2M1) s2 = *(const uint16_t*)(ssc + (((wave * MT + mt) * 16 + lr) * 4 + lg) * slg + 2 * (ph * UPT + uu));
#pragma unroll
    for (int j = 0; j < LPU; ++j) {
      auto feed = [&](const u32x4_t& w, float sc) {
#pragma unroll
        for (int m = 0; m < MPL; ++m) {
          const bf16x8_t a = *(const bf16x8_t*)(xrow + (32 * MPL * j + 8 * m) * 2);
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, gr_operand<F>(w, m, sc), acc[mt], 0, 0, 0);
        }
      };
      if constexpr (F == GR_E2M1) {
        // scale byte 0: the block counts as zero.  The conversion reads the exponent field of its scale operand only (0.0f acts as 2^-127,
        // measured: sums of 1e-36), so the zero is made here: +0 codes convert to +0 under any scale
        const uint32_t sb = (s2 >> (8 * j)) & 0xffu;
        feed(sb ? wb[j] : u32x4_t{0u, 0u, 0u, 0u}, __uint_as_float(sb << 23));      // 2^(byte - 127)
      } else {
        feed(wb[j], 1.0f);
      }
    }
  };

  // ---- x staging: chunk c of slab row r = x[r][w slice + ph PK + 8 c ..], normalised on the way; rows >= B are zeros
  auto xaddr = [&](int r, int ph, int c) { return (const u32x4_t*)(p.x + (int64_t)min(r, p.B - 1) * p.ldx + (int64_t)wave * slice + ph * PK) + c; };
  auto xnorm = [&](u32x4_t v, int r, int ph, int c) {
    if (r >= p.B) return u32x4_t{0u, 0u, 0u, 0u};
    if (p.nw) {
      const float rs = rstd_s[r];
      const f32x4_t* nw4 = (const f32x4_t*)(p.nw + (int64_t)wave * slice + ph * PK) + 2 * c;
      const f32x4_t g0 = nw4[0], g1 = nw4[1];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float f0 = bf2f(f2bf(__uint_as_float(v[e] << 16) * rs)) * (e < 2 ? g0[2 * e] : g1[2 * e - 4]);
        const float f1 = bf2f(f2bf(__uint_as_float(v[e] & 0xffff0000u) * rs)) * (e < 2 ? g0[2 * e + 1] : g1[2 * e - 3]);
        v[e] = f2bf2(f0, f1);
      }
    }
    return v;
  };

  // the ring of D units in flight: two buffers for bf16, more (r a constant wherever it is used) for the formats whose units are fewer bytes
  u32x4_t w0[LPU], w1[LPU];
  u32x4_t wr[D > 2 ? D - 2 : 1][LPU];
  issue(w0, 0, 0);
  issue(w1, 0, 1);
  if constexpr (D > 2) {
#pragma unroll
    for (int d = 2; d < D; ++d) issue(wr[d - 2], 0, d);
  }
#pragma unroll
  for (int i = 0; i < XC; ++i) {
    const int c = min(lane + 64 * i, PK / 8 - 1);
    u32x4_t xv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) xv[r] = *xaddr(r, 0, c);
    if (lane + 64 * i < PK / 8) {
#pragma unroll
      for (int r = 0; r < 16; ++r) *(u32x4_t*)(xs + r * PITCH + c * 16) = xnorm(xv[r], r, 0, c);
    }
  }
  __builtin_amdgcn_wave_barrier();

  for (int ph = 0; ph < nph; ++ph) {
    u32x4_t xn[16];
    if constexpr (UPT == 2) {                      // more than one phase only with 64 chunks per slab row: one per lane
      if (ph + 1 < nph) {
#pragma unroll
        for (int r = 0; r < 16; ++r) xn[r] = *xaddr(r, ph + 1, lane);
      }
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      if (i % D == 0) { consume(w0, ph, i); issue(w0, ph, i + D); }
      else if (i % D == 1) { consume(w1, ph, i); issue(w1, ph, i + D); }
      else { consume(wr[D > 2 ? i % D - 2 : 0], ph, i); issue(wr[D > 2 ? i % D - 2 : 0], ph, i + D); }
    }
    if constexpr (UPT == 2) {
      if (ph + 1 < nph) {
        __builtin_amdgcn_wave_barrier();           // the wave's reads of this phase are issued: LDS serves a wave in order
#pragma unroll
        for (int r = 0; r < 16; ++r) *(u32x4_t*)(xs + r * PITCH + lane * 16) = xnorm(xn[r], r, ph + 1, lane);
        __builtin_amdgcn_wave_barrier();
      }
    }
  }

  // ---- the four K slices, added in a fixed order; wave w then owns accumulator register w = batch rows 4 (l >> 4) + w
  __syncthreads();
  f32x4_t* part = (f32x4_t*)gr_smem;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) part[(wave * MT + mt) * 64 + lane] = acc[mt];
  __syncthreads();
  const float* pf = (const float*)gr_smem;
  const int b = 4 * lg + wave;
  auto total = [&](int mt) {
    float s = pf[((0 * MT + mt) * 64 + lane) * 4 + wave];
    s += pf[((1 * MT + mt) * 64 + lane) * 4 + wave];
    s += pf[((2 * MT + mt) * 64 + lane) * 4 + wave];
    s += pf[((3 * MT + mt) * 64 + lane) * 4 + wave];
    return s;
  };
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int gt = blockIdx.x * TPW + t;
    const int n = gt * 16 + lr;
    if (n >= p.N || b >= p.B) continue;
    TO* y = (TO*)p.y + (int64_t)b * p.ldy + n;
    const TO* R = p.R ? (const TO*)p.R + (int64_t)b * p.ldr + n : nullptr;
    float v;
    const float s0 = F == GR_E4M3 ? p.wscale[n] : 1.f;                     // e4m3: the row scales leave the dot products, as vg_decode_gemv_w8
    if constexpr (GLU) {
      const float s1 = F == GR_E4M3 ? p.wscale[p.N + n] : 1.f;
      float g = bf2f(f2bf(F == GR_E4M3 ? total(t) * s0 : total(t))), u = bf2f(f2bf(F == GR_E4M3 ? total(TPW + t) * s1 : total(TPW + t)));      // gate / up materialise in bf16, as dec_gemv_store
      g = bf2f(f2bf(vg_silu(g)));
      v = g * u;
    } else {
      v = F == GR_E4M3 ? total(t) * s0 : total(t);
    }
    if (R) v += vg_elt<TO>::ld(R);
    vg_elt<TO>::st(y, v);
  }
}

template <int F, typename TO, bool GLU, int TPW, int UPT>
int launch_gr(const GemmRowsArgs& p, hipStream_t st, const char* who) {
  constexpr int MT = TPW * (GLU ? 2 : 1);
  // e2m1: the staged scale heads behind the x slabs, MT x 256 x SLG bytes (reserved once for the longest row of this UPT)
  constexpr int lds_max = gr_lds<UPT>() + (F == GR_E2M1 ? MT * 256 * gr_slg(UPT == 3 ? 3072 : 14336) : 0);
  const int lds = gr_lds<UPT>() + (F == GR_E2M1 ? MT * 256 * gr_slg(p.K) : 0);
  static bool attr = false;
  if (!attr) {
    if (hipFuncSetAttribute((const void*)decode_gemm_rows_kernel<F, TO, GLU, TPW, UPT>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max) != hipSuccess) {
      vg_set_error("%s: cannot reserve %d bytes of LDS", who, lds_max);
      return VG_ERR_LAUNCH;
    }
    attr = true;
  }
  decode_gemm_rows_kernel<F, TO, GLU, TPW, UPT><<<(p.ntile + TPW - 1) / TPW, 256, lds, st>>>(p);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

template <int F, typename TO, bool GLU>
int launch_gr_shape(const GemmRowsArgs& p, hipStream_t st, const char* who) {
  // tiles per workgroup: the fewest that keep the grid within ~2 workgroups per CU (512), at most 4
  const int tpw = p.ntile <= 512 ? 1 : p.ntile <= 1024 ? 2 : 4;
  if (p.K == 3072) {       // one phase of 768 k per wave
    return tpw == 1 ? launch_gr<F, TO, GLU, 1, 3>(p, st, who) : tpw == 2 ? launch_gr<F, TO, GLU, 2, 3>(p, st, who) : launch_gr<F, TO, GLU, 4, 3>(p, st, who);
  }
  return tpw == 1 ? launch_gr<F, TO, GLU, 1, 2>(p, st, who) : tpw == 2 ? launch_gr<F, TO, GLU, 2, 2>(p, st, who) : launch_gr<F, TO, GLU, 4, 2>(p, st, who);
}

template <int F>
int launch_gr_fmt(const GemmRowsArgs& p, int glu, int out_dtype, hipStream_t st, const char* who) {
  if (out_dtype == VG_F32) return glu ? launch_gr_shape<F, float, true>(p, st, who) : launch_gr_shape<F, float, false>(p, st, who);
  return glu ? launch_gr_shape<F, bf16_t, true>(p, st, who) : launch_gr_shape<F, bf16_t, false>(p, st, who);
}

bool gr_shape(int N, int K) { return N > 0 && (K == 3072 || K == 4096 || K == 8192 || K == 14336); }

}  // namespace

extern "C" int vg_decode_gemm_rows_supported(int N, int K) { return gr_shape(N, K); }

extern "C" int vg_decode_gemm_rows(const void* x, int64_t ldx, const void* W, int64_t ldw, void* y, int64_t ldy, const float* norm_w, float eps,
                                   const void* R, int64_t ldr, int N, int K, int B, int glu, int out_dtype, vg_stream_t stream) {
  VG_CHECK(x && W && y && dec_rows_b_ok(B), VG_ERR_ARG, "vg_decode_gemm_rows: bad args B=%d", B);
  VG_CHECK(out_dtype == VG_BF16 || out_dtype == VG_F32, VG_ERR_ARG, "vg_decode_gemm_rows: out_dtype %d (bf16 or fp32)", out_dtype);
  VG_CHECK(vg_decode_gemm_rows_supported(N, K), VG_ERR_UNSUPPORTED,
           "vg_decode_gemm_rows: K one of 3072, 4096, 8192, 14336 only (N=%d K=%d)", N, K);
  VG_CHECK(ldw % 8 == 0 && ldx % 8 == 0 && ldw >= K && ((((uintptr_t)x) | ((uintptr_t)W) | ((uintptr_t)norm_w)) & 15) == 0, VG_ERR_ARG,
           "vg_decode_gemm_rows: alignment (16 bytes; ldx / ldw multiples of 8, ldw >= K)");
  VG_CHECK(!norm_w || K <= 4096, VG_ERR_UNSUPPORTED, "vg_decode_gemm_rows: the norm form exists at K <= 4096 only (B=%d K=%d)", B, K);
  GemmRowsArgs p{(const bf16_t*)x, ldx, W, ldw, y, ldy, norm_w, eps, R, ldr, N, K, B, (N + 15) / 16, nullptr, 0};
  return launch_gr_fmt<GR_BF16>(p, glu, out_dtype, (hipStream_t)stream, "vg_decode_gemm_rows");
}

extern "C" int vg_decode_gemm_w8_rows_supported(int N, int K) { return gr_shape(N, K); }

extern "C" int vg_decode_gemm_w8_rows(const void* x, int64_t ldx, const uint8_t* W8, int64_t ldw, const float* wscale, void* y, int64_t ldy,
                                      const float* norm_w, float eps, const void* R, int64_t ldr, int N, int K, int B, int glu, int out_dtype,
                                      vg_stream_t stream) {
  VG_CHECK(x && W8 && wscale && y && dec_rows_b_ok(B), VG_ERR_ARG, "vg_decode_gemm_w8_rows: bad args B=%d", B);
  VG_CHECK(out_dtype == VG_BF16 || out_dtype == VG_F32, VG_ERR_ARG, "vg_decode_gemm_w8_rows: out_dtype %d (bf16 or fp32)", out_dtype);
  VG_CHECK(gr_shape(N, K), VG_ERR_UNSUPPORTED, "vg_decode_gemm_w8_rows: K one of 3072, 4096, 8192, 14336 only (N=%d K=%d)", N, K);
  VG_CHECK(ldw % 16 == 0 && ldx % 8 == 0 && ldw >= K && ((((uintptr_t)x) | ((uintptr_t)W8) | ((uintptr_t)norm_w)) & 15) == 0, VG_ERR_ARG,
           "vg_decode_gemm_w8_rows: alignment (16 bytes; ldx a multiple of 8, ldw of 16, ldw >= K)");
  VG_CHECK(!norm_w || K <= 4096, VG_ERR_UNSUPPORTED, "vg_decode_gemm_w8_rows: the norm form exists at K <= 4096 only (B=%d K=%d)", B, K);
  GemmRowsArgs p{(const bf16_t*)x, ldx, W8, ldw, y, ldy, norm_w, eps, R, ldr, N, K, B, (N + 15) / 16, wscale, 0};
  return launch_gr_fmt<GR_E4M3>(p, glu, out_dtype, (hipStream_t)stream, "vg_decode_gemm_w8_rows");
}

extern "C" int vg_decode_gemm_w4_rows_supported(int N, int K) { return gr_shape(N, K); }

extern "C" int vg_decode_gemm_w4_rows(const void* x, int64_t ldx, const uint8_t* W4, int64_t ldw_bytes, void* y, int64_t ldy, const float* norm_w,
                                      float eps, const void* R, int64_t ldr, int N, int K, int B, int glu, int out_dtype, vg_stream_t stream) {
  VG_CHECK(x && W4 && y && dec_rows_b_ok(B), VG_ERR_ARG, "vg_decode_gemm_w4_rows: bad args B=%d", B);
  VG_CHECK(out_dtype == VG_BF16 || out_dtype == VG_F32, VG_ERR_ARG, "vg_decode_gemm_w4_rows: out_dtype %d (bf16 or fp32)", out_dtype);
  VG_CHECK(gr_shape(N, K), VG_ERR_UNSUPPORTED, "vg_decode_gemm_w4_rows: K one of 3072, 4096, 8192, 14336 only (N=%d K=%d)", N, K);
  const int head = 64 * (K <= 4096 ? 2 : K == 8192 ? 4 : 8);      // SPL scale bytes per lane: the packed rows of vg_decode_gemv_w4
  VG_CHECK(ldw_bytes % 16 == 0 && ldx % 8 == 0 && ldw_bytes >= head + K / 2 && ((((uintptr_t)x) | ((uintptr_t)W4) | ((uintptr_t)norm_w)) & 15) == 0,
           VG_ERR_ARG, "vg_decode_gemm_w4_rows: alignment (16 bytes; ldx a multiple of 8, ldw_bytes of 16 and >= %d: packed rows)", head + K / 2);
  VG_CHECK(!norm_w || K <= 4096, VG_ERR_UNSUPPORTED, "vg_decode_gemm_w4_rows: the norm form exists at K <= 4096 only (B=%d K=%d)", B, K);
  GemmRowsArgs p{(const bf16_t*)x, ldx, W4, ldw_bytes, y, ldy, norm_w, eps, R, ldr, N, K, B, (N + 15) / 16, nullptr, head};
  return launch_gr_fmt<GR_E2M1>(p, glu, out_dtype, (hipStream_t)stream, "vg_decode_gemm_w4_rows");
}
