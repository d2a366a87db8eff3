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
#include "vg_common.h"

namespace {

struct GemmRowsArgs {
  const bf16_t* x; int64_t ldx; const bf16_t* W; int64_t ldw; void* y; int64_t ldy; const float* nw; float eps; const void* R; int64_t ldr;
  int N, K, B, ntile;
};

constexpr int GR_UNIT = 8;     // MFMAs (of 32 k) per unit

template <int UPT> constexpr int gr_pitch() { return 256 * UPT * 2 + 16; }       // bytes between the rows of a wave's x slab
template <int UPT> constexpr int gr_lds() { return 4 * 16 * gr_pitch<UPT>(); }

template <typename TO, bool GLU, int TPW, int UPT>
__global__ __launch_bounds__(256) void decode_gemm_rows_kernel(GemmRowsArgs p) {
  constexpr int PK = 256 * UPT, PITCH = gr_pitch<UPT>(), MT = TPW * (GLU ? 2 : 1), NU = MT * UPT;
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

  // ---- weight cursor: lane (lr, lg) reads weight row lr of every tile at k = 8 lg + 32 j
  const bf16_t* wrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int gt = min(blockIdx.x * TPW + mt % TPW, p.ntile - 1);      // a tile past the end re-reads the last one; nothing of it is stored
    const int64_t n = (int64_t)min(gt * 16 + lr, p.N - 1) + (GLU && mt >= TPW ? p.N : 0);      // ... as a row past N (a ragged last tile) re-reads row N - 1
    wrow[mt] = p.W + n * p.ldw + (int64_t)wave * slice + 8 * lg;
  }
  auto issue = [&](u32x4_t (&wb)[GR_UNIT], int ph, int i) {            // i may run past the phase: units NU, NU + 1 are the next phase's first two
    const int phc = i >= NU ? min(ph + 1, nph - 1) : ph;               // past the last phase: a valid address again, never consumed
    const int ii = i >= NU ? i - NU : i;
    const int mt = ii / UPT, uu = ii % UPT;
    const bf16_t* w = wrow[mt] + phc * PK + uu * 256;
#pragma unroll
    for (int j = 0; j < GR_UNIT; ++j) wb[j] = __builtin_nontemporal_load((const u32x4_t*)(w + 32 * j));
  };

  f32x4_t acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  auto consume = [&](const u32x4_t (&wb)[GR_UNIT], int i) {
    const int mt = i / UPT, uu = i % UPT;
    const char* xrow = xs + lr * PITCH + (uu * 256 + 8 * lg) * 2;
#pragma unroll
    for (int j = 0; j < GR_UNIT; ++j) {
      const bf16x8_t a = *(const bf16x8_t*)(xrow + 64 * j);
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, __builtin_bit_cast(bf16x8_t, wb[j]), acc[mt], 0, 0, 0);
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

  u32x4_t wa[GR_UNIT], wb[GR_UNIT];
  issue(wa, 0, 0);
  issue(wb, 0, 1);
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
      if (i % 2 == 0) { consume(wa, i); issue(wa, ph, i + 2); }
      else { consume(wb, i); issue(wb, ph, i + 2); }
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
    if constexpr (GLU) {
      float g = bf2f(f2bf(total(t))), u = bf2f(f2bf(total(TPW + t)));      // gate / up materialise in bf16, as dec_gemv_store
      g = bf2f(f2bf(vg_silu(g)));
      v = g * u;
    } else {
      v = total(t);
    }
    if (R) v += vg_elt<TO>::ld(R);
    vg_elt<TO>::st(y, v);
  }
}

template <typename TO, bool GLU, int TPW, int UPT>
int launch_gr(const GemmRowsArgs& p, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    if (hipFuncSetAttribute((const void*)decode_gemm_rows_kernel<TO, GLU, TPW, UPT>, hipFuncAttributeMaxDynamicSharedMemorySize, gr_lds<UPT>()) != hipSuccess) {
      vg_set_error("vg_decode_gemm_rows: cannot reserve %d bytes of LDS", gr_lds<UPT>());
      return VG_ERR_LAUNCH;
    }
    attr = true;
  }
  decode_gemm_rows_kernel<TO, GLU, TPW, UPT><<<(p.ntile + TPW - 1) / TPW, 256, gr_lds<UPT>(), st>>>(p);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

template <typename TO, bool GLU>
int launch_gr_shape(const GemmRowsArgs& p, hipStream_t st) {
  // tiles per workgroup: the fewest that keep the grid within ~2 workgroups per CU (512), at most 4
  const int tpw = p.ntile <= 512 ? 1 : p.ntile <= 1024 ? 2 : 4;
  if (p.K == 3072) {       // one phase of 768 k per wave
    return tpw == 1 ? launch_gr<TO, GLU, 1, 3>(p, st) : tpw == 2 ? launch_gr<TO, GLU, 2, 3>(p, st) : launch_gr<TO, GLU, 4, 3>(p, st);
  }
  return tpw == 1 ? launch_gr<TO, GLU, 1, 2>(p, st) : tpw == 2 ? launch_gr<TO, GLU, 2, 2>(p, st) : launch_gr<TO, GLU, 4, 2>(p, st);
}

}  // namespace

extern "C" int vg_decode_gemm_rows_supported(int N, int K) {
  return N > 0 && (K == 3072 || K == 4096 || K == 8192 || K == 14336);
}

extern "C" int vg_decode_gemm_rows(const void* x, int64_t ldx, const void* W, int64_t ldw, void* y, int64_t ldy, const float* norm_w, float eps,
                                   const void* R, int64_t ldr, int N, int K, int B, int glu, int out_dtype, vg_stream_t stream) {
  VG_CHECK(x && W && y && B >= 1 && B <= 16, VG_ERR_ARG, "vg_decode_gemm_rows: bad args B=%d", B);
  VG_CHECK(out_dtype == VG_BF16 || out_dtype == VG_F32, VG_ERR_ARG, "vg_decode_gemm_rows: out_dtype %d (bf16 or fp32)", out_dtype);
  VG_CHECK(vg_decode_gemm_rows_supported(N, K), VG_ERR_UNSUPPORTED,
           "vg_decode_gemm_rows: K one of 3072, 4096, 8192, 14336 only (N=%d K=%d)", N, K);
  VG_CHECK(ldw % 8 == 0 && ldx % 8 == 0 && ldw >= K && ((((uintptr_t)x) | ((uintptr_t)W) | ((uintptr_t)norm_w)) & 15) == 0, VG_ERR_ARG,
           "vg_decode_gemm_rows: alignment (16 bytes; ldx / ldw multiples of 8, ldw >= K)");
  VG_CHECK(!norm_w || K <= 4096, VG_ERR_UNSUPPORTED, "vg_decode_gemm_rows: the norm form exists at K <= 4096 only (B=%d K=%d)", B, K);
  GemmRowsArgs p{(const bf16_t*)x, ldx, (const bf16_t*)W, ldw, y, ldy, norm_w, eps, R, ldr, N, K, B, (N + 15) / 16};
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == VG_F32) return glu ? launch_gr_shape<float, true>(p, st) : launch_gr_shape<float, false>(p, st);
  return glu ? launch_gr_shape<bf16_t, true>(p, st) : launch_gr_shape<bf16_t, false>(p, st);
}
