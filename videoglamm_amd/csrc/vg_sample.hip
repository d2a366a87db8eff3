// Sampled decoding on the device: HF generate(do_sample=True)'s Temperature -> TopK -> TopP warpers and the draw, for one fp32
// logits row.  The result is written as the packed (ordered value bits, ~index) key vg_argmax_partial leaves in
// acc[0], so vg_decode_step_end consumes it unchanged.
//
// Contract (transformers 4.41 _get_logits_warper + _sample):
//   y = x / T (a true fp32 division; -0 counts as +0); top-k keeps every entry >= the k-th largest y (ties at the threshold all kept, k = 0 or k >= n: off);
//   top-p (p < 1) keeps, in descending order, the entries whose probability mass ABOVE them is < p (the largest always kept);
//   the token is the inverse CDF of softmax(kept) at u, walking the kept entries by descending y, ties by ascending index;
//   u = (philox4x32_10(key = seed, counter = (step, 0, 0, 0))[0] >> 8) * 2^-24.
//
// Arithmetic: the kernels never sort.  Every cut is a radix select over the 32-bit ordered keys of y (three 11/11/10-bit digits, an LDS
// histogram per digit), weighted either by count (top-k) or by probability mass.  Mass is fixed point: q(y) = floor(expf(y - ymax) * 2^40)
// in uint64, so histogram sums are integer atomics whose result does not depend on their order: the same seed, row and parameters give the
// same token on every run.  The truncation costs < 2^-40 of the largest probability per entry (< 1.2e-7 summed over 128 256 entries).
//
// Two routes, each ONE launch (vg_sample_partial_rows: the same two routes with a row grid dimension, B rows of a batched step in one launch,
// row r bit-identical to the single-row launch on row r):
//   fast (1 <= k <= 64, n <= 64 * 2048): up to 64 workgroups of 256 threads (argmax_stage1's shape); each keeps the top 64 of its slice
//     (a radix select over the slice held in registers) in a workspace; the last workgroup to arrive (self-resetting ticket) merges the
//     <= 4096 candidates in LDS and finishes the chain there.  A slice that had to drop entries tied at its 64th value while that value is
//     the global top-k threshold (tie overflow) makes the last workgroup run the general route over the whole row instead.
//   general (any k): one workgroup of 1024 threads; survivors of the top-k cut that fit in LDS (<= 4096) are compacted and every later pass
//     reads LDS, otherwise every pass re-reads the row from L2.
#include "vg_common.h"
#include <math.h>

namespace {

constexpr int SB = 1024;     // threads of the one workgroup
constexpr int NB = 2048;     // histogram bins (11-bit digits)
constexpr int CAP = 4096;    // candidates held in LDS

struct SampleLds {
  unsigned long long w[NB];
  unsigned int c[NB];
  float cy[CAP];
  int ci[CAP];
  float fred[SB / 64];
  unsigned long long part[64];
  unsigned long long sk[256];       // the fast route's survivors as packed keys, sorted
  unsigned long long sum;
  int ncand, neq, last;
  unsigned int sel_bin, sel_c;
  unsigned long long sel_above, sel_w;
  int found;
};

struct SampleParams {     // the device parameter block (ops.sampling_params): 24 bytes
  float T, p;
  int k, pad;
  unsigned long long seed;
};

struct Sel {
  uint32_t key;
  unsigned long long above, w;
  unsigned int cnt;
};

__device__ __forceinline__ uint32_t okey(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // amax_key's monotone map
}
__device__ __forceinline__ unsigned long long qmass(float y, float ymax) {
  return (unsigned long long)ldexpf(expf(y - ymax), 40);
}

// the fast route's hand-off between workgroups: write-through stores and sc1 loads at agent scope (the decode attention's merge pattern,
// vg_decode.hip: no cache write-back / invalidate fences needed)
template <typename V> __device__ __forceinline__ void st_ag(V* p, V v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename V> __device__ __forceinline__ V ld_ag(const V* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t philox_x0(unsigned long long seed, uint32_t ctr) {
  uint32_t c0 = ctr, c1 = 0, c2 = 0, c3 = 0, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

// f(y, index) over the row (y = x / T) or over the LDS candidates (y kept from the compaction: the same bits)
template <int NT, typename F>
__device__ __forceinline__ void each(const SampleLds& s, bool cand, const float* __restrict__ x, int n, float T, F&& f) {
  if (cand) {
    const int nc = s.ncand < CAP ? s.ncand : CAP;
    for (int i = threadIdx.x; i < nc; i += NT) f(s.cy[i], s.ci[i]);
  } else {
    // four independent loads in flight per thread before any of them is used: one L2 round trip per four entries instead of one per entry
    int i = threadIdx.x;
    for (; i + 3 * NT < n; i += 4 * NT) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = x[i + u * NT];
#pragma unroll
      for (int u = 0; u < 4; ++u) f(v[u] / T + 0.f, i + u * NT);     // y + 0: -0 counts as +0, as HF's float comparisons have it
    }
    for (; i < n; i += NT) f(x[i] / T + 0.f, i);
  }
}

// One digit's pick, after the histogram of this digit is complete in s.c / s.w: walking the bins in descending key order, the first bin b with
// above + (weight of the bins before it) + W(b) > t.  Wave 0 scans: lane l owns bins NB-1-32l down to NB-32-32l; the lanes' partial sums meet in
// LDS and every lane adds up the ones before it (broadcast reads, no cross-lane shuffles).  Every thread calls it (barriers inside).
template <bool MASS>
__device__ __forceinline__ void pick_bin(SampleLds& s, unsigned long long above, unsigned long long t) {
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned long long part = 0;
  if (tid < 64) {
#pragma unroll 8
    for (int j = 0; j < 32; ++j) {
      const int b = NB - 1 - 32 * lane - j;
      part += MASS ? s.w[b] : (unsigned long long)s.c[b];
    }
    s.part[lane] = part;
  }
  __syncthreads();
  if (tid < 64) {
    unsigned long long pre = 0;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
      const unsigned long long v = s.part[j];
      pre += j < lane ? v : 0ull;
    }
    const unsigned long long hit = __ballot(above + pre + part > t);
    const int L = hit ? __ffsll((long long)hit) - 1 : 63;
    if (lane == L) {
      unsigned long long base = above + pre;
      int bs = NB - 32 - 32 * L;
      for (int j = 0; j < 32; ++j) {
        const int b = NB - 1 - 32 * L - j;
        const unsigned long long wb = MASS ? s.w[b] : (unsigned long long)s.c[b];
        if (base + wb > t) {
          bs = b;
          break;
        }
        base += wb;
      }
      s.sel_bin = (unsigned)bs;
      s.sel_above = base;
      s.sel_w = MASS ? s.w[bs] : (unsigned long long)s.c[bs];
      s.sel_c = s.c[bs];
    }
  }
  __syncthreads();
}

// Radix select.  Among the entries e with pred(y, i), keyed by keyfn(y, i) (BITS significant bits) and weighted by q(y) (MASS) or 1:
// the key K* with above <= t < above + W(K*), above = weight of the entries with a key > K*.  W(K*) and the count of K* come back too.
// The caller guarantees t < total weight.  Every thread calls it (barriers inside).
template <int NT, int BITS, bool MASS, typename P, typename KF>
__device__ __forceinline__ Sel select(SampleLds& s, bool cand, const float* __restrict__ x, int n, float T, float ymax, unsigned long long t, P pred, KF keyfn) {
  constexpr int ND = (BITS + 10) / 11;
  const int tid = threadIdx.x;
  uint32_t prefix = 0;
  unsigned long long above = 0, wsel = 0;
  unsigned int csel = 0;
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    const int shift = BITS - 11 * (d + 1) > 0 ? BITS - 11 * (d + 1) : 0;
    const int width = BITS - 11 * d - shift;
    const int hs = shift + width;
    for (int b = tid; b < NB; b += NT) {
      s.w[b] = 0;
      s.c[b] = 0;
    }
    __syncthreads();
    each<NT>(s, cand, x, n, T, [&](float y, int i) {
      if (!pred(y, i)) return;
      const uint32_t k = keyfn(y, i);
      if (hs < 32 && (k >> hs) != prefix) return;
      const uint32_t b = (k >> shift) & ((1u << width) - 1u);
      atomicAdd(&s.c[b], 1u);
      if (MASS) atomicAdd(&s.w[b], qmass(y, ymax));
    });
    __syncthreads();
    pick_bin<MASS>(s, above, t);
    prefix = (prefix << width) | s.sel_bin;
    above = s.sel_above;
    wsel = s.sel_w;
    csel = s.sel_c;
    __syncthreads();
  }
  return Sel{prefix, above, wsel, csel};
}

// index of the j-th (0-based) smallest index among the entries with pred(y, i) and okey(y) == key: a count select on (2^22 - 1 - i)
template <int NT, typename P>
__device__ __forceinline__ int nth_index(SampleLds& s, bool cand, const float* __restrict__ x, int n, float T, uint32_t key, unsigned int j, P pred) {
  const Sel r = select<NT, 22, false>(s, cand, x, n, T, 0.f, j, [&](float y, int i) { return okey(y) == key && pred(y, i); },
                                      [](float, int i) { return (uint32_t)((1 << 22) - 1 - i); });
  return (1 << 22) - 1 - (int)r.key;
}

template <int NT>
__device__ __forceinline__ float block_max(SampleLds& s, float m) {
  m = wave_max(m);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s.fred[threadIdx.x >> 6] = m;
  __syncthreads();
  float r = s.fred[0];
  for (int w = 1; w < NT / 64; ++w) r = fmaxf(r, s.fred[w]);
  return r;
}

struct SampleOut {
  const int* step;
  const float* u_override;
  unsigned long long* acc;
  int64_t* tok;
  int64_t* sidx;     // survivor dump (tests): the kept entries' indices and probabilities, no draw
  float* sprob;
  int scap;
  int* scount;
};

// the chain after the top-k cut: survivors = okey(y) >= Kk among the source (LDS candidates when cand); top-p, then the draw
template <int NT>
__device__ __forceinline__ void sample_tail(SampleLds& s, bool cand, const float* __restrict__ x, int n, const SampleParams* __restrict__ prm, float ymax,
                            uint32_t Kk, const SampleOut& o) {
  const int tid = threadIdx.x;
  const float T = prm->T, p = prm->p;
  auto all = [](float, int) { return true; };
  auto kf = [](float y, int) { return okey(y); };
  if (tid == 0) {
    s.sum = 0;
    s.found = 0x7fffffff;
  }
  __syncthreads();
  // Zs = mass of the survivors
  {
    unsigned long long z = 0;
    each<NT>(s, cand, x, n, T, [&](float y, int) {
      if (okey(y) >= Kk) z += qmass(y, ymax);
    });
    atomicAdd(&s.sum, z);
    __syncthreads();
  }
  const unsigned long long Zs = s.sum;
  // top-p: the cut entry is the first (descending) whose inclusive mass reaches p * Zs; ties at its key kept by ascending index
  uint32_t Kc = Kk;
  int ic = 0x7fffffff;
  unsigned long long Zk = Zs;
  if (p < 1.f) {
    const double tp = (double)p * (double)Zs;
    unsigned long long Tp = (unsigned long long)ceil(tp);
    if (Tp < 1) Tp = 1;
    if (Tp > Zs) Tp = Zs;
    const Sel r = select<NT, 32, true>(s, cand, x, n, T, ymax, Tp - 1, [&](float y, int) { return okey(y) >= Kk; }, kf);
    Kc = r.key;
    const unsigned long long mc = r.cnt ? r.w / r.cnt : 1;
    unsigned long long nc = mc ? (Tp - r.above + mc - 1) / mc : r.cnt;
    if (nc < 1) nc = 1;
    if (nc > r.cnt) nc = r.cnt;
    if (nc < r.cnt) ic = nth_index<NT>(s, cand, x, n, T, Kc, (unsigned)(nc - 1), all);
    Zk = r.above + nc * mc;
  }
  auto kept = [&](float y, int i) {
    const uint32_t kk = okey(y);
    return kk > Kc || (kk == Kc && i <= ic);
  };
  if (o.sidx) {
    const float inv = 1.0f / ldexpf((float)Zk, -40);
    each<NT>(s, cand, x, n, T, [&](float y, int i) {
      if (!kept(y, i)) return;
      const int slot = atomicAdd(o.scount, 1);
      if (slot < o.scap) {
        o.sidx[slot] = i;
        o.sprob[slot] = ldexpf((float)qmass(y, ymax), -40) * inv;
      }
    });
    return;
  }
  // the draw
  const float u = o.u_override ? *o.u_override : (float)(philox_x0(prm->seed, (uint32_t)*o.step) >> 8) * 0x1p-24f;
  unsigned long long td = (unsigned long long)floor((double)u * (double)Zk);
  if (td >= Zk) td = Zk - 1;
  const Sel r = select<NT, 32, true>(s, cand, x, n, T, ymax, td, kept, kf);
  const unsigned long long md = r.cnt ? r.w / r.cnt : 1;
  unsigned long long j = md ? (td - r.above) / md : 0;
  if (j >= r.cnt) j = r.cnt ? r.cnt - 1 : 0;
  int idx;
  if (r.cnt > 1) {
    idx = nth_index<NT>(s, cand, x, n, T, r.key, (unsigned)j, kept);
  } else {
    each<NT>(s, cand, x, n, T, [&](float y, int i) {
      if (okey(y) == r.key && kept(y, i)) atomicMin(&s.found, i);
    });
    __syncthreads();
    idx = s.found;
  }
  if (tid == 0 && o.acc) o.acc[0] = ((unsigned long long)r.key << 32) | (unsigned long long)(0xffffffffu - (uint32_t)idx);
  if (tid == 0 && o.tok) o.tok[0] = idx;
}

// the general route over the whole row
template <int NT>
__device__ __forceinline__ void sample_general(SampleLds& s, const float* __restrict__ x, int n, const SampleParams* __restrict__ prm, const SampleOut& o) {
  const int tid = threadIdx.x;
  const float T = prm->T;
  const int k = prm->k;
  __syncthreads();
  if (tid == 0) s.ncand = 0;
  float m = -INFINITY;
  each<NT>(s, false, x, n, T, [&](float y, int) { m = fmaxf(m, y); });
  const float ymax = block_max<NT>(s, m);
  auto all = [](float, int) { return true; };
  auto kf = [](float y, int) { return okey(y); };
  // top-k: Kk = the k-th largest key; survivors = key >= Kk
  uint32_t Kk = 0;
  unsigned int nsurv = (unsigned)n;
  if (k > 0 && k < n) {
    const Sel r = select<NT, 32, false>(s, false, x, n, T, ymax, (unsigned long long)(k - 1), all, kf);
    Kk = r.key;
    nsurv = (unsigned)(r.above + r.cnt);
  }
  // survivors that fit in LDS: compacted once, every later pass reads LDS
  const bool cand = nsurv <= (unsigned)CAP;
  if (cand) {
    each<NT>(s, false, x, n, T, [&](float y, int i) {
      if (okey(y) >= Kk) {
        const int slot = atomicAdd(&s.ncand, 1);
        if (slot < CAP) {
          s.cy[slot] = y;
          s.ci[slot] = i;
        }
      }
    });
    __syncthreads();
  }
  sample_tail<NT>(s, cand, x, n, prm, ymax, Kk, o);
}

__global__ __launch_bounds__(SB) void sample_kernel(const float* __restrict__ x, int n, const SampleParams* __restrict__ prm, SampleOut o) {
  __shared__ SampleLds s;
  sample_general<SB>(s, x, n, prm, o);
}

// row r of a batched step: its own step word, uniform, accumulator and token slot (the survivor dump is single-row only)
__device__ __forceinline__ SampleOut out_row(const SampleOut& o, int r) {
  return SampleOut{o.step + r, o.u_override ? o.u_override + r : nullptr, o.acc ? o.acc + r : nullptr, o.tok ? o.tok + r : nullptr,
                   nullptr, nullptr, 0, nullptr};
}

// the general route for B rows in one launch: workgroup r runs sample_kernel's body on row r (x + r * ldx) with parameter block prm[r]
__global__ __launch_bounds__(SB) void sample_rows_kernel(const float* __restrict__ x, long long ldx, int n, const SampleParams* __restrict__ prm,
                                                         SampleOut o) {
  __shared__ SampleLds s;
  const int r = blockIdx.y;
  sample_general<SB>(s, x + (long long)r * ldx, n, prm + r, out_row(o, r));
}

// The fast route.  ws: FAST_WS_INTS int32, zero-filled once (the ticket resets itself): [64][64] float y, [64][64] int index, [64][4] meta
// (stored count, the slice's 64th key Kloc, dropped-ties flag), ticket.
constexpr int FT = 256;            // threads per workgroup
constexpr int FPT = 8;             // entries per thread: a slice is at most 2048 entries
constexpr int FMAXWG = 64;
constexpr int FAST_WS_INTS = 2 * FMAXWG * 64 + FMAXWG * 4 + 64;

// the body of a fast-route workgroup: slice blockIdx.x of nb of the row x[n], workspace ws (the row's own)
__device__ __forceinline__ void sample_fast(SampleLds& s, const float* __restrict__ x, int n, const SampleParams* __restrict__ prm, const SampleOut& o,
                                            int* __restrict__ ws, int nb) {
  const int tid = threadIdx.x, b = blockIdx.x;
  float* wy = (float*)ws;
  int* wi = ws + FMAXWG * 64;
  int* meta = ws + 2 * FMAXWG * 64;
  int* ticket = meta + FMAXWG * 4;
  const float T = prm->T;
  const int k = prm->k;
  const int chunk = (n + nb - 1) / nb;
  const int lo = b * chunk, hi = min(n, lo + chunk);
  // 1. the slice in registers (four loads at a time in flight), its top 64 by value: a count select over the registers
  float y[FPT];
  uint32_t kv[FPT];
#pragma unroll
  for (int u = 0; u < FPT; ++u) {
    const int i = lo + tid + u * FT;
    y[u] = i < hi ? x[i] / T + 0.f : -INFINITY;     // (-0 counts as +0, as in each())
    kv[u] = i < hi ? okey(y[u]) : 0u;     // 0 is below every real key: out-of-slice entries never win a bin
  }
  const int len = hi > lo ? hi - lo : 0;
  uint32_t Kloc = 0;
  unsigned int above = 0;
  if (len > 64) {
    uint32_t prefix = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int shift = d == 0 ? 21 : d == 1 ? 10 : 0;
      const int width = d == 2 ? 10 : 11;
      const int hs = shift + width;
      for (int q = tid; q < NB; q += FT) s.c[q] = 0;
      __syncthreads();
#pragma unroll
      for (int u = 0; u < FPT; ++u)
        if (lo + tid + u * FT < hi && (hs >= 32 || (kv[u] >> hs) == prefix)) atomicAdd(&s.c[(kv[u] >> shift) & ((1u << width) - 1u)], 1u);
      __syncthreads();
      pick_bin<false>(s, above, 63);
      prefix = (prefix << width) | s.sel_bin;
      above = (unsigned)s.sel_above;
      __syncthreads();
    }
    Kloc = prefix;
  }
  // 2. keys > Kloc (above < 64 of them) first, then keys == Kloc while there is room; dropped ties are flagged
  if (tid == 0) {
    s.ncand = 0;
    s.neq = 0;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < FPT; ++u) {
    const int i = lo + tid + u * FT;
    if (i < hi && kv[u] > Kloc) {
      const int slot = atomicAdd(&s.ncand, 1);
      st_ag(wy + b * 64 + slot, y[u]);
      st_ag(wi + b * 64 + slot, i);
    }
  }
#pragma unroll
  for (int u = 0; u < FPT; ++u) {
    const int i = lo + tid + u * FT;
    if (i < hi && kv[u] == Kloc) {
      const int e = atomicAdd(&s.neq, 1);
      if ((int)above + e < 64) {
        st_ag(wy + b * 64 + above + e, y[u]);
        st_ag(wi + b * 64 + above + e, i);
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    st_ag(meta + b * 4 + 0, min(64, s.ncand + s.neq));      // (len <= 64: everything is above Kloc = 0)
    st_ag(meta + b * 4 + 1, (int)Kloc);
    st_ag(meta + b * 4 + 2, (int)(s.ncand + s.neq > 64));
  }
  // 3. arrival: the last workgroup merges (every lane's write-through stores have completed before the ticket)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) s.last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nb - 1;
  __syncthreads();
  if (!s.last) return;
  if (tid == 0) {
    st_ag(ticket, 0);                   // self-resetting for the next launch
    s.ncand = 0;
  }
  __syncthreads();
  for (int f = tid; f < nb * 64; f += FT) {
    const int wb = f >> 6, j = f & 63;
    if (j < ld_ag(meta + wb * 4)) {
      const int slot = atomicAdd(&s.ncand, 1);
      s.cy[slot] = ld_ag(wy + f);
      s.ci[slot] = ld_ag(wi + f);
    }
  }
  __syncthreads();
  float m = -INFINITY;
  each<FT>(s, true, x, n, T, [&](float yy, int) { m = fmaxf(m, yy); });
  const float ymax = block_max<FT>(s, m);
  bool ok = k >= 1 && k <= 64 && k < n;
  uint32_t Kk = 0;
  if (ok) {
    const Sel r = select<FT, 32, false>(s, true, x, n, T, ymax, (unsigned long long)(k - 1), [](float, int) { return true; },
                                        [](float yy, int) { return okey(yy); });
    Kk = r.key;
    // tie overflow: a slice dropped entries tied at its 64th value and that value is the threshold -> survivors may be missing
    if (tid == 0) s.found = 0;
    __syncthreads();
    if (tid < nb && ld_ag(meta + tid * 4 + 2) && (uint32_t)ld_ag(meta + tid * 4 + 1) >= Kk)
      atomicOr(&s.found, 1);
    __syncthreads();
    ok = s.found == 0;
    __syncthreads();
  }
  if (!ok) {
    sample_general<FT>(s, x, n, prm, o);
    return;
  }
  // 4. the survivors (key >= Kk: k plus ties) as packed (ordered value, ~index) keys; up to 256 of them are sorted in LDS and the rest of the
  //    chain is a prefix sum over them, more take the select-based tail
  if (tid == 0) s.neq = 0;
  __syncthreads();
  each<FT>(s, true, x, n, T, [&](float yy, int i) {
    if (okey(yy) >= Kk) {
      const int slot = atomicAdd(&s.neq, 1);
      if (slot < FT) s.sk[slot] = ((unsigned long long)okey(yy) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
    }
  });
  __syncthreads();
  const int nsv = s.neq;
  if (nsv > FT) {
    sample_tail<FT>(s, true, x, n, prm, ymax, Kk, o);
    return;
  }
  if (tid >= nsv) s.sk[tid] = 0ull;           // below every real key: sorts last, no mass
  for (int size = 2; size <= FT; size <<= 1) {  // bitonic sort, descending: value descending, ties by ascending index
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      const int j = tid ^ stride;
      if (j > tid) {
        const unsigned long long a = s.sk[tid], c = s.sk[j];
        if ((a < c) == ((tid & size) == 0)) {
          s.sk[tid] = c;
          s.sk[j] = a;
        }
      }
    }
  }
  __syncthreads();
  const unsigned long long key = s.sk[tid];
  const uint32_t ok32 = (uint32_t)(key >> 32);
  const float yk = __uint_as_float((ok32 & 0x80000000u) ? (ok32 & 0x7fffffffu) : ~ok32);
  const unsigned long long q = tid < nsv ? qmass(yk, ymax) : 0ull;
  // inclusive prefix sum of the masses (integer: exact, order-independent)
  unsigned long long* sc = s.w;
  int src = 0;
  sc[tid] = q;
  __syncthreads();
  for (int off = 1; off < FT; off <<= 1) {
    const unsigned long long v = sc[src + tid] + (tid >= off ? sc[src + tid - off] : 0ull);
    sc[(src ^ FT) + tid] = v;
    src ^= FT;
    __syncthreads();
  }
  const unsigned long long incl = sc[src + tid], prev = tid ? sc[src + tid - 1] : 0ull;
  const unsigned long long Zs = sc[src + nsv - 1];
  const float p = prm->p;
  unsigned long long Zk = Zs;
  if (p < 1.f) {    // the cut: the first entry whose inclusive mass reaches p * Zs (the select-based tail's rule)
    unsigned long long Tp = (unsigned long long)ceil((double)p * (double)Zs);
    if (Tp < 1) Tp = 1;
    if (Tp > Zs) Tp = Zs;
    if (tid < nsv && incl >= Tp && prev < Tp) s.found = tid;
    __syncthreads();
    Zk = sc[src + s.found];
  }
  const float u = o.u_override ? *o.u_override : (float)(philox_x0(prm->seed, (uint32_t)*o.step) >> 8) * 0x1p-24f;
  unsigned long long td = (unsigned long long)floor((double)u * (double)Zk);
  if (td >= Zk) td = Zk - 1;
  if (tid < nsv && incl > td && prev <= td) {       // exactly one entry: incl is non-decreasing and incl[last kept] = Zk > td
    if (o.acc) o.acc[0] = key;
    if (o.tok) o.tok[0] = (int64_t)(0xffffffffu - (uint32_t)key);
  }
}

__global__ __launch_bounds__(FT) void sample_fast_kernel(const float* __restrict__ x, int n, const SampleParams* __restrict__ prm, SampleOut o,
                                                         int* __restrict__ ws, int nb) {
  __shared__ SampleLds s;
  sample_fast(s, x, n, prm, o, ws, nb);
}

// the fast route for B rows in one launch: grid (nb, B); the workgroups of row r = blockIdx.y work in the row's own slice of the workspace
// (candidates, meta and a self-resetting ticket per row), so a row's last arriver merges that row alone and a tie overflow or a k outside
// 1..64 sends only that row to the general route
__global__ __launch_bounds__(FT) void sample_fast_rows_kernel(const float* __restrict__ x, long long ldx, int n, const SampleParams* __restrict__ prm,
                                                              SampleOut o, int* __restrict__ ws, int nb) {
  __shared__ SampleLds s;
  const int r = blockIdx.y;
  sample_fast(s, x + (long long)r * ldx, n, prm + r, out_row(o, r), ws + (long long)r * FAST_WS_INTS, nb);
}

__global__ __launch_bounds__(256) void philox_kernel(const unsigned long long* __restrict__ seeds, const int* __restrict__ steps, int n,
                                                     uint32_t* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = philox_x0(seeds[i], (uint32_t)steps[i]);
}

}  // namespace

extern "C" int vg_sample_workspace_ints(void) { return FAST_WS_INTS; }

extern "C" int vg_sample_partial(const float* x, int n, const void* params, const int* step, const float* u_override, uint64_t* acc,
                                 int64_t* tok, int* fast_ws, vg_stream_t stream) {
  VG_CHECK(x && params && step && (acc || tok) && n > 0 && n < (1 << 22), VG_ERR_ARG, "vg_sample_partial: bad args");
  VG_CHECK(!fast_ws || n <= FMAXWG * FT * FPT, VG_ERR_ARG, "vg_sample_partial: the fast route takes rows of at most 131072 entries");
  const SampleOut o{step, u_override, (unsigned long long*)acc, tok, nullptr, nullptr, 0, nullptr};
  if (fast_ws) {
    int nb = (n + FT * FPT - 1) / (FT * FPT);
    nb = nb < 1 ? 1 : nb;
    sample_fast_kernel<<<nb, FT, 0, (hipStream_t)stream>>>(x, n, (const SampleParams*)params, o, fast_ws, nb);
  } else {
    sample_kernel<<<1, SB, 0, (hipStream_t)stream>>>(x, n, (const SampleParams*)params, o);
  }
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_sample_partial_rows(const float* x, int64_t ldx, int n, int B, const void* params, const int* step, const float* u_override,
                                      uint64_t* acc, int64_t* tok, int* fast_ws, vg_stream_t stream) {
  VG_CHECK(x && params && step && (acc || tok) && n > 0 && n < (1 << 22) && B >= 1 && B <= 65535 && ldx >= n, VG_ERR_ARG,
           "vg_sample_partial_rows: bad args");
  VG_CHECK(!fast_ws || n <= FMAXWG * FT * FPT, VG_ERR_ARG, "vg_sample_partial_rows: the fast route takes rows of at most 131072 entries");
  const SampleOut o{step, u_override, (unsigned long long*)acc, tok, nullptr, nullptr, 0, nullptr};
  if (fast_ws) {
    int nb = (n + FT * FPT - 1) / (FT * FPT);
    nb = nb < 1 ? 1 : nb;
    sample_fast_rows_kernel<<<dim3(nb, B), FT, 0, (hipStream_t)stream>>>(x, (long long)ldx, n, (const SampleParams*)params, o, fast_ws, nb);
  } else {
    sample_rows_kernel<<<dim3(1, B), SB, 0, (hipStream_t)stream>>>(x, (long long)ldx, n, (const SampleParams*)params, o);
  }
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_sample_survivors(const float* x, int n, const void* params, int64_t* idx, float* prob, int cap, int* count,
                                   vg_stream_t stream) {
  VG_CHECK(x && params && idx && prob && count && n > 0 && n < (1 << 22) && cap > 0, VG_ERR_ARG, "vg_sample_survivors: bad args");
  const SampleOut o{nullptr, nullptr, nullptr, nullptr, idx, prob, cap, count};
  sample_kernel<<<1, SB, 0, (hipStream_t)stream>>>(x, n, (const SampleParams*)params, o);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_sample_philox(const uint64_t* seeds, const int* steps, int n, uint32_t* out, vg_stream_t stream) {
  VG_CHECK(seeds && steps && out && n >= 0, VG_ERR_ARG, "vg_sample_philox: bad args");
  if (n == 0) return VG_OK;
  philox_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>((const unsigned long long*)seeds, steps, n, out);
  VG_LAUNCH_CHECK();
  return VG_OK;
}
