// Per-token scores of the decode step: for B rows of fp32 logits, in ONE launch, the two largest entries, their margin
// and the log-probability of the token the step emitted, written into slot step[b] of the row's history — what a caller of
// generate(output_scores=True) reads, and what the top-2-margin policy of SURVEY section 7 needs.
//
// Contract (include/vg_kernels.h): top1 / top2 by value, ties to the lower index (the packed (ordered value bits, ~index) keys of vg_argmax:
// the largest and the second-largest KEY); margin = x[top1] - x[top2], one fp32 subtraction; logprob = log_softmax(x)[pick] on the raw logits.
//
// Geometry: argmax_stage1's — up to 64 workgroups of 256 threads per row, a slice of at most 2048 entries held in registers.  A workgroup
// leaves (largest key, second-largest key, mass) of its slice; mass is vg_sample.hip's fixed point, sum of floor(expf(x - m) * 2^40) in uint64
// with m the SLICE's maximum, so the integer sum does not depend on the order of its terms.  The last workgroup of a row to arrive
// (sample_fast's self-resetting ticket, write-through stores and agent-scope loads) merges the partials: the keys exactly, the masses as
// sum_w mass_w * exp(m_w - M) in float64, added in slice order by one thread.  The number of slices is a function of n alone, so row b of a
// B-row launch and a one-row launch on the same row add the same terms in the same order: bit-equal, and equal from launch to launch.
// n <= 2048 is one workgroup per row and needs no workspace.
#include "vg_common.h"
#include <math.h>

namespace {

constexpr int ST = 256;           // threads per workgroup
constexpr int SPT = 8;            // entries per thread held in registers: a slice of up to 2048 entries
constexpr int SMAXWG = 64;
constexpr int SC_WS_INTS = SMAXWG * 6 + 16;    // per slice {largest key, second key, mass} as uint64, then the ticket (padded to 64 bytes)

struct Top2 {
  unsigned long long a, b;        // a > b; 0 = none (below the key of every float)
};

__device__ __forceinline__ unsigned long long skey(float v, int i) {
  const uint32_t u = __float_as_uint(v);
  return ((unsigned long long)((u & 0x80000000u) ? ~u : (u | 0x80000000u)) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);   // amax_key
}
__device__ __forceinline__ float skey_value(unsigned long long k) {
  const uint32_t u = (uint32_t)(k >> 32);
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ long long skey_index(unsigned long long k) { return (long long)(0xffffffffu - (uint32_t)k); }

__device__ __forceinline__ void top2_push(Top2& t, unsigned long long k) {
  if (k > t.a) {
    t.b = t.a;
    t.a = k;
  } else if (k > t.b) {
    t.b = k;
  }
}
// the two largest keys of two disjoint sets
__device__ __forceinline__ Top2 top2_merge(const Top2& x, const Top2& y) {
  const unsigned long long hi = x.a > y.a ? x.a : y.a, lo = x.a > y.a ? y.a : x.a, sec = x.b > y.b ? x.b : y.b;
  return Top2{hi, lo > sec ? lo : sec};
}
__device__ __forceinline__ Top2 top2_wave(Top2 t) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t = top2_merge(t, Top2{__shfl_xor(t.a, o, 64), __shfl_xor(t.b, o, 64)});
  return t;
}
__device__ __forceinline__ unsigned long long smass(float v, float m) { return (unsigned long long)ldexpf(expf(v - m), 40); }   // vg_sample's qmass

// the hand-off of sample_fast (vg_sample.hip): write-through stores and sc1 loads at agent scope
template <typename V> __device__ __forceinline__ void st_ag(V* p, V v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename V> __device__ __forceinline__ V ld_ag(const V* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// grid (nb, B): workgroup (w, r) reduces slice w of row r; ws: the rows' workspaces, SC_WS_INTS int32 each (unused when nb == 1)
__global__ __launch_bounds__(ST) void token_scores_kernel(const float* __restrict__ x, long long ldx, int n, const unsigned long long* __restrict__ acc,
                                                          const int64_t* __restrict__ tok, const int* __restrict__ step, float* __restrict__ scores,
                                                          int64_t* __restrict__ top2, int cap, int* __restrict__ ws, int nb) {
  __shared__ unsigned long long s_a[ST / 64], s_b[ST / 64], s_q;
  __shared__ double s_z[SMAXWG];
  __shared__ int s_last;
  const int tid = threadIdx.x, w = blockIdx.x, r = blockIdx.y;
  const float* __restrict__ xr = x + (long long)r * ldx;
  const int chunk = (n + nb - 1) / nb;
  const int lo = w * chunk, hi = min(n, lo + chunk);
  // 1. the slice in registers (v + 0: -0 counts as +0, as a float comparison has it); its two largest keys
  float v[SPT];
  Top2 t{0ull, 0ull};
#pragma unroll
  for (int u = 0; u < SPT; ++u) {
    const int i = lo + tid + u * ST;
    v[u] = i < hi ? xr[i] + 0.f : -INFINITY;
  }
#pragma unroll
  for (int u = 0; u < SPT; ++u) {
    const int i = lo + tid + u * ST;
    if (i < hi) top2_push(t, skey(v[u], i));
  }
  for (int i = lo + tid + SPT * ST; i < hi; i += ST) top2_push(t, skey(xr[i] + 0.f, i));     // rows past 64 * 2048 entries: the rest from memory
  t = top2_wave(t);
  if ((tid & 63) == 0) {
    s_a[tid >> 6] = t.a;
    s_b[tid >> 6] = t.b;
  }
  if (tid == 0) s_q = 0ull;
  __syncthreads();
  t = Top2{s_a[0], s_b[0]};
#pragma unroll
  for (int k = 1; k < ST / 64; ++k) t = top2_merge(t, Top2{s_a[k], s_b[k]});
  // 2. the slice's mass relative to its own maximum: integer, so the sum is the same in any order
  unsigned long long q = 0ull;
  if (t.a) {
    const float m = skey_value(t.a);
#pragma unroll
    for (int u = 0; u < SPT; ++u) q += smass(v[u], m);        // (-inf beyond the slice: mass 0)
    for (int i = lo + tid + SPT * ST; i < hi; i += ST) q += smass(xr[i] + 0.f, m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  if ((tid & 63) == 0) atomicAdd(&s_q, q);
  __syncthreads();
  q = s_q;
  // 3. arrival: the row's last workgroup merges (one workgroup per row: nothing to hand over)
  unsigned long long* wp = (unsigned long long*)(ws + (long long)r * SC_WS_INTS);
  if (nb > 1) {
    int* ticket = ws + (long long)r * SC_WS_INTS + SMAXWG * 6;
    if (tid == 0) {
      st_ag(wp + 3 * w + 0, t.a);
      st_ag(wp + 3 * w + 1, t.b);
      st_ag(wp + 3 * w + 2, q);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the write-through stores have completed before the ticket
    __syncthreads();
    if (tid == 0) s_last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nb - 1;
    __syncthreads();
    if (!s_last) return;
    if (tid == 0) st_ag(ticket, 0);                         // self-resetting for the next launch
  }
  // 4. wave 0: lane l holds slice l's partial; the keys merge exactly, every mass is rescaled to the row's maximum in float64
  Top2 g{0ull, 0ull};
  if (tid < 64) {
    Top2 p{0ull, 0ull};
    unsigned long long pq = 0ull;
    if (tid < nb) {
      p = nb > 1 ? Top2{ld_ag(wp + 3 * tid + 0), ld_ag(wp + 3 * tid + 1)} : t;
      pq = nb > 1 ? ld_ag(wp + 3 * tid + 2) : q;
    }
    g = top2_wave(p);
    s_z[tid] = p.a ? (double)pq * exp((double)skey_value(p.a) - (double)skey_value(g.a)) : 0.0;
  }
  __syncthreads();
  if (tid != 0) return;
  const int j = step[r];
  if (j < 0 || j >= cap) return;
  double Z = 0.0;
  for (int k = 0; k < nb; ++k) Z += s_z[k];               // slice order, one thread: the same sum on every launch
  const float M = skey_value(g.a);
  const long long pick = tok ? (long long)tok[r] : skey_index(acc[r]);
  float lp = __uint_as_float(0x7fc00000u);
  if (pick >= 0 && pick < n) lp = (float)(((double)(xr[pick] + 0.f) - (double)M) - (log(Z) - 40.0 * 0.69314718055994530942));
  const long long o = ((long long)r * cap + j) * 2;
  scores[o] = lp;
  scores[o + 1] = M - skey_value(g.b);
  top2[o] = skey_index(g.a);
  top2[o + 1] = skey_index(g.b);
}

}  // namespace

extern "C" int vg_token_scores_workspace_ints(void) { return SC_WS_INTS; }

extern "C" int vg_token_scores_rows(const float* x, int64_t ldx, int n, int B, const uint64_t* acc, const int64_t* tok, const int* step,
                                    float* scores, int64_t* top2, int cap, int* ws, vg_stream_t stream) {
  VG_CHECK(x && scores && top2 && step, VG_ERR_ARG, "vg_token_scores_rows: x, scores, top2 and step must not be NULL");
  VG_CHECK((acc != nullptr) != (tok != nullptr), VG_ERR_ARG, "vg_token_scores_rows: the pick comes from acc or from tok, exactly one of them");
  VG_CHECK(n >= 2 && B >= 1 && B <= 16 && ldx >= n && cap > 0, VG_ERR_ARG, "vg_token_scores_rows: bad args (n >= 2, 1 <= B <= 16, ldx >= n, cap > 0)");
  int nb = (n + ST * SPT - 1) / (ST * SPT);
  nb = nb > SMAXWG ? SMAXWG : nb;
  VG_CHECK(nb == 1 || ws, VG_ERR_ARG, "vg_token_scores_rows: rows of more than 2048 entries need the workspace");
  token_scores_kernel<<<dim3(nb, B), ST, 0, (hipStream_t)stream>>>(x, (long long)ldx, n, (const unsigned long long*)acc, tok, step, scores, top2, cap,
                                                                  ws, nb);
  VG_LAUNCH_CHECK();
  return VG_OK;
}
