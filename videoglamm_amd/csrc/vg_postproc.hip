// Mask post-processing and evaluation counts on the device: integer / byte work, HBM-bound.
//
//   connected components : union-find over the pixel grid, all N images of a batch in ONE launch per pass (the
//                          reference's sam2/csrc/connected_components.cu:240-282 loops 6 launches per image).
//                          Passes: 64x64 tiles merged entirely in LDS (row runs from a ballot, one LDS atomicMin union
//                          per run contact, tile-local counts) -> unions across tile borders in global memory
//                          (3 % of the pixels) -> flatten + tile counts handed to the global roots -> finalize.
//                          The root of a component is its smallest pixel index, so labels are canonical:
//                          1 + min linear index.
//   remove_small_blobs   : 4-connectivity components smaller than min_size are cleared (R/eval_gcg_infer.py:20-29;
//                          skimage.morphology.remove_small_objects on a bool image).
//   fill_holes           : 8-connectivity background (score <= 0) components of area <= max_area get score 0.1
//                          (R/model/segment_anything_2/sam2/utils/misc.py:216-227).
//   mask_pair_counts     : |a & b|, |a | b| for every (prediction, ground truth) pair (R/eval_gcg_metrics.py:26-37,
//                          R/eval_referdavis_metrics.py:147-176).
//   boundary_counts      : the four integer counts of the boundary F-measure: seg2bmap of both masks, dilation by a
//                          disk, matches (R/eval_referdavis_metrics.py:194-305).
//   mask_boxes           : (xmin, ymin, xmax, ymax, area) of every mask of a batch in one pass over its bytes
//                          (masks_to_boxes, R/utils/grounding_utils/box_ops.py:118-142), and blob_boxes: the same table
//                          for the mask after remove_small_blobs, reduced on the finalize side of the union-find
//                          (the chain of R/eval_grounding.py:281-287).
//   mask_rle / rle_to_mask : COCO's uncompressed run-length code of every mask of a batch, in two phases (count, emit),
//                          and its inverse in gather form (mask_to_rle_pytorch / rle_to_mask,
//                          R/model/segment_anything_2/sam2/utils/amg.py:109-151).
#include "vg_common.h"

namespace {

struct CCArgs {
  const void* in;     // uint8 mask (foreground = nonzero) or fp32 scores (foreground = score <= 0)
  int32_t* L;         // parent links / labels          [N, H, W]
  int32_t* cnt;       // per-root pixel counts / areas  [N, H, W]
  void* out;          // finalize modes 1, 2
  int N, H, W, conn;
  int mode;           // finalize: 0 labels+areas, 1 remove small (uint8 out), 2 fill holes (fp32 out)
  int limit;          // min_size (mode 1) / max_area (mode 2)
};

template <int IN>
__device__ __forceinline__ bool cc_fg(const void* in, int64_t i) {
  if (IN == 0) return ((const uint8_t*)in)[i] != 0;
  return ((const float*)in)[i] <= 0.f;
}

// ---- pass 1: a 64x64 tile per workgroup, merged completely in LDS.  A wave owns 16 rows (lane = column), so the runs
// of a row come from one ballot and there are no seams inside a tile.  Out: L[p] = global index of the pixel's TILE root
// (trees of depth 1), cnt[tile root] = size of the tile component, 0 elsewhere.
__device__ __forceinline__ int lds_find(volatile int* l, int a) {
  int q;
  while ((q = l[a]) != a) a = q;
  return a;
}
__device__ __forceinline__ void lds_unite(int* l, int a, int b) {
  while (true) {
    a = lds_find(l, a);
    b = lds_find(l, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&l[a], b);
    if (old == a) return;
    a = old;
  }
}
__device__ __forceinline__ bool bit64(uint64_t m, int i) { return (m >> i) & 1; }

template <int IN>
__global__ __launch_bounds__(256) void cc_tile_kernel(CCArgs p) {
  __shared__ int lbl[64 * 64];
  __shared__ int cntl[64 * 64];
  __shared__ uint64_t rowmask[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + lane, y0 = blockIdx.y * 64;
  const int64_t base = (int64_t)blockIdx.z * p.H * p.W;
  uint64_t bits[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = wave + 4 * i, y = y0 + r;
    const bool fg = x < p.W && y < p.H && cc_fg<IN>(p.in, base + (int64_t)y * p.W + x);
    const uint64_t b = __ballot(fg);
    bits[i] = b;
    if (lane == 0) rowmask[r] = b;
    int v = -1;
    if (fg) {
      const uint64_t below = lane ? (~b & ((1ull << lane) - 1)) : 0ull;   // background lanes left of this one
      v = r * 64 + (below ? 64 - __clzll((long long)below) : 0);          // first pixel of this pixel's run
    }
    lbl[r * 64 + lane] = v;
    cntl[r * 64 + lane] = 0;
  }
  __syncthreads();
  // a vertical contact is united once per pair of touching runs: when the left neighbour touches the same upper run
  // (left && ul) it has made (or delegated further left) the union
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = wave + 4 * i, idx = r * 64 + lane;
    if (r == 0 || !bit64(bits[i], lane)) continue;
    const uint64_t um = rowmask[r - 1];
    const bool left = lane > 0 && bit64(bits[i], lane - 1);
    const bool ul = lane > 0 && bit64(um, lane - 1);
    if (bit64(um, lane)) {
      if (!(left && ul)) lds_unite(lbl, idx, idx - 64);
    } else if (p.conn == 8) {
      if (ul && !left) lds_unite(lbl, idx, idx - 65);
      if (lane < 63 && bit64(um, lane + 1)) lds_unite(lbl, idx, idx - 63);
    }
  }
  __syncthreads();
  int roots[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = wave + 4 * i;
    bool active = bit64(bits[i], lane);
    const int root = active ? lds_find(lbl, r * 64 + lane) : -1;
    roots[i] = root;
    uint64_t m;
    while ((m = __ballot(active)) != 0) {                  // one LDS atomic per (row, component)
      const int leader = __ffsll((long long)m) - 1;
      const int rr = __shfl(root, leader, 64);
      const bool same = active && root == rr;
      const uint64_t sm = __ballot(same);
      if (lane == leader) atomicAdd(&cntl[rr], (int)__popcll(sm));
      active = active && !same;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int r = wave + 4 * i, y = y0 + r;
    if (x >= p.W || y >= p.H) continue;
    const int64_t g = base + (int64_t)y * p.W + x;
    const int root = roots[i];
    p.L[g] = root < 0 ? -1 : (y0 + (root >> 6)) * p.W + blockIdx.x * 64 + (root & 63);
    p.cnt[g] = root == r * 64 + lane ? cntl[root] : 0;
  }
}

// ---- pass 2: unions across tile borders (global memory).  Links are only ever lowered (atomicMin), the atomic returns the
// true previous value and a failed attempt continues with it: a stale plain load (the XCD L2s are not coherent with
// each other inside a kernel) costs a retry, never a wrong union.  Path halving keeps the walks short.
__device__ __forceinline__ int cc_find(int32_t* L, int a) {
  int q;
  while ((q = L[a]) != a) {
    const int g = L[q];
    if (g != q) L[a] = g;       // benign race: any ancestor is a valid link
    a = q;
  }
  return a;
}
__device__ __forceinline__ int cc_find_ro(const int32_t* L, int a) {   // no halving: pass 3 stores final roots concurrently
  int q;
  while ((q = L[a]) != a) a = q;
  return a;
}
__device__ __forceinline__ void cc_unite(int32_t* L, int a, int b) {
  while (true) {
    a = cc_find(L, a);
    b = cc_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(192) void cc_border_kernel(CCArgs p) {
  const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;     // 0: top row, 1: left column, 2: right column
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 64, W = p.W, H = p.H;
  int32_t* L = p.L + (int64_t)blockIdx.z * H * W;
  const int x = role == 0 ? x0 + lane : role == 1 ? x0 : x0 + 63;
  const int y = role == 0 ? y0 : y0 + lane;
  if (x >= W || y >= H) return;
  const int pix = y * W + x;
  if (L[pix] < 0) return;
  if (role == 0) {
    if (y == 0) return;
    const bool left = x > 0 && L[pix - 1] >= 0;
    const bool ul = x > 0 && L[pix - W - 1] >= 0;
    if (L[pix - W] >= 0) {
      if (!(lane > 0 && left && ul)) cc_unite(L, pix, pix - W);
    } else if (p.conn == 8) {
      if (ul && !(lane > 0 && left)) cc_unite(L, pix, pix - W - 1);
      if (x < W - 1 && L[pix - W + 1] >= 0) cc_unite(L, pix, pix - W + 1);
    }
  } else if (role == 1) {
    if (x == 0) return;
    if (L[pix - 1] >= 0) cc_unite(L, pix, pix - 1);
    // the diagonal into the left tile; row 0 of the tile belongs to the top-row threads.  With the upper pixel set the
    // contact is implied (upper ~ its own left neighbour by this same rule or by the run)
    else if (p.conn == 8 && lane > 0 && L[pix - W] < 0 && L[pix - W - 1] >= 0) cc_unite(L, pix, pix - W - 1);
  } else {
    if (p.conn != 8 || lane == 0 || x >= W - 1) return;
    if (L[pix - W] < 0 && L[pix - W + 1] >= 0) cc_unite(L, pix, pix - W + 1);
  }
}

// ---- pass 3: every pixel takes the global root; every tile root hands its tile count to the global root, tile roots of
// one tile that share a global root combined in an LDS table first (same-address device atomics cost ~90 ns each).
__global__ __launch_bounds__(256) void cc_flatten_count_kernel(CCArgs p) {
  constexpr int SLOTS = 64;
  __shared__ int hkey[SLOTS], hval[SLOTS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + lane, y0 = blockIdx.y * 64;
  const int64_t base = (int64_t)blockIdx.z * p.H * p.W;
  int32_t* L = p.L + base;
  int32_t* cnt = p.cnt + base;
  if (threadIdx.x < SLOTS) { hkey[threadIdx.x] = -1; hval[threadIdx.x] = 0; }
  __syncthreads();
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int y = y0 + wave + 4 * i;
    if (x >= p.W || y >= p.H) continue;
    const int pix = y * p.W + x;
    const int t = L[pix];
    if (t < 0) continue;
    const int root = cc_find_ro(L, t);
    L[pix] = root;              // concurrent walkers through this pixel see its old parent or the root: both ancestors
    const int c = cnt[pix];
    if (c > 0 && root != pix) {           // a tile root that is not the global root
      int s = (root * 0x9E3779B1u) >> 26;   // 6 bits
      bool done = false;
      for (int probe = 0; probe < SLOTS && !done; ++probe, s = (s + 1) & (SLOTS - 1)) {
        const int k = atomicCAS(&hkey[s], -1, root);
        if (k == -1 || k == root) { atomicAdd(&hval[s], c); done = true; }
      }
      if (!done) atomicAdd(&cnt[root], c);
    }
  }
  __syncthreads();
  if (threadIdx.x < SLOTS && hkey[threadIdx.x] >= 0) atomicAdd(&cnt[hkey[threadIdx.x]], hval[threadIdx.x]);
}

// one wave = 64 consecutive pixels of one row; a workgroup = 4 rows
template <int IN>
__global__ __launch_bounds__(256) void cc_finalize_kernel(CCArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + lane, y = blockIdx.y * 4 + wave;
  if (x >= p.W || y >= p.H) return;
  const int64_t base = (int64_t)blockIdx.z * p.H * p.W;
  const int64_t i = base + y * p.W + x;
  const int root = p.L[i];
  const bool fg = root >= 0;
  const int area = fg ? p.cnt[base + root] : 0;
  if (p.mode == 0) {
    p.L[i] = fg ? root + 1 : 0;
    p.cnt[i] = area;        // a global root rewrites its own value; everyone else only reads global roots
  } else if (p.mode == 1) {
    ((uint8_t*)p.out)[i] = (fg && area >= p.limit) ? 1 : 0;
  } else {
    ((float*)p.out)[i] = (fg && area <= p.limit) ? 0.1f : ((const float*)p.in)[i];
  }
}

template <int IN>
int cc_run(const CCArgs& p, hipStream_t st) {
  const dim3 tiles((p.W + 63) / 64, (p.H + 63) / 64, p.N);
  cc_tile_kernel<IN><<<tiles, 256, 0, st>>>(p);
  if (tiles.x > 1 || tiles.y > 1) cc_border_kernel<<<tiles, 192, 0, st>>>(p);
  cc_flatten_count_kernel<<<tiles, 256, 0, st>>>(p);
  cc_finalize_kernel<IN><<<dim3((p.W + 63) / 64, (p.H + 3) / 4, p.N), 256, 0, st>>>(p);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

int cc_check(const void* in, const void* a, const void* b, int N, int H, int W, const char* who) {
  VG_CHECK(in && a && b, VG_ERR_ARG, "%s: null pointer", who);
  VG_CHECK(N > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) && N <= 65535, VG_ERR_ARG, "%s: bad shape N=%d H=%d W=%d", who, N, H, W);
  return VG_OK;
}

// ---------------------------------------------------------------------------------------------- pair counts
__device__ __forceinline__ uint32_t nz_bytes(uint32_t v) {   // 0x80 in every byte of v that is nonzero
  return (v | ((v & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;
}

__global__ __launch_bounds__(256) void pair_counts_kernel(const uint8_t* a, const uint8_t* b, unsigned long long* inter,
                                                          unsigned long long* uni, int G, int64_t L, int vec, int diag) {
  const int pair = blockIdx.y, pi = diag ? pair : pair / G, gi = diag ? pair : pair % G;
  const uint8_t* pa = a + (int64_t)pi * L;
  const uint8_t* pb = b + (int64_t)gi * L;
  unsigned ci = 0, cu = 0;       // a thread sees at most L / (gridDim.x * 256) * 16 < 2^32 pixels
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  if (vec) {
    const int64_t nw = L / 16;
    for (int64_t w = tid; w < nw; w += nth) {
      const u32x4_t va = __builtin_nontemporal_load((const u32x4_t*)pa + w);
      const u32x4_t vb = __builtin_nontemporal_load((const u32x4_t*)pb + w);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t na = nz_bytes(va[k]), nb = nz_bytes(vb[k]);
        ci += __popc(na & nb);
        cu += __popc(na | nb);
      }
    }
    for (int64_t i = nw * 16 + tid; i < L; i += nth) {
      const bool x = pa[i] != 0, y = pb[i] != 0;
      ci += x && y;
      cu += x || y;
    }
  } else {
    for (int64_t i = tid; i < L; i += nth) {
      const bool x = pa[i] != 0, y = pb[i] != 0;
      ci += x && y;
      cu += x || y;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ci += __shfl_xor(ci, o, 64);
    cu += __shfl_xor(cu, o, 64);
  }
  // one atomic pair per workgroup: same-address device atomics serialise at ~90 ns each on this part
  __shared__ unsigned red[2][4];
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = ci; red[1][threadIdx.x >> 6] = cu; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long ti = (unsigned long long)red[0][0] + red[0][1] + red[0][2] + red[0][3];
    const unsigned long long tu = (unsigned long long)red[1][0] + red[1][1] + red[1][2] + red[1][3];
    if (ti) atomicAdd(&inter[pair], ti);
    if (tu) atomicAdd(&uni[pair], tu);
  }
}

// ---------------------------------------------------------------------------------------------- boundary F counts
// 64x64 output pixels per workgroup, everything as ROW BITMASKS in LDS (a row of the 64 + 2r (+1) wide halo tile is
// 128 bits): the masks are staged with one ballot per 64 columns, the boundary stencil of _seg2bmap is three shifts and
// xors per row, and the disk test of a pixel is one shifted window compare per disk row (2r + 1 of them instead of
// ~3r^2 byte reads).  Only pixels that lie on one of the two boundaries search at all.
struct Bits128 {
  uint64_t lo, hi;
};
__device__ __forceinline__ Bits128 shr1(Bits128 v) { return {(v.lo >> 1) | (v.hi << 63), v.hi >> 1}; }
__device__ __forceinline__ uint64_t window64(Bits128 v, int sh) {   // bits [sh, sh + 63] of v, 0 <= sh < 128
  if (sh >= 64) return v.hi >> (sh - 64);
  return sh ? (v.lo >> sh) | (v.hi << (64 - sh)) : v.lo;
}

__global__ __launch_bounds__(256) void boundary_counts_kernel(const uint8_t* fg, const uint8_t* gt, unsigned long long* out,
                                                              int H, int W, int r) {
  __shared__ Bits128 seg[2][128];     // [mask][row]: rows y0 .. y0 + BW (one extra row for the stencil)
  __shared__ Bits128 bnd[2][128];     // boundary maps, rows y0 .. y0 + BW - 1
  __shared__ int hw[64];              // half-width of the disk row dy = i - r
  __shared__ unsigned red[4][4];
  __shared__ uint16_t list[64 * 64];  // compacted boundary pixels: lx | ly << 7 | on-fg << 14 | on-gt << 15
  __shared__ int nlist;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) nlist = 0;
  const int BW = 64 + 2 * r, SW = BW + 1;
  const int x0 = blockIdx.x * 64 - r, y0 = blockIdx.y * 64 - r;
  const int64_t base = (int64_t)blockIdx.z * H * W;
  for (int j0 = wave * 8; j0 < 4 * SW; j0 += 32) {           // jobs = (mask, row, 64-column half); 8 loads in flight per lane
    bool v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int job = j0 + k, m = job & 1, half = (job >> 1) & 1, row = job >> 2;
      const int yy = y0 + row, xx = x0 + half * 64 + lane;
      const uint8_t* src = m ? gt : fg;
      v[k] = job < 4 * SW && yy >= 0 && yy < H && xx >= 0 && xx < W && (half * 64 + lane) < SW && src[base + (int64_t)yy * W + xx] != 0;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int job = j0 + k, m = job & 1, half = (job >> 1) & 1, row = job >> 2;
      const uint64_t b = __ballot(v[k]);
      if (lane == 0 && job < 4 * SW) { if (half) seg[m][row].hi = b; else seg[m][row].lo = b; }
    }
  }
  if (tid <= 2 * r) {
    const int dy = tid - r;
    int w = 0;
    while ((w + 1) * (w + 1) + dy * dy <= r * r) ++w;
    hw[tid] = w;
  }
  __syncthreads();
  if (tid < 2 * BW) {                                          // one thread per (mask, row) of the boundary maps
    const int m = tid & 1, row = tid >> 1, yy = y0 + row;
    Bits128 b = {0, 0};
    if (yy >= 0 && yy < H) {
      const Bits128 S = seg[m][row], N = seg[m][row + 1];      // N is all zero below the image
      const Bits128 e = shr1(S), se = shr1(N);
      if (yy == H - 1) b = {S.lo ^ e.lo, S.hi ^ e.hi};
      else b = {(S.lo ^ e.lo) | (S.lo ^ N.lo) | (S.lo ^ se.lo), (S.hi ^ e.hi) | (S.hi ^ N.hi) | (S.hi ^ se.hi)};
      const int lc = W - 1 - x0;                               // the image's last column: seg ^ south, corner 0
      if (lc >= 0 && lc < 128) {
        const uint64_t bit = 1ull << (lc & 63);
        const uint64_t v = yy == H - 1 ? 0ull : ((lc < 64 ? S.lo ^ N.lo : S.hi ^ N.hi) & bit);
        if (lc < 64) b.lo = (b.lo & ~bit) | v; else b.hi = (b.hi & ~bit) | v;
      }
      // keep only columns inside the image: bits [max(0, -x0), min(127, W - 1 - x0)]
      const int c0 = x0 < 0 ? -x0 : 0, c1 = lc < 127 ? lc : 127;
      Bits128 keep = {0, 0};
      if (c1 >= c0) {
        const uint64_t lo_m = c0 < 64 ? (~0ull << c0) : 0ull, hi_m = c0 < 64 ? ~0ull : (~0ull << (c0 - 64));
        const uint64_t lo_M = c1 < 64 ? (~0ull >> (63 - c1)) : ~0ull, hi_M = c1 < 64 ? 0ull : (~0ull >> (127 - c1));
        keep = {lo_m & lo_M, hi_m & hi_M};
      }
      b = {b.lo & keep.lo, b.hi & keep.hi};
    }
    bnd[m][row] = b;
  }
  __syncthreads();
  // boundary pixels are a few per cent of the tile: compact them into a list first so that the disk search runs with
  // full waves (a wave that holds a single boundary pixel would otherwise walk all 2r + 1 disk rows for it)
  unsigned nf = 0, ng = 0, mf = 0, mg = 0;
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const int ly = r + wave + 4 * i, lx = r + lane;
    const bool f = (window64(bnd[0][ly], lx) & 1) != 0, g = (window64(bnd[1][ly], lx) & 1) != 0;
    const uint64_t m = __ballot(f || g);
    if (m == 0) continue;                                   // wave-uniform
    int slot = 0;
    if (lane == 0) slot = atomicAdd(&nlist, (int)__popcll(m));
    slot = __shfl(slot, 0, 64) + (int)__popcll(m & ((1ull << lane) - 1));
    if (f || g) list[slot] = (uint16_t)(lx | (ly << 7) | (f ? 0x4000 : 0) | (g ? 0x8000 : 0));
    nf += f;
    ng += g;
  }
  __syncthreads();
  const int n = nlist;
  for (int e = tid; e < n; e += 256) {
    const int v = list[e], lx = v & 127, ly = (v >> 7) & 127;
    const bool f = v & 0x4000, g = v & 0x8000;
    bool df = false, dg = false;          // the OTHER map's boundary within the disk of this pixel
    for (int dy = -r; dy <= r; ++dy) {
      const int w = hw[dy + r];
      const uint64_t win = w >= 31 ? ~0ull >> 1 : (1ull << (2 * w + 1)) - 1;    // 2w + 1 <= 63 bits
      if (g) df |= (window64(bnd[0][ly + dy], lx - w) & win) != 0;
      if (f) dg |= (window64(bnd[1][ly + dy], lx - w) & win) != 0;
    }
    mf += f && dg;      // fg boundary pixels matched by the dilated gt boundary
    mg += g && df;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nf += __shfl_xor(nf, o, 64);
    ng += __shfl_xor(ng, o, 64);
    mf += __shfl_xor(mf, o, 64);
    mg += __shfl_xor(mg, o, 64);
  }
  if (lane == 0) { red[0][wave] = nf; red[1][wave] = ng; red[2][wave] = mf; red[3][wave] = mg; }
  __syncthreads();
  if (tid < 4) {                          // one atomic per counter per workgroup
    const unsigned t = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
    if (t) atomicAdd(out + (int64_t)blockIdx.z * 4 + tid, (unsigned long long)t);
  }
}

// ---------------------------------------------------------------------------------------------- boxes from masks
// out[n] = (xmin, ymin, xmax, ymax, area), maxima inclusive; (W, H, -1, -1, 0) for an empty mask: the values the
// reductions start from, written by box_init_kernel in front of every reducing launch (no caller-side memset).
__global__ __launch_bounds__(256) void box_init_kernel(int32_t* out, int N, int H, int W) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  int32_t* o = out + (int64_t)n * 5;
  o[0] = W; o[1] = H; o[2] = -1; o[3] = -1; o[4] = 0;
}

// registers -> wave -> LDS -> one set of five device atomics per workgroup of WAVES waves, none from a workgroup without
// foreground.  Integer min / max / sum: any arrival order gives the same table.  Every thread of the workgroup calls it.
// (Tried: sending a bound only when it beats the value the table holds at that moment.  The extra read made every
// shape slower, 30 -> 54 us on 32 x 1024^2 at 64 workgroups per mask; few workgroups per mask is what pays, box_chunks.)
template <int WAVES>
__device__ __forceinline__ void box_commit(int xmin, int ymin, int xmax, int ymax, int cnt, int32_t* o) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    xmin = min(xmin, __shfl_xor(xmin, s, 64));
    ymin = min(ymin, __shfl_xor(ymin, s, 64));
    xmax = max(xmax, __shfl_xor(xmax, s, 64));
    ymax = max(ymax, __shfl_xor(ymax, s, 64));
    cnt += __shfl_xor(cnt, s, 64);
  }
  __shared__ int red[5][WAVES];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wave] = xmin; red[1][wave] = ymin; red[2][wave] = xmax; red[3][wave] = ymax; red[4][wave] = cnt; }
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= 5) return;
  int lo = red[t][0], hi = lo, sum = lo, area = red[4][0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) {
    const int v = red[t][w];
    lo = min(lo, v); hi = max(hi, v); sum += v; area += red[4][w];
  }
  if (area == 0) return;
  if (t < 2) atomicMin(o + t, lo);
  else if (t < 4) atomicMax(o + t, hi);
  else atomicAdd(o + 4, sum);
}

// One pass over the bytes, 1 B per pixel.  A mask is L = H * W bytes from p = mask + n * L, aligned to nothing when
// W % 16 != 0 or the base is a view: `head` bytes up to the first 16-byte boundary and the < 16 bytes behind the last
// whole word go through the byte path (workgroup 0 of the mask), the words between them are 16-byte loads.  Rows are
// y = index / W, monotone in the index, so ymin / ymax come from the smallest / largest foreground INDEX with one
// division per thread at the end; the column of a word's first byte is carried along the thread's stride (x0 += step
// mod W) and not divided out per word.  A word that lies inside one row gives its first and last foreground byte to
// xmin / xmax; a word that straddles a row end (every word when W < 16) walks its 16 bytes with a wrapping column.
__global__ __launch_bounds__(256) void mask_boxes_kernel(const uint8_t* mask, int32_t* out, int H, int W, int step) {
  const int n = blockIdx.y, L = H * W;
  const uint8_t* p = mask + (int64_t)n * L;
  const int head = min(L, (int)((16 - ((uintptr_t)p & 15)) & 15));
  const int nw = (L - head) >> 4;
  const int tid = blockIdx.x * 256 + threadIdx.x, nth = gridDim.x * 256;
  int xmin = W, xmax = -1, imin = 0x7fffffff, imax = -1, cnt = 0;
  if (tid < nw) {
    const u32x4_t* pw = (const u32x4_t*)(p + head);
    int x0 = (int)((unsigned)(head + 16 * tid) % (unsigned)W);
    for (int w = tid; w < nw; w += nth) {
      const u32x4_t v = __builtin_nontemporal_load(pw + w);
      if ((v[0] | v[1] | v[2] | v[3]) != 0) {
        const uint64_t lo = nz_bytes(v[0]) | ((uint64_t)nz_bytes(v[1]) << 32), hi = nz_bytes(v[2]) | ((uint64_t)nz_bytes(v[3]) << 32);
        const int first = lo ? (__ffsll((long long)lo) - 1) >> 3 : 8 + ((__ffsll((long long)hi) - 1) >> 3);
        const int last = hi ? 8 + ((63 - __clzll((long long)hi)) >> 3) : (63 - __clzll((long long)lo)) >> 3;
        const int o = head + 16 * w;
        cnt += __popcll(lo) + __popcll(hi);
        imin = min(imin, o + first);
        imax = max(imax, o + last);
        if (x0 + 15 < W) {
          xmin = min(xmin, x0 + first);
          xmax = max(xmax, x0 + last);
        } else {
          int x = x0;
          for (int k = 0; k < 16; ++k) {
            if (((k < 8 ? lo : hi) >> (8 * (k & 7) + 7)) & 1) { xmin = min(xmin, x); xmax = max(xmax, x); }
            if (++x == W) x = 0;
          }
        }
      }
      x0 += step;                 // step = (16 * nth) % W
      if (x0 >= W) x0 -= W;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 32) {           // the unaligned ends: at most 15 bytes each
    const int tail0 = head + 16 * nw;
    const int i = threadIdx.x < 16 ? threadIdx.x : tail0 + threadIdx.x - 16;
    if ((threadIdx.x < 16 ? i < head : i < L) && p[i] != 0) {
      const int x = (int)((unsigned)i % (unsigned)W);
      xmin = min(xmin, x); xmax = max(xmax, x); imin = min(imin, i); imax = max(imax, i); ++cnt;
    }
  }
  const int ymin = cnt ? (int)((unsigned)imin / (unsigned)W) : H, ymax = cnt ? (int)((unsigned)imax / (unsigned)W) : -1;
  box_commit<4>(xmin, ymin, xmax, ymax, cnt, out + (int64_t)n * 5);
}

// The finalize side of vg_blob_boxes: after the three union-find passes L[p] is the pixel's global root (-1 on
// background) and cnt[root] the component's area.  A workgroup takes a band of rows of one image (wave = row, lanes
// stride the columns), keeps the pixels of components with area >= limit, reduces their box, and writes the filtered
// mask on the way when asked to: cc_finalize_kernel mode 1 and mask_boxes_kernel in one read of the labels.
// 16 waves per workgroup: the area gather (cnt[root]) wants as many pixels in flight as cc_finalize_kernel's one pixel
// per thread gives, while the atomics want few workgroups per mask.
__global__ __launch_bounds__(1024) void cc_boxes_kernel(CCArgs p, int32_t* boxes, int rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.y * p.H * p.W;
  const int32_t* L = p.L + base;
  const int32_t* cnt = p.cnt + base;
  uint8_t* om = p.out ? (uint8_t*)p.out + base : nullptr;
  const int y0 = blockIdx.x * rows, y1 = min(p.H, y0 + rows);
  int xmin = p.W, ymin = p.H, xmax = -1, ymax = -1, area = 0;
  for (int y = y0 + wave; y < y1; y += 16) {
#pragma unroll 4
    for (int x = lane; x < p.W; x += 64) {
      const int i = y * p.W + x;
      const int root = L[i];
      const bool keep = root >= 0 && cnt[root] >= p.limit;
      if (om) om[i] = keep ? 1 : 0;
      if (keep) {
        xmin = min(xmin, x); xmax = max(xmax, x); ymin = min(ymin, y); ymax = max(ymax, y); ++area;
      }
    }
  }
  box_commit<16>(xmin, ymin, xmax, ymax, area, boxes + (int64_t)blockIdx.y * 5);
}

// ---------------------------------------------------------------------------------------------- class counts from logits
// The validator's intersectionAndUnionGPU(logit > 0, target, K = 2, ignore_index) (R/utils/utils.py:78-90) for all N masks
// of a call in one pass: 4 or 2 bytes of logit and 1 byte of target per pixel.  A thread takes groups of 16 pixels: the
// logits in 16-byte loads from the first 16-byte boundary of the mask's logits on (`head` pixels in front of it and the
// < 16 behind the last whole group go pixel by pixel, workgroup 0 of the mask), the 16 target bytes in one load at
// whatever alignment that leaves them.  Everything is counted on byte masks (0x80 per pixel of a target dword).
//
// "logit > 0" is decided on the BITS: positive, not zero, not NaN <=> bits - 1 < 0x7f800000 (0x7f80 for bf16) as unsigned.
// No floating-point compare, so the smallest denormal is class 1 whatever the kernel's denormal mode is.
__device__ __forceinline__ bool lcc_pos(float v) { return __float_as_uint(v) - 1u < 0x7f800000u; }
__device__ __forceinline__ bool lcc_pos(bf16_t v) { return (uint32_t)v - 1u < 0x7f80u; }

struct LccCounts {
  uint32_t nv, o1, t0, t1, i0, i1;      // not ignored; of those: class 1, target 0, target 1, target 0 & class 0, target 1 & class 1
};

// v: four target bytes, P: 0x80 in the byte of every pixel of class 1, ign4: the ignore label in all four bytes
__device__ __forceinline__ void lcc_count4(LccCounts& c, uint32_t v, uint32_t P, uint32_t ign4) {
  const uint32_t V = nz_bytes(v ^ ign4);
  const uint32_t Z = ~nz_bytes(v) & V, O = ~nz_bytes(v ^ 0x01010101u) & V;
  c.nv += __popc(V);
  c.o1 += __popc(V & P);
  c.t0 += __popc(Z);
  c.t1 += __popc(O);
  c.i0 += __popc(Z & ~P);
  c.i1 += __popc(O & P);
}

template <typename T>
__global__ __launch_bounds__(256) void logit_class_counts_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target,
                                                                 unsigned long long* __restrict__ out, int64_t L, uint32_t ign) {
  constexpr int PER = 16 / sizeof(T);       // logits per 16-byte load: 4 (fp32) or 8 (bf16)
  const int n = blockIdx.y;
  const T* pl = logits + (int64_t)n * L;
  const uint8_t* pt = target + (int64_t)n * L;
  const int64_t head = min(L, (int64_t)(((16 - ((uintptr_t)pl & 15)) & 15) / sizeof(T)));
  const int64_t nw = (L - head) >> 4;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
  const uint32_t ign4 = ign * 0x01010101u;
  LccCounts c = {0, 0, 0, 0, 0, 0};       // a thread sees fewer than 2^32 pixels: L < 2^40 and >= 16 workgroups per mask of that size
  for (int64_t w = tid; w < nw; w += nth) {
    const int64_t i = head + 16 * w;
    u32x4_t lv[16 / PER], tv;
#pragma unroll
    for (int k = 0; k < 16 / PER; ++k) lv[k] = __builtin_nontemporal_load((const u32x4_t*)(pl + i) + k);
    __builtin_memcpy(&tv, pt + i, 16);
#pragma unroll
    for (int d = 0; d < 4; ++d) {           // target dword d = pixels 4 d .. 4 d + 3
      uint32_t P = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int e = 4 * d + b;
        bool pos;
        if constexpr (sizeof(T) == 4) pos = lv[e / 4][e % 4] - 1u < 0x7f800000u;
        else pos = ((lv[e / 8][(e % 8) / 2] >> (16 * (e & 1))) & 0xffffu) - 1u < 0x7f80u;
        P |= pos ? 0x80u << (8 * b) : 0u;
      }
      lcc_count4(c, tv[d], P, ign4);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 32) {           // the ends: at most 15 pixels each
    const int64_t tail0 = head + 16 * nw;
    const int64_t i = threadIdx.x < 16 ? threadIdx.x : tail0 + threadIdx.x - 16;
    if (threadIdx.x < 16 ? i < head : i < L) lcc_count4(c, pt[i] | (ign4 & 0xffffff00u), lcc_pos(pl[i]) ? 0x80u : 0u, ign4);
  }
  // registers -> wave -> LDS -> at most six 64-bit device atomics per workgroup, none for a zero.  Integer sums: any
  // arrival order gives the same table.
  unsigned long long v[6] = {(unsigned long long)c.i0, c.i1, (unsigned long long)c.nv - c.o1, c.o1, c.t0, c.t1};
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v[k] += __shfl_xor(v[k], s, 64);
  __shared__ unsigned long long red[6][4];
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) red[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const unsigned long long t = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    if (t) atomicAdd(out + (int64_t)n * 6 + threadIdx.x, t);
  }
}

int box_init(int32_t* out, int N, int H, int W, hipStream_t st) {
  box_init_kernel<<<(N + 255) / 256, 256, 0, st>>>(out, N, H, W);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

// ---------------------------------------------------------------------------------------------- run-length codes
// COCO's uncompressed RLE in the form of mask_to_rle_pytorch (R/model/segment_anything_2/sam2/utils/amg.py:109-137): the
// pixels of a mask in COLUMN-major order j = x * H + y, a count for every run, a leading 0 when pixel 0 is foreground.
// The mask is row-major, so a lane owns RLE_G adjacent columns (one dword of every row) and walks down the rows: a wave
// reads 256 contiguous bytes per row, and a column's state (previous bit, count / write index, last transition) stays in
// registers.  A column is cut into S = ceil(H / R) segments of R rows (rle_rows) so that a 1024-row mask is walked by 16
// lanes per column group and not by one; segment s of column x is unit u = x * S + s, and the units in this order cover
// the pixels in the code's order.  Unit u owns the transitions at its own pixels: those inside it and the one at its
// first pixel against the pixel before it, which is the LAST pixel of unit u - 1 (the row above, or, for s = 0, the
// last pixel of column x - 1: the comparison runs across column ends).
//
// ws_cols: int32 [N, 4, U], U = W * S.  After rle_count_kernel: [0] transitions inside the unit, [1] the position j of
// the last of them (-1: none), [2] bit 0 = first pixel, bit 1 = last pixel.  rle_scan_kernel (one workgroup per mask,
// its own launch: nothing waits on another workgroup) turns [0] into the exclusive scan of the units' transition counts
// (the unit's write offset), [1] into the inclusive max-scan "last transition at or before this unit's end" (0: none;
// unit u starts its first run at [1][u - 1] without seeing another unit's pixels), and writes [3] = 1 where the unit's
// first pixel differs from the one before it.  Every entry is rewritten by every call: no state survives.
constexpr int RLE_G = 4;

// rows per column segment: 64, more only where the grid's y extent (65535) asks for it
inline int rle_rows(int H) { return max(64, (H + 65534) / 65535); }

// the foreground bits of w <= RLE_G adjacent pixels of a row (bit k = pixel k).  FULL: one dword load at whatever
// alignment the row has (gfx950 takes unaligned global dwords; hipcc emits global_load_dword for it); otherwise the
// last lane group of a row whose W is no multiple of RLE_G, byte by byte and never past the row's end.
template <bool FULL>
__device__ __forceinline__ uint32_t rle_row_bits(const uint8_t* row, int w) {
  uint32_t v = 0;
  if (FULL) {
    __builtin_memcpy(&v, row, 4);
  } else {
    for (int k = 0; k < w; ++k) v |= (uint32_t)row[k] << (8 * k);
  }
  const uint32_t z = nz_bytes(v) >> 7;
  return (z | (z >> 7) | (z >> 14) | (z >> 21)) & 15u;
}

// f(y, bits) for the rows y0 + 1 .. y1 - 1 of the lane's columns, in order (p: the lane's first column in row 0)
template <class F>
__device__ __forceinline__ void rle_walk(const uint8_t* p, int y0, int y1, int W, int w, F&& f) {
  if (w == RLE_G) {
#pragma unroll 8
    for (int y = y0 + 1; y < y1; ++y) f(y, rle_row_bits<true>(p + (int64_t)y * W, w));
  } else {
    for (int y = y0 + 1; y < y1; ++y) f(y, rle_row_bits<false>(p + (int64_t)y * W, w));
  }
}

// grid (lane groups of 64, S, N)
__global__ __launch_bounds__(64) void rle_count_kernel(const uint8_t* __restrict__ mask, int32_t* __restrict__ ws, int H, int W, int R) {
  const int n = blockIdx.z, seg = blockIdx.y, S = gridDim.y, x0 = (blockIdx.x * 64 + threadIdx.x) * RLE_G;
  if (x0 >= W) return;
  const int w = min(RLE_G, W - x0), y0 = seg * R, y1 = min(H, y0 + R), U = W * S;
  const uint8_t* p = mask + (int64_t)n * H * W + x0;
  int32_t* c = ws + (int64_t)n * 4 * U;
  const uint32_t first = w == RLE_G ? rle_row_bits<true>(p + (int64_t)y0 * W, w) : rle_row_bits<false>(p + (int64_t)y0 * W, w);
  uint32_t prev = first;
  int cnt[RLE_G], last[RLE_G];
#pragma unroll
  for (int k = 0; k < RLE_G; ++k) { cnt[k] = 0; last[k] = -1; }
  rle_walk(p, y0, y1, W, w, [&](int y, uint32_t b) {
    const uint32_t d = b ^ prev;
    prev = b;
#pragma unroll
    for (int k = 0; k < RLE_G; ++k)
      if ((d >> k) & 1) { ++cnt[k]; last[k] = y; }
  });
#pragma unroll
  for (int k = 0; k < RLE_G; ++k) {
    if (k >= w) break;
    const int x = x0 + k, u = x * S + seg;
    c[u] = cnt[k];
    c[U + u] = last[k] < 0 ? -1 : x * H + last[k];
    c[2 * U + u] = (int)(((first >> k) & 1) | (((prev >> k) & 1) << 1));
  }
}

// inclusive scans over the 1024 values of a workgroup: sum and max at once.  wsum / wmax: 16 words of LDS each.
__device__ __forceinline__ void rle_block_scan(int& s, int& m, int& total_s, int& total_m, int* wsum, int* wmax) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(s, o, 64), b = __shfl_up(m, o, 64);
    if (lane >= o) { s += a; m = max(m, b); }
  }
  if (lane == 63) { wsum[wave] = s; wmax[wave] = m; }
  __syncthreads();
  total_s = 0; total_m = 0;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    if (v < wave) { s += wsum[v]; m = max(m, wmax[v]); }
    total_s += wsum[v]; total_m = max(total_m, wmax[v]);
  }
  __syncthreads();
}

__global__ __launch_bounds__(1024) void rle_scan_kernel(int32_t* ws, int32_t* n_runs, int H, int W, int S, int R) {
  __shared__ int wsum[16], wmax[16];
  const int n = blockIdx.x, t = threadIdx.x, U = W * S;
  int32_t* c = ws + (int64_t)n * 4 * U;
  int carry_s = 0, carry_m = 0;
  for (int base = 0; base < U; base += 1024) {
    const int u = base + t;
    int own = 0, m = 0;
    if (u < U) {
      const int flag = u > 0 && (c[2 * U + u] & 1) != ((c[2 * U + u - 1] >> 1) & 1);
      const int lp = c[U + u];
      own = c[u] + flag;
      m = lp >= 0 ? lp : (flag ? (u / S) * H + (u % S) * R : 0);       // the unit's first pixel
      c[3 * U + u] = flag;
    }
    int s = own, ts, tm;
    rle_block_scan(s, m, ts, tm, wsum, wmax);
    if (u < U) {
      c[u] = carry_s + s - own;
      c[U + u] = max(carry_m, m);
    }
    carry_s += ts;
    carry_m = max(carry_m, tm);
  }
  if (t == 0) n_runs[n] = carry_s + 1 + (c[2 * U] & 1);
}

__global__ __launch_bounds__(64) void rle_emit_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ ws,
                                                      const int64_t* __restrict__ offsets, int32_t* __restrict__ counts, int H, int W, int R) {
  const int n = blockIdx.z, seg = blockIdx.y, S = gridDim.y, x0 = (blockIdx.x * 64 + threadIdx.x) * RLE_G;
  if (x0 >= W) return;
  const int64_t lo = offsets[n], hi = offsets[n + 1];
  if (hi <= lo) return;
  const int w = min(RLE_G, W - x0), len = (int)min(hi - lo, (int64_t)0x7fffffff);
  const int y0 = seg * R, y1 = min(H, y0 + R), U = W * S;
  const uint8_t* p = mask + (int64_t)n * H * W + x0;
  const int32_t* c = ws + (int64_t)n * 4 * U;
  int32_t* out = counts + lo;
  // every store goes through here: an index is clamped to the mask's own [offsets[n], offsets[n + 1])
  auto put = [&](int i, int v) { out[min(max(i, 0), len - 1)] = v; };
  const int fg0 = c[2 * U] & 1;
  int idx[RLE_G], prev[RLE_G], xh[RLE_G];
#pragma unroll
  for (int k = 0; k < RLE_G; ++k) {
    const int x = min(x0 + k, W - 1), u = x * S + seg;      // k >= w: a copy of the last column that never sees a transition (its bits are 0)
    xh[k] = x * H;
    idx[k] = fg0 + c[u];
    prev[k] = u > 0 ? c[U + u - 1] : 0;
    if (k < w && c[3 * U + u]) {              // the transition at the unit's first pixel
      put(idx[k]++, xh[k] + y0 - prev[k]);
      prev[k] = xh[k] + y0;
    }
  }
  uint32_t pb = w == RLE_G ? rle_row_bits<true>(p + (int64_t)y0 * W, w) : rle_row_bits<false>(p + (int64_t)y0 * W, w);
  rle_walk(p, y0, y1, W, w, [&](int y, uint32_t b) {
    const uint32_t d = b ^ pb;
    pb = b;
#pragma unroll
    for (int k = 0; k < RLE_G; ++k)
      if ((d >> k) & 1) {
        const int j = xh[k] + y;
        put(idx[k]++, j - prev[k]);
        prev[k] = j;
      }
  });
  if (x0 == 0 && seg == 0 && fg0) put(0, 0);
  if (x0 + w == W && seg == S - 1) {          // the run that ends the code
    int last = prev[0];
#pragma unroll
    for (int k = 1; k < RLE_G; ++k) last = k < w ? prev[k] : last;
    put(len - 1, H * W - last);
  }
}

// decode, first launch: ends = the inclusive scan of mask n's counts (clamped to H * W: a larger value only occurs in a
// code that is refused), status[n] = 1 when a count is negative or the total is not H * W.  One workgroup per mask.
__global__ __launch_bounds__(256) void rle_ends_kernel(const int32_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                       int32_t* __restrict__ ends, int32_t* __restrict__ status, int HW) {
  __shared__ long long wsum[4];
  const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t lo = offsets[n], len = offsets[n + 1] - lo;
  long long carry = 0;
  int bad = 0;
  for (int64_t base = 0; base < len; base += 256) {
    const int64_t i = base + t;
    long long s = 0;
    if (i < len) {
      const int v = counts[lo + i];
      bad |= v < 0;
      s = v < 0 ? 0 : v;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long a = __shfl_up(s, o, 64);
      if (lane >= o) s += a;
    }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    long long total = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (v < wave) s += wsum[v];
      total += wsum[v];
    }
    __syncthreads();
    if (i < len) ends[lo + i] = (int32_t)min(carry + s, (long long)HW);
    carry += total;
  }
  bad = __syncthreads_or(bad);
  if (t == 0) status[n] = (bad || carry != HW) ? 1 : 0;
}

// decode, second launch, in gather form: a lane owns RLE_G adjacent columns of a band of `rows` rows and asks, for each
// of its pixels j = x * H + y, for the first run whose end lies beyond j (zero counts are skipped by that rule); the
// run's parity is the pixel.  One binary search per column segment, then the index only advances.  The store address
// is a function of the thread's index alone; a refused code (status[n] != 0) stores zeros.
__global__ __launch_bounds__(64) void rle_gather_kernel(const int32_t* __restrict__ ends, const int64_t* __restrict__ offsets,
                                                        const int32_t* __restrict__ status, uint8_t* __restrict__ out, int H, int W, int rows) {
  const int n = blockIdx.z, x0 = (blockIdx.x * 64 + threadIdx.x) * RLE_G;
  if (x0 >= W) return;
  const int w = min(RLE_G, W - x0), y0 = blockIdx.y * rows, y1 = min(H, y0 + rows);
  const int64_t lo = offsets[n];
  const int len = (int)min(offsets[n + 1] - lo, (int64_t)0x7fffffff);
  const bool ok = status[n] == 0 && len > 0;
  const int32_t* e = ends + lo;
  uint8_t* o = out + (int64_t)n * H * W + x0;
  int idx[RLE_G], xh[RLE_G];
#pragma unroll
  for (int k = 0; k < RLE_G; ++k) {
    xh[k] = min(x0 + k, W - 1) * H;
    idx[k] = 0;
    if (ok && k < w) {                        // upper bound of j0 in e[0, len - 1): e[len - 1] = H * W lies beyond every pixel
      const int j0 = xh[k] + y0;
      int a = 0, b = len - 1;
      while (a < b) {
        const int mid = a + ((b - a) >> 1);
        if (e[mid] > j0) b = mid; else a = mid + 1;
      }
      idx[k] = a;
    }
  }
  for (int y = y0; y < y1; ++y) {
    uint32_t v = 0;
    if (ok) {
#pragma unroll
      for (int k = 0; k < RLE_G; ++k) {
        if (k < w) {
          const int j = xh[k] + y;
          while (idx[k] < len - 1 && e[idx[k]] <= j) ++idx[k];
          v |= (uint32_t)(idx[k] & 1) << (8 * k);
        }
      }
    }
    uint8_t* q = o + (int64_t)y * W;
    if (w == RLE_G) {
      __builtin_memcpy(q, &v, 4);
    } else {
      for (int k = 0; k < w; ++k) q[k] = (uint8_t)(v >> (8 * k));
    }
  }
}

}  // namespace

extern "C" int vg_connected_components(const uint8_t* mask, int32_t* labels, int32_t* counts, int N, int H, int W,
                                       int connectivity, vg_stream_t stream) {
  if (int e = cc_check(mask, labels, counts, N, H, W, "vg_connected_components")) return e;
  VG_CHECK(connectivity == 4 || connectivity == 8, VG_ERR_ARG, "vg_connected_components: connectivity %d not in {4, 8}", connectivity);
  CCArgs p{mask, labels, counts, nullptr, N, H, W, connectivity, 0, 0};
  return cc_run<0>(p, (hipStream_t)stream);
}

extern "C" int vg_remove_small_blobs(const uint8_t* mask, uint8_t* out, int32_t* ws_labels, int32_t* ws_counts, int N,
                                     int H, int W, int min_size, vg_stream_t stream) {
  if (int e = cc_check(mask, ws_labels, ws_counts, N, H, W, "vg_remove_small_blobs")) return e;
  VG_CHECK(out, VG_ERR_ARG, "vg_remove_small_blobs: null output");
  CCArgs p{mask, ws_labels, ws_counts, out, N, H, W, 4, 1, min_size};
  return cc_run<0>(p, (hipStream_t)stream);
}

extern "C" int vg_fill_holes(const float* scores, float* out, int32_t* ws_labels, int32_t* ws_counts, int N, int H,
                             int W, int max_area, vg_stream_t stream) {
  if (int e = cc_check(scores, ws_labels, ws_counts, N, H, W, "vg_fill_holes")) return e;
  VG_CHECK(out, VG_ERR_ARG, "vg_fill_holes: null output");
  VG_CHECK(max_area > 0, VG_ERR_ARG, "vg_fill_holes: max_area must be positive");   // misc.py:222
  CCArgs p{scores, ws_labels, ws_counts, out, N, H, W, 8, 2, max_area};
  return cc_run<1>(p, (hipStream_t)stream);
}

extern "C" int vg_mask_pair_counts(const uint8_t* a, const uint8_t* b, int64_t* inter, int64_t* uni, int P, int G,
                                   int64_t L, int diagonal, vg_stream_t stream) {
  VG_CHECK(a && b && inter && uni, VG_ERR_ARG, "vg_mask_pair_counts: null pointer");
  VG_CHECK(P > 0 && G > 0 && L > 0, VG_ERR_ARG, "vg_mask_pair_counts: bad shape P=%d G=%d L=%lld", P, G, (long long)L);
  VG_CHECK(!diagonal || P == G, VG_ERR_ARG, "vg_mask_pair_counts: diagonal needs P == G (got %d, %d)", P, G);
  const int64_t pairs = diagonal ? P : (int64_t)P * G;
  VG_CHECK(pairs <= 65535, VG_ERR_UNSUPPORTED, "vg_mask_pair_counts: %lld pairs > 65535", (long long)pairs);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(inter, 0, sizeof(int64_t) * pairs, st) != hipSuccess || hipMemsetAsync(uni, 0, sizeof(int64_t) * pairs, st) != hipSuccess) {
    vg_set_error("vg_mask_pair_counts: memset failed");
    return VG_ERR_LAUNCH;
  }
  const int vec = (L % 16 == 0) && ((((uintptr_t)a | (uintptr_t)b) & 15) == 0);
  int chunks = (int)((L / 16 + 255) / 256);      // at most 64 workgroups (= atomics per counter) per pair, >= 4 KB each
  chunks = chunks < 1 ? 1 : (chunks > 64 ? 64 : chunks);
  pair_counts_kernel<<<dim3(chunks, (unsigned)pairs), 256, 0, st>>>(a, b, (unsigned long long*)inter, (unsigned long long*)uni, G, L, vec, diagonal);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

// workgroups per mask of the two box reductions: `budget` over the batch, between 16 and 64 per mask, and never more
// than there are units of work.  Measured on 1024^2 masks, workgroups per mask 8 / 16 / 32 / 64 / 256: vg_mask_boxes
// 25.8 / 21.3 / 23.2 / 30.0 / 30.5 us at N = 32 and 23.7 / 19.3 / 18.9 / 21.7 / 21.9 us at N = 8; vg_blob_boxes
// 16 / 64 / 256: 549 / 571 / 567 us at N = 32 and 170 / 152 / 152 us at N = 8.
static int box_chunks(int N, int64_t units, int budget) {
  const int cap = budget / N < 16 ? 16 : (budget / N > 64 ? 64 : budget / N);
  return (int)(units < 1 ? 1 : (units > cap ? cap : units));
}

extern "C" int vg_mask_boxes(const uint8_t* mask, int32_t* out, int N, int H, int W, vg_stream_t stream) {
  VG_CHECK(mask && out, VG_ERR_ARG, "vg_mask_boxes: null pointer");
  VG_CHECK(N > 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) && N <= 65535, VG_ERR_ARG, "vg_mask_boxes: bad shape N=%d H=%d W=%d", N, H, W);
  hipStream_t st = (hipStream_t)stream;
  if (int e = box_init(out, N, H, W, st)) return e;
  const int chunks = box_chunks(N, ((int64_t)H * W / 16 + 1023) / 1024, 256);      // >= 4 words (64 B) per thread
  mask_boxes_kernel<<<dim3(chunks, N), 256, 0, st>>>(mask, out, H, W, (int)((16ll * chunks * 256) % W));
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_blob_boxes(const uint8_t* mask, int32_t* out, uint8_t* out_mask, int32_t* ws_labels, int32_t* ws_counts,
                             int N, int H, int W, int min_size, vg_stream_t stream) {
  if (int e = cc_check(mask, ws_labels, ws_counts, N, H, W, "vg_blob_boxes")) return e;
  VG_CHECK(out, VG_ERR_ARG, "vg_blob_boxes: null output");
  VG_CHECK(min_size > 0, VG_ERR_ARG, "vg_blob_boxes: min_size must be positive (vg_mask_boxes is the unfiltered reduction)");
  hipStream_t st = (hipStream_t)stream;
  if (int e = box_init(out, N, H, W, st)) return e;
  CCArgs p{mask, ws_labels, ws_counts, out_mask, N, H, W, 4, 1, min_size};
  const dim3 tiles((W + 63) / 64, (H + 63) / 64, N);      // the three union-find passes of cc_run
  cc_tile_kernel<0><<<tiles, 256, 0, st>>>(p);
  if (tiles.x > 1 || tiles.y > 1) cc_border_kernel<<<tiles, 192, 0, st>>>(p);
  cc_flatten_count_kernel<<<tiles, 256, 0, st>>>(p);
  const int chunks = box_chunks(N, (H + 15) / 16, 512);
  cc_boxes_kernel<<<dim3(chunks, N), 1024, 0, st>>>(p, out, (H + chunks - 1) / chunks);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_boundary_counts(const uint8_t* fg, const uint8_t* gt, int64_t* out, int N, int H, int W, int radius,
                                  vg_stream_t stream) {
  VG_CHECK(fg && gt && out, VG_ERR_ARG, "vg_boundary_counts: null pointer");
  VG_CHECK(N > 0 && N <= 65535 && H > 0 && W > 0, VG_ERR_ARG, "vg_boundary_counts: bad shape N=%d H=%d W=%d", N, H, W);
  VG_CHECK(radius >= 0 && radius <= 31, VG_ERR_UNSUPPORTED, "vg_boundary_counts: radius %d not in [0, 31]", radius);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, sizeof(int64_t) * 4 * N, st) != hipSuccess) {
    vg_set_error("vg_boundary_counts: memset failed");
    return VG_ERR_LAUNCH;
  }
  boundary_counts_kernel<<<dim3((W + 63) / 64, (H + 63) / 64, N), 256, 0, st>>>(fg, gt, (unsigned long long*)out, H, W, radius);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_logit_class_counts(const void* logits, const uint8_t* target, int64_t* out, int N, int64_t L, int dtype,
                                     int ignore_index, vg_stream_t stream) {
  VG_CHECK(logits && target && out, VG_ERR_ARG, "vg_logit_class_counts: null pointer");
  VG_CHECK(N > 0 && N <= 65535 && L > 0 && L < (1ll << 40), VG_ERR_ARG, "vg_logit_class_counts: bad shape N=%d L=%lld", N, (long long)L);
  VG_CHECK(dtype == VG_F32 || dtype == VG_BF16, VG_ERR_ARG, "vg_logit_class_counts: dtype %d is neither VG_F32 nor VG_BF16", dtype);
  VG_CHECK(ignore_index >= 0 && ignore_index <= 255, VG_ERR_ARG, "vg_logit_class_counts: ignore_index %d not in [0, 255]", ignore_index);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, sizeof(int64_t) * 6 * N, st) != hipSuccess) {
    vg_set_error("vg_logit_class_counts: memset failed");
    return VG_ERR_LAUNCH;
  }
  // workgroups per mask: >= 4 groups of 16 pixels per thread, 2048 workgroups over the batch, between 16 and 256 per mask
  const int64_t units = (L / 16 + 1023) / 1024;
  const int cap = 2048 / N < 16 ? 16 : (2048 / N > 256 ? 256 : 2048 / N);
  const int chunks = (int)(units < 1 ? 1 : (units > cap ? cap : units));
  const dim3 grid(chunks, N);
  if (dtype == VG_BF16)
    logit_class_counts_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)logits, target, (unsigned long long*)out, L, (uint32_t)ignore_index);
  else
    logit_class_counts_kernel<float><<<grid, 256, 0, st>>>((const float*)logits, target, (unsigned long long*)out, L, (uint32_t)ignore_index);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

// U of ws_cols; 0 for a shape that is refused.  The kernels index the four planes of a mask's scratch in int (up to
// 4 * U), so 4 * U < 2^31 belongs to the contract: it only bites for masks of at most 64 rows and W >= 2^29.
extern "C" int vg_mask_rle_units(int H, int W) {
  if (H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31)) return 0;
  const int R = rle_rows(H);
  const int64_t U = (int64_t)W * ((H + R - 1) / R);
  return 4 * U < (1ll << 31) ? (int)U : 0;
}

static int rle_check(int N, int H, int W, const char* who) {
  VG_CHECK(N > 0 && N <= 65535 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31) && vg_mask_rle_units(H, W) > 0, VG_ERR_ARG,
           "%s: bad shape N=%d H=%d W=%d", who, N, H, W);
  return VG_OK;
}

static inline int rle_groups(int W) { return ((W + RLE_G - 1) / RLE_G + 63) / 64; }      // workgroups of 64 lanes per mask

extern "C" int vg_mask_rle_count(const uint8_t* mask, int32_t* ws_cols, int32_t* n_runs, int N, int H, int W, vg_stream_t stream) {
  VG_CHECK(mask && ws_cols && n_runs, VG_ERR_ARG, "vg_mask_rle_count: null pointer");
  if (int e = rle_check(N, H, W, "vg_mask_rle_count")) return e;
  hipStream_t st = (hipStream_t)stream;
  const int R = rle_rows(H), S = (H + R - 1) / R;
  rle_count_kernel<<<dim3(rle_groups(W), S, N), 64, 0, st>>>(mask, ws_cols, H, W, R);
  rle_scan_kernel<<<N, 1024, 0, st>>>(ws_cols, n_runs, H, W, S, R);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_mask_rle_emit(const uint8_t* mask, const int32_t* ws_cols, const int64_t* offsets, int32_t* counts, int N, int H, int W,
                                vg_stream_t stream) {
  VG_CHECK(mask && ws_cols && offsets && counts, VG_ERR_ARG, "vg_mask_rle_emit: null pointer");
  if (int e = rle_check(N, H, W, "vg_mask_rle_emit")) return e;
  const int R = rle_rows(H), S = (H + R - 1) / R;
  rle_emit_kernel<<<dim3(rle_groups(W), S, N), 64, 0, (hipStream_t)stream>>>(mask, ws_cols, offsets, counts, H, W, R);
  VG_LAUNCH_CHECK();
  return VG_OK;
}

extern "C" int vg_rle_to_mask(const int32_t* counts, const int64_t* offsets, uint8_t* out, int32_t* status, int32_t* ws_ends, int N, int H,
                              int W, vg_stream_t stream) {
  // counts / ws_ends may be null when every code is empty (offsets all equal): such codes are refused and nothing is read
  VG_CHECK(offsets && out && status && (!counts == !ws_ends), VG_ERR_ARG, "vg_rle_to_mask: null pointer");
  if (int e = rle_check(N, H, W, "vg_rle_to_mask")) return e;
  hipStream_t st = (hipStream_t)stream;
  rle_ends_kernel<<<N, 256, 0, st>>>(counts, offsets, ws_ends, status, H * W);
  const int rows = rle_rows(H);
  rle_gather_kernel<<<dim3(rle_groups(W), (H + rows - 1) / rows, N), 64, 0, st>>>(ws_ends, offsets, status, out, H, W, rows);
  VG_LAUNCH_CHECK();
  return VG_OK;
}
