// Which kernel runs an (M, N, K) GEMM of vg_gemm / vg_gemm_window / vg_gemm_ln, and with what launch geometry: the launch record, the shape rules and
// gemm_plan.  launch_gemm (vg_gemm.hip) launches what the plan says and vg_gemm_route answers from the same plan, so the launcher and the query cannot
// disagree.  Host code only, plain C++17, no HIP types: tests/gemm_route_plan_main.cpp builds it with the host compiler alone.  A wrong grid, gn, nt or
// LDS size passes every numerical test and only costs time, so the plan is pinned by tests/test_gemm_route_plan.py.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/vg_kernels.h"

struct GemmArgs {
  const void* A; const void* W; void* C; const float* bias; const float* gamma; const void* R;
  int64_t lda, ldw, ldc, ldr, sA, sW, sC, sR;
  int M, N, K, act;
  int vec_out;  // C/R rows are 16-byte aligned: the epilogue stores whole 16-byte chunks
  int a_op;     // 1: W holds gate|up rows ([2N,K]); output column n = silu(A.gate_n)*(A.up_n) (skinny path only)
  int gn;       // tile order: column groups of gn N-tiles, M-tiles fastest-but-one inside a group (see gemm_tile_of)
  // window-order <-> image-order row maps (vg_gemm_window): wmode 1 = A rows are gathered from an image-order tensor
  // (window_partition fused into the load), 2 = C and R rows are scattered to / read from image order (window_unpartition
  // + residual add fused into the epilogue).  GEMM row m is always the window-order index.
  int wmode, wH, wW, wws, wnH, wnW;
  int wsh;      // >= 0: ws, wnW, wnH are powers of two, their log2 packed as ws | nW << 8 | nH << 16 (gemm_window_row's shift path); -1: divide
  const void* zrow;   // K zeros: source of the padded window rows (the LDS-DMA cannot zero-fill)
  // fp8 operands (vg_gemm_f8): C = (A8 . W8^T) * sa[m] * sw[n] — one fp32 scale per A row (token) and per W row (output)
  const float* sa; const float* sw;
  // split-K (vg_gemm_splitk, 128x128 LDS-DMA kernel only): blockIdx.z = K slice of kchunk elements; raw fp32 partial tiles
  // go to part[z][M][N], a second kernel sums them and applies the epilogue
  int ksplit, kchunk; float* part;
  int nbatch;   // persistent 256x256 kernel: batch count (tiles of all batch entries form one queue)
  int nt;       // output tiles leave with non-temporal (streaming) stores: large outputs whose rows are whole 64-byte sectors (gemm_plan)
  // LayerNorm over K in front of the contraction (vg_gemm_ln; the row-register kernel only): A rows are normalised as they arrive in registers
  const float* ln_w; const float* ln_b; float ln_eps;
};

// the window fields of the record from a window call's geometry (mode 1 | 2, an H x W token grid in ws x ws windows, the zero row of mode 1)
inline void gemm_set_window(GemmArgs& p, int mode, int H, int W, int ws, const void* zrow) {
  p.wmode = mode; p.wH = H; p.wW = W; p.wws = ws;
  p.wnH = (H + ws - 1) / ws; p.wnW = (W + ws - 1) / ws;
  p.zrow = zrow;
  auto lg2 = [](int v) { int s = 0; while ((1 << s) < v) ++s; return (1 << s) == v ? s : -1; };
  const int a = lg2(p.wws), b = lg2(p.wnW), c = lg2(p.wnH);
  p.wsh = (a >= 0 && b >= 0 && c >= 0) ? (a | (b << 8) | (c << 16)) : -1;
}

// The knobs, read once from the environment by the library (vg_gemm.hip) and passed in; a test passes its own.
struct GemmKnobs {
  int rr;     // VG_GEMM_RR, row-register kernel (K = 144 / 288): 0 off (A/B), 1 rule (M >= 65536 rows), 2 every eligible shape (tests)
  int p8;     // VG_GEMM_P8, 0: no 256-row tile routes (A/B), 1 the rules, 2 / 3: the 256x256 / 256x192 kernel on every eligible bf16 shape, 4: the rules without the 256x192 tile
};

enum GemmKernel { GEMM_SKINNY, GEMM_SMALL64, GEMM_RR, GEMM_P8N, GEMM_P8, GEMM_S128, GEMM_K64B, GEMM_GLDS, GEMM_GLDS_GLU };

struct GemmPlan {
  GemmKernel kernel;
  int gx, gy, gz;   // the grid; the persistent kernels (rr, p8n, p8): gx workgroups.  (skinny: the row-streaming form's grid; launch_skinny has a short-K form of its own)
  int gn;           // GemmArgs::gn of the launch
  int nt;           // GemmArgs::nt of the launch
  int lds;          // dynamic LDS bytes
};

constexpr int GEMM_GLDS_LDS = 4 * 128 * 144;      // the fp32 epilogue staging needs 4 x 64 x 68 floats = 69632 B of LDS whatever the K step
constexpr int GEMM_P8_LDS = 160 * 1024, GEMM_P8N_LDS = 144 * 1024, GEMM_RR_LDS_CAP = 160 * 1024;

// tile walk (gemm_tile_of): column groups of 4 N-tiles, i.e. a 4 x 16 patch of concurrent tiles per XCD
// (measured r01, tools/bench_gemm.py: 4 >= 8 > 16 > row-major on every C1 shape)
inline int gemm_gn(int nt) { return nt < 4 ? nt : 4; }

// small problems with a short K: fewer than 256 tiles of 128x128 (the chip is not filled), K = 64 / 128 / 192 / 256 bf16 -> gemm_small64_kernel
inline bool route_small64(int64_t M, int64_t N, int64_t K, int es, int a_op, int wmode, int vec_out, int batch) {
  if (es != 2 || a_op || wmode || !vec_out || M <= 16 || K % 64 != 0 || K > 256) return false;
  return ((M + 127) / 128) * ((N + 127) / 128) * batch < 256;
}
// few K-steps per tile (K x element size <= 3 KB): the 64-byte-step kernel with four workgroups per CU
// (measured r01, tools/bench_gemm.py: +20...50 % on the Hiera / tower shapes up to K = 1408, -10...15 % from K = 2304 up)
inline bool route_small_k(int64_t K, int es, int a_op) {
  return K * es <= 3072 && a_op == 0;
}
// single-stage 128-byte-row kernel: the small-K shapes with at least four whole-line K steps (measured r01: +16...18 % on
// Hiera stage 3 / 4 and +7...14 % on the tower shapes over the 64-byte-row kernel; K = 144 / 288 stay there)
inline bool route_s128(int64_t K, int es, int a_op) {
  return route_small_k(K, es, a_op) && K * es >= 1024;
}
// 256x256 tile, 128x128 per wave: bf16, whole 128-byte K steps, and the 256-tiles must use the chip well: (useful
// fraction of the tiles' area) x (fill of the rounds of 256 workgroups) >= 0.7 — Hiera's N = 576 outputs or 168-tile
// grids stay on the 128x128 kernels (measured r01, tools/bench_gemm.py).  a_op == 1: a tile is 256 rows x 128 outputs
inline bool route_p8(int w /* GemmKnobs::p8 */, int64_t M, int64_t N, int64_t K, int es, int a_op, int wmode, int vec_out, int batch, int* ntw_out, int* mtw_out) {
  const int ntw = (int)(a_op == 1 ? (N + 127) / 128 : (N + 255) / 256), mtw = (int)((M + 255) / 256);
  *ntw_out = ntw; *mtw_out = mtw;
  // (r02, persistent kernel + straight-line epilogue: from K x es = 2304 B — Hiera stage 4, InternVideo2 — the 256x256 kernel beats the
  // single-stage 128x128 one by 2...9 %; K = 1024 / 576 stay there)
  constexpr int smallk_min = 1152;     // r04: with the phase-split kernel also K = 576 (Hiera stage 3): C2 268.5 -> 266.7 ms same-box
  if (!w || es != 2 || (route_small_k(K, es, a_op) && K * es < smallk_min) || wmode || K % (128 / es) != 0 || !vec_out) return false;
  if (w == 2) return true;       // 2: force the 256x256 kernel on every eligible shape (4 = the shape rule, without the 256x192 tile)
  const int64_t t256 = (int64_t)ntw * mtw * batch;
  const double useful = (double)M * N / ((double)mtw * 256 * ntw * (a_op == 1 ? 128 : 256));
  const double fill = (double)t256 / (double)(((t256 + 255) / 256) * 256);
  return t256 >= 128 && useful * fill >= 0.7;
}

// 256 x 192 tiles (vg_gemm_p8n.hip, r05) instead of 256 x 256 when whole rounds x tile cost say so: cost = rounds of 256 workgroups x
// (0.87 | 1) — measured r05 (tools/lab/p8n_ab.sh, same box): a narrow tile costs 0.83-0.90 of a wide one at equal rounds (it stages 7/8 of the
// bytes for 3/4 of the MFMAs).  N = 576 is three exact 192-tiles against 2.25 of three 256-tiles (Hiera stage 3 fc2 195 -> 162 us, proj
// 86 -> 55), Llama's q|k|v at M = 3361 two rounds of the narrow tile against two of the wide one (189 -> 170 us; r04's 128x128 route: 213).  Without a valid 256-route for the shape (under-filled or badly quantised grids) the narrow tile is judged by the
// same fill rule.
inline bool route_p8n(int w /* GemmKnobs::p8 */, int64_t M, int64_t N, int64_t K, int es, int a_op, int wmode, int vec_out, int batch, bool p8_ok, int* nt_out, int* mt_out) {
  const int nt = (int)((N + 191) / 192), mt = (int)((M + 255) / 256);
  *nt_out = nt; *mt_out = mt;
  if (es != 2 || a_op || wmode || K % 64 != 0 || K < 128 || !vec_out) return false;
  if (w == 3) return true;       // 3: force the 256x192 kernel on every eligible shape (tests: minimal K, tiny grids)
  if (w != 1 || (route_small_k(K, es, a_op) && K * es < 1152)) return false;      // (4: the shape rule without the narrow tile — A/B)
  const int64_t t192 = (int64_t)nt * mt * batch, t256 = (int64_t)((N + 255) / 256) * mt * batch;
  if (t192 < 128) return false;
  const int64_t r192 = (t192 + 255) / 256, r256 = (t256 + 255) / 256;
  if (!p8_ok) {
    const double useful = (double)M * N / ((double)mt * 256 * nt * 192), fill = (double)t192 / (double)(r192 * 256);
    return useful * fill >= 0.7;
  }
  return (double)r192 * 0.87 < 0.97 * (double)r256;
}

// the window forms the 256-row kernels take: A rows gathered (mode 1) or C / R rows scattered (mode 2), windows a power of two that tile the image exactly (no padding rows: the 32-bit
// source offsets cannot reach the zero row)
inline bool vg_gemm_p8_window_ok(int wmode, int wsh, int wH, int wW, int wws) {
  return (wmode == 1 || wmode == 2) && wsh >= 0 && wws > 0 && wH % wws == 0 && wW % wws == 0;
}

// what the 32-bit source offsets of the 256-row kernels (vg_gemm_p8.hip, vg_gemm_p8n.hip) need; route_p8 / route_p8n decide the rest
inline bool vg_gemm_p8_eligible(const GemmArgs& p, int batch) {
  const int64_t arows = p.M, wrows = p.a_op == 1 ? 2 * (int64_t)p.N : p.N;
  const bool win_ok = p.wmode == 0 || (vg_gemm_p8_window_ok(p.wmode, p.wsh, p.wH, p.wW, p.wws) && !(p.wmode == 2 && p.a_op == 1));
  return p.K % 64 == 0 && p.K >= 128 && arows * p.lda * 2 < (int64_t)1 << 32 && wrows * p.ldw * 2 < (int64_t)1 << 32 && !p.sa && win_ok && p.vec_out;
}

// the row-register kernel (vg_gemm_rr.hip): K in {144, 288}, bf16 in and out, N a multiple of 16, 16-byte aligned C / R rows, act none | GELU (GELU without a residual), no LayerScale / fp8 scales / batch
inline bool vg_gemm_rr_eligible(const GemmArgs& p, int batch, bool out_is_bf16) {
  return (p.K == 144 || p.K == 288) && out_is_bf16 && batch == 1 && !p.a_op && !p.sa && !p.gamma && p.vec_out && p.N % 16 == 0 && p.N >= 16 &&
         (p.act == VG_ACT_NONE || (p.act == VG_ACT_GELU && !p.R)) && p.ksplit <= 1 && !((p.ln_w || p.ln_b) && p.R) &&
         // the streamed form's LDS: bias per 64-column chunk + gamma | beta + the epilogue slabs + two weight slots (gemm_rr_form) within 158 KB
         (size_t)((p.N + 63) / 64) * 256 + 8 * (size_t)p.K + 8 * 4096 + 2 * 64 * (size_t)(p.K * 2 + 16) <= 158 * 1024;
}

// the row-register kernel's launch: one workgroup per CU walks the 256-row panels; at K = 144 every weight chunk stays resident in LDS when they all fit, else two slots are streamed
struct GemmRrForm { bool resident; int wgs; size_t lds; };
inline GemmRrForm gemm_rr_form(const GemmArgs& q, int ncu) {
  const int npanel = (q.M + 255) / 256, wgs = npanel < ncu ? npanel : ncu, nch = (q.N + 63) / 64;
  const size_t slot = 64 * (size_t)(q.K * 2 + 16), fixed = (size_t)nch * 256 + ((q.ln_w || q.ln_b) ? 8 * (size_t)q.K : 0) + 8 * 4096;   // bias | gamma, beta | slabs
  if (q.K == 144 && fixed + nch * slot <= 158 * 1024) return {true, wgs, fixed + nch * slot};
  return {false, wgs, fixed + 2 * slot};
}

// The route of one launch.  p: the launch record (gn, nt, nbatch are outputs of the plan, not read), es: bytes per input element, ncu: the device's CU count.
// The order of the tests is the launcher's: M <= 16, small64, rr, narrow, big, s128, small-K, glds.
inline GemmPlan gemm_plan(const GemmArgs& p, int batch, int es, bool out_is_bf16, const GemmKnobs& kn, int ncu) {
  const int oes = out_is_bf16 ? 2 : 4;
  if (p.M <= 16) return {GEMM_SKINNY, (p.N + 3) / 4, 1, batch, p.gn, 0, 0};
  const int mt = (p.M + 127) / 128, nt = (p.N + 127) / 128;
  GemmPlan pl{GEMM_GLDS, nt, mt, batch, gemm_gn(nt), 0, GEMM_GLDS_LDS};
  // streaming stores for big outputs (>= 128 MB, r03) with sector-aligned rows (epi_store16)
  pl.nt = p.vec_out && (p.ldc * (int64_t)oes) % 64 == 0 && (int64_t)p.M * p.N * (int64_t)oes * batch >= (int64_t)128 << 20;
  auto persistent = [&](GemmKernel k, int mtk, int ntk, int lds) {      // one workgroup per CU walks the tile queue
    const int64_t tot = (int64_t)ntk * mtk * batch;
    pl.kernel = k; pl.gx = (int)(tot > ncu ? ncu : tot); pl.gy = pl.gz = 1; pl.gn = gemm_gn(ntk); pl.lds = lds;
    return pl;
  };
  if (es == 2 && route_small64(p.M, p.N, p.K, es, p.a_op, p.wmode, p.vec_out, batch) && !p.sa) {
    const int nseg = p.K / 64;
    pl.kernel = GEMM_SMALL64; pl.gx = (p.N + 63) / 64; pl.gy = (p.M + 63) / 64;
    pl.lds = nseg * 2 * 64 * 128 > 4 * 32 * 36 * 4 ? nseg * 2 * 64 * 128 : 4 * 32 * 36 * 4;
    return pl;
  }
  // short K over very many rows (Hiera stages 1-2, the FPN laterals of those levels): A rows in registers, no tiles (vg_gemm_rr.hip)
  if (es == 2 && kn.rr && vg_gemm_rr_eligible(p, batch, out_is_bf16) && (kn.rr == 2 || p.M >= 65536)) {
    const GemmRrForm f = gemm_rr_form(p, ncu);
    pl.kernel = GEMM_RR; pl.gx = f.wgs; pl.gy = pl.gz = 1; pl.lds = (int)f.lds;
    return pl;
  }
  // (r04: a padding-free power-of-two window GATHER rides on the phase-split kernel — Hiera stage 3's windowed qkv; everything else windowed
  // stays on the 128x128 kernels)
  const int wroute = ((kn.p8 == 1 || kn.p8 >= 3) && es == 2 && vg_gemm_p8_window_ok(p.wmode, p.wsh, p.wH, p.wW, p.wws)) ? 0 : p.wmode;
  int ntw, mtw, ntn, mtn;
  const bool big = route_p8(kn.p8, p.M, p.N, p.K, es, p.a_op, wroute, p.vec_out, batch, &ntw, &mtw) && vg_gemm_p8_eligible(p, batch);
  const bool narrow = route_p8n(kn.p8, p.M, p.N, p.K, es, p.a_op, wroute, p.vec_out, batch, big, &ntn, &mtn) && vg_gemm_p8_eligible(p, batch);
  if (narrow) return persistent(GEMM_P8N, mtn, ntn, GEMM_P8N_LDS);
  if (big) return persistent(GEMM_P8, mtw, ntw, GEMM_P8_LDS);
  if (route_s128(p.K, es, p.a_op)) { pl.kernel = GEMM_S128; pl.lds = 4 * 32 * 68 * 4; }
  else if (route_small_k(p.K, es, p.a_op)) { pl.kernel = GEMM_K64B; pl.lds = 4 * 32 * 68 * 4; }
  else if (p.a_op == 1) {       // SwiGLU in the epilogue: a tile = 128 rows x 64 outputs (gate | up halves)
    pl.kernel = GEMM_GLDS_GLU; pl.gx = (p.N + 63) / 64; pl.gn = gemm_gn(pl.gx);
  }
  return pl;
}
