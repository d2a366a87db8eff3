// Prints gemm_plan's answer for tests/test_gemm_route_plan.py: one "kernel gx gy gz gn nt lds" line per call read from stdin, at ncu = 256.
// A call is one line of integers in the order of tests/_gemm_route_rules.py's Call.  Host C++17 only: vg_gemm_route.h is what launch_gemm and
// vg_gemm_route (vg_gemm.hip) ask.
#include <cstdio>

#include "../videoglamm_amd/csrc/vg_gemm_route.h"

int main() {
  static const char* const names[] = {"skinny", "small64", "rr", "p8n", "p8", "s128", "k64b", "glds", "glds_glu"};
  static const float one = 1.f;
  long long M, N, K, lda, ldw, ldc;
  int es, out_bf16, a_op, batch, vec_out, wmode, H, W, ws, fp8, act, res, gamma, ln, rr, p8;
  while (std::scanf("%lld %lld %lld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld %lld %lld %d %d", &M, &N, &K, &es, &out_bf16, &a_op, &batch, &vec_out, &wmode,
                    &H, &W, &ws, &fp8, &act, &res, &gamma, &ln, &lda, &ldw, &ldc, &rr, &p8) == 22) {
    GemmArgs p{};
    p.M = (int)M; p.N = (int)N; p.K = (int)K; p.lda = lda; p.ldw = ldw; p.ldc = ldc;
    p.act = act; p.vec_out = vec_out; p.a_op = a_op; p.gn = 1; p.wsh = -1;
    if (wmode && ws) gemm_set_window(p, wmode, H, W, ws, &one);
    else p.wmode = wmode;                             // a window call of unknown geometry: what vg_gemm_route's windowed = 1 stands for
    if (fp8) p.sa = p.sw = &one;
    if (res) p.R = &one;
    if (gamma) p.gamma = &one;
    if (ln) p.ln_w = p.ln_b = &one;
    const GemmPlan pl = gemm_plan(p, batch, es, out_bf16 != 0, GemmKnobs{rr, p8}, 256);
    std::printf("%s %d %d %d %d %d %d\n", names[pl.kernel], pl.gx, pl.gy, pl.gz, pl.gn, pl.nt, pl.lds);
  }
  return 0;
}
