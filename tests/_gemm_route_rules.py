"""The GEMM launcher's routing rules, transcribed into Python from launch_gemm (videoglamm_amd/csrc/vg_gemm.hip) as it stood before the rules moved
to vg_gemm_route.h: which kernel runs a call, and its grid / workgroup count, gn, nt flag and dynamic LDS bytes.  The order of the tests is the
launcher's: M <= 16, small64, rr, narrow (256x192), big (256x256), s128, small-K, glds.  Shared by test_gemm_route_query.py (vg_gemm_route against
the kernel of this plan) and test_gemm_route_plan.py (the C++ plan, field by field)."""
from collections import namedtuple

CODE = {"skinny": 0, "glds": 1, "glds_glu": 1, "k64b": 2, "p8": 3, "s128": 4, "small64": 5, "p8n": 6, "rr": 7}      # vg_gemm_route's answers
GRID_M = (17, 64, 213, 300, 1697, 3361, 4096, 9232, 16384, 32768, 65536, 131072, 524288)
GRID_N = (16, 64, 128, 192, 256, 432, 576, 1024, 1152, 1728, 2304, 4096, 4608, 6144, 14336)
GRID_K = (64, 128, 144, 192, 256, 288, 320, 576, 704, 1024, 1152, 1408, 2304, 4096, 4608, 14336)
ACT_NONE, ACT_GELU = 0, 1

Plan = namedtuple("Plan", "kernel gx gy gz gn nt lds")
_FIELDS = "M N K es out_bf16 a_op batch vec_out wmode H W ws fp8 act res gamma ln lda ldw ldc rr p8"


class Call(namedtuple("Call", _FIELDS)):
    """One launch record.  wmode 1 | 2 with ws = 0: a window call of unknown geometry (vg_gemm_route's windowed = 1)."""

    def line(self):
        return " ".join(str(int(v)) for v in self)


def call(M, N, K, es=2, out_bf16=None, a_op=0, batch=1, vec_out=1, wmode=0, H=0, W=0, ws=0, fp8=0, act=ACT_NONE, res=0, gamma=0, ln=0, lda=None, ldw=None,
         ldc=None, rr=1, p8=1):
    return Call(M, N, K, es, (es == 2) if out_bf16 is None else out_bf16, a_op, batch, vec_out, wmode, H, W, ws, fp8, act, res, gamma, ln,
                K if lda is None else lda, K if ldw is None else ldw, N if ldc is None else ldc, rr, p8)


def cdiv(a, b):
    return (a + b - 1) // b


def gn_of(nt):
    return min(nt, 4)


def small_k(K, es, a_op):
    return K * es <= 3072 and a_op == 0


def window_pow2(c):
    """the shift form of the window row map: ws and the window counts are powers of two"""
    if not c.wmode or not c.ws:
        return False
    p2 = lambda v: v > 0 and v & (v - 1) == 0
    return p2(c.ws) and p2(cdiv(c.W, c.ws)) and p2(cdiv(c.H, c.ws))


def p8_window_ok(c):
    return c.wmode in (1, 2) and window_pow2(c) and c.H % c.ws == 0 and c.W % c.ws == 0


def p8_eligible(c):
    wrows = 2 * c.N if c.a_op == 1 else c.N
    win_ok = c.wmode == 0 or (p8_window_ok(c) and not (c.wmode == 2 and c.a_op == 1))
    return (c.K % 64 == 0 and c.K >= 128 and c.M * c.lda * 2 < 1 << 32 and wrows * c.ldw * 2 < 1 << 32 and not c.fp8 and win_ok and bool(c.vec_out))


def rr_eligible(c):
    return (c.K in (144, 288) and c.out_bf16 and c.batch == 1 and not c.a_op and not c.fp8 and not c.gamma and c.vec_out and c.N % 16 == 0 and c.N >= 16
            and (c.act == ACT_NONE or (c.act == ACT_GELU and not c.res)) and not (c.ln and c.res)
            and cdiv(c.N, 64) * 256 + 8 * c.K + 8 * 4096 + 2 * 64 * (c.K * 2 + 16) <= 158 * 1024)


def route_p8(c, wroute):
    ntw, mtw = (cdiv(c.N, 128) if c.a_op == 1 else cdiv(c.N, 256)), cdiv(c.M, 256)
    if (not c.p8 or c.es != 2 or (small_k(c.K, c.es, c.a_op) and c.K * c.es < 1152) or wroute or c.K % (128 // c.es) != 0 or not c.vec_out):
        return False, ntw, mtw
    if c.p8 == 2:
        return True, ntw, mtw
    t256 = ntw * mtw * c.batch
    useful = float(c.M) * c.N / (float(mtw) * 256 * ntw * (128 if c.a_op == 1 else 256))
    fill = float(t256) / float(cdiv(t256, 256) * 256)
    return t256 >= 128 and useful * fill >= 0.7, ntw, mtw


def route_p8n(c, wroute, p8_ok):
    nt, mt = cdiv(c.N, 192), cdiv(c.M, 256)
    if c.es != 2 or c.a_op or wroute or c.K % 64 != 0 or c.K < 128 or not c.vec_out:
        return False, nt, mt
    if c.p8 == 3:
        return True, nt, mt
    if c.p8 != 1 or (small_k(c.K, c.es, c.a_op) and c.K * c.es < 1152):
        return False, nt, mt
    t192, t256 = nt * mt * c.batch, cdiv(c.N, 256) * mt * c.batch
    if t192 < 128:
        return False, nt, mt
    r192, r256 = cdiv(t192, 256), cdiv(t256, 256)
    if not p8_ok:
        useful, fill = float(c.M) * c.N / (float(mt) * 256 * nt * 192), float(t192) / float(r192 * 256)
        return useful * fill >= 0.7, nt, mt
    return float(r192) * 0.87 < 0.97 * float(r256), nt, mt


def plan(c, ncu=256):
    oes = 2 if c.out_bf16 else 4
    if c.M <= 16:
        return Plan("skinny", cdiv(c.N, 4), 1, c.batch, 1, 0, 0)
    mt, nt = cdiv(c.M, 128), cdiv(c.N, 128)
    gn = gn_of(nt)
    stream = int(bool(c.vec_out) and (c.ldc * oes) % 64 == 0 and c.M * c.N * oes * c.batch >= 128 << 20)
    if c.es == 2 and not c.a_op and not c.wmode and c.vec_out and c.K % 64 == 0 and c.K <= 256 and mt * nt * c.batch < 256 and not c.fp8:
        return Plan("small64", cdiv(c.N, 64), cdiv(c.M, 64), c.batch, gn, stream, max(c.K // 64 * 2 * 64 * 128, 4 * 32 * 36 * 4))
    if c.es == 2 and c.rr and rr_eligible(c) and (c.rr == 2 or c.M >= 65536):
        nch, slot = cdiv(c.N, 64), 64 * (c.K * 2 + 16)
        fixed = nch * 256 + (8 * c.K if c.ln else 0) + 8 * 4096
        lds = fixed + nch * slot if c.K == 144 and fixed + nch * slot <= 158 * 1024 else fixed + 2 * slot
        return Plan("rr", min(cdiv(c.M, 256), ncu), 1, 1, gn, stream, lds)
    wroute = 0 if (c.p8 == 1 or c.p8 >= 3) and c.es == 2 and p8_window_ok(c) else c.wmode
    big, ntw, mtw = route_p8(c, wroute)
    big = big and p8_eligible(c)
    narrow, ntn, mtn = route_p8n(c, wroute, big)
    narrow = narrow and p8_eligible(c)
    if narrow:
        return Plan("p8n", min(ntn * mtn * c.batch, ncu), 1, 1, gn_of(ntn), stream, 144 * 1024)
    if big:
        return Plan("p8", min(ntw * mtw * c.batch, ncu), 1, 1, gn_of(ntw), stream, 160 * 1024)
    if small_k(c.K, c.es, c.a_op):
        return Plan("s128" if c.K * c.es >= 1024 else "k64b", nt, mt, c.batch, gn, stream, 4 * 32 * 68 * 4)
    if c.a_op == 1:
        return Plan("glds_glu", cdiv(c.N, 64), mt, c.batch, gn_of(cdiv(c.N, 64)), stream, 4 * 128 * 144)
    return Plan("glds", nt, mt, c.batch, gn, stream, 4 * 128 * 144)


def query_grid():
    """(M, N, K, in_dtype, a_op, windowed) in the order both sides walk: the arguments of vg_gemm_route"""
    return [(M, N, K, dt, a_op, win) for dt in (1, 0) for a_op in (0, 1) for win in (0, 1) for M in GRID_M for N in GRID_N for K in GRID_K]


def query_call(M, N, K, dt, a_op, win, rr=1, p8=1):
    """the record vg_gemm_route stands for: contiguous, aligned, batch 1, no epilogue; windowed = geometry unknown"""
    return call(M, N, K, es=2 if dt == 1 else 4, a_op=a_op, wmode=1 if win else 0, rr=rr, p8=p8)
