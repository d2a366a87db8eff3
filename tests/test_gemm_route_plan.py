"""The GEMM launcher's whole plan — kernel, grid or workgroup count, gn, the nt flag, dynamic LDS bytes — pinned without a GPU.

tests/gemm_route_plan_main.cpp is built with the host compiler alone and prints gemm_plan (videoglamm_amd/csrc/vg_gemm_route.h, what launch_gemm
launches) for every call it reads; the expected values are the transcription of the launcher's rules in tests/_gemm_route_rules.py, plus the
product's shapes and the corner forms by literal value.  A wrong grid, gn, nt or LDS size is invisible to the numerical tests (or only costs
time), so it is pinned here."""
import os
import subprocess

import pytest

import _gemm_route_rules as rules
from _gemm_route_rules import call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")       # the Makefile's compiler; -x c++: host code only
KNOBS = [(1, 1), (1, 0), (1, 2), (1, 3), (1, 4), (0, 1), (2, 1)]          # (VG_GEMM_RR, VG_GEMM_P8)
GLDS, P8, P8N, S128 = 4 * 128 * 144, 160 * 1024, 144 * 1024, 4 * 32 * 68 * 4

# call -> "kernel gx gy gz gn nt lds" at 256 CUs, worked out by hand from launch_gemm's rules
LITERAL = [
    # the shapes of test_abi.py::test_gemm_routing_rules
    (call(1, 4096, 4096), "skinny 1024 1 1 1 0 0"),
    (call(1697, 4096, 4096), "glds 32 14 1 4 0 %d" % GLDS),
    (call(1697, 14336, 4096, a_op=1), "p8 256 1 1 4 0 %d" % P8),
    (call(3361, 4096, 14336), "p8 224 1 1 4 0 %d" % P8),
    (call(32768, 1728, 576), "p8 256 1 1 4 0 %d" % P8),
    (call(32768, 1728, 576, wmode=1), "s128 14 256 1 4 0 %d" % S128),
    (call(131072, 1152, 288), "rr 256 1 1 4 1 %d" % (18 * 256 + 8 * 4096 + 2 * 64 * 592)),
    (call(524288, 432, 144), "rr 256 1 1 4 0 %d" % (7 * 256 + 8 * 4096 + 2 * 64 * 304)),
    (call(32768, 1152, 288), "k64b 9 256 1 4 0 %d" % S128),
    (call(4096, 432, 144), "k64b 4 32 1 4 0 %d" % S128),
    (call(524288, 432, 144, es=4), "k64b 4 4096 1 4 1 %d" % S128),
    (call(65536, 2304, 576), "p8 256 1 1 4 1 %d" % P8),
    (call(9232, 4096, 1024), "p8 256 1 1 4 0 %d" % P8),
    (call(65536, 576, 2304), "p8n 256 1 1 3 0 %d" % P8N),
    (call(65536, 576, 576), "p8n 256 1 1 3 0 %d" % P8N),
    (call(3361, 6144, 4096), "p8n 256 1 1 4 0 %d" % P8N),
    (call(9232, 1024, 4096), "p8n 222 1 1 4 0 %d" % P8N),
    (call(16384, 1152, 4608), "p8n 256 1 1 4 0 %d" % P8N),
    (call(16384, 4608, 1152), "p8 256 1 1 4 1 %d" % P8),          # 144 MB of output in 9216-byte rows: streaming stores
    (call(3361, 4096, 4096), "p8 224 1 1 4 0 %d" % P8),
    (call(3361, 14336, 4096, a_op=1), "p8 256 1 1 4 0 %d" % P8),
    (call(1697, 4096, 4096, es=4), "glds 32 14 1 4 0 %d" % GLDS),
    # a padding-free power-of-two window gather rides on the phase-split kernel; the same gather on a grid the windows do not tile does not
    (call(32768, 1728, 576, wmode=1, H=64, W=64, ws=8), "p8 256 1 1 4 0 %d" % P8),
    (call(32768, 1728, 576, wmode=1, H=60, W=60, ws=8), "s128 14 256 1 4 0 %d" % S128),
    (call(32768, 1728, 576, wmode=1, H=64, W=64, ws=8, p8=2), "s128 14 256 1 4 0 %d" % S128),      # (knob 2: the 256x256 kernel without its window form)
    # the row-register kernel with a LayerNorm (gamma | beta in LDS), and at K = 144 with every weight chunk resident
    (call(131072, 1152, 288, ln=1), "rr 256 1 1 4 1 %d" % (18 * 256 + 8 * 288 + 8 * 4096 + 2 * 64 * 592)),
    (call(65536, 144, 144, act=rules.ACT_GELU), "rr 256 1 1 2 0 %d" % (3 * 256 + 8 * 4096 + 3 * 64 * 304)),
    (call(300, 16, 144, rr=2), "rr 2 1 1 1 0 %d" % (256 + 8 * 4096 + 64 * 304)),
    # fp8 records (vg_gemm_f8 has its own launcher; the rules refuse them all the same): never rr, p8 or small64
    (call(3361, 4096, 4096, es=1, fp8=1), "glds 32 27 1 4 0 %d" % GLDS),
    (call(4096, 256, 256, fp8=1), "k64b 2 32 1 2 0 %d" % S128),
    (call(131072, 1152, 288, fp8=1), "k64b 9 1024 1 4 1 %d" % S128),
    (call(3361, 4096, 4096, fp8=1), "glds 32 27 1 4 0 %d" % GLDS),
    # rows that are not 16-byte aligned
    (call(3361, 4096, 4096, vec_out=0), "glds 32 27 1 4 0 %d" % GLDS),
    (call(4096, 256, 256, vec_out=0), "k64b 2 32 1 2 0 %d" % S128),
    (call(4096, 256, 256), "small64 4 64 1 2 0 %d" % (4 * 2 * 64 * 128)),
    # batched launches: grid z, and one tile queue over all entries on the persistent kernel
    (call(1024, 1024, 1152, batch=3), "s128 8 8 3 4 0 %d" % S128),
    (call(1024, 1024, 1152, batch=24), "p8 256 1 1 4 0 %d" % P8),
    (call(300, 128, 128, batch=3), "small64 2 5 3 1 0 %d" % (2 * 2 * 64 * 128)),
    (call(300, 64, 64), "small64 1 5 1 1 0 %d" % (4 * 32 * 36 * 4)),
    # Llama's gate|up at M = 3361 with 14336 outputs in the SwiGLU form of the 128x128 kernel: tiles of 128 rows x 64 outputs
    (call(3361, 14336, 4096, a_op=1, p8=0), "glds_glu 224 27 1 4 0 %d" % GLDS),
    (call(300, 128, 4096, a_op=1), "glds_glu 2 3 1 2 0 %d" % GLDS),
    # streaming stores: outputs of at least 128 MB whose rows are whole 64-byte sectors
    (call(65536, 1024, 576), "p8 256 1 1 4 1 %d" % P8),
    (call(65535, 1024, 576), "p8 256 1 1 4 0 %d" % P8),
    (call(70000, 1000, 576), "p8 256 1 1 4 0 %d" % P8),
]


def grid_calls():
    out = [rules.query_call(*q, rr=rr, p8=p8) for rr, p8 in KNOBS[:1] for q in rules.query_grid()]
    # the other knob settings, and epilogues / batch / unaligned rows, on bf16 (what the knobs and the row-register rules read)
    bf16 = [q for q in rules.query_grid() if q[3] == 1]
    out += [rules.query_call(*q, rr=rr, p8=p8) for rr, p8 in KNOBS[1:] for q in bf16]
    for M, N, K, _, a_op, win in bf16:
        if a_op or win or M not in (213, 4096, 65536, 131072):
            continue
        out += [call(M, N, K, batch=3), call(M, N, K, vec_out=0), call(M, N, K, out_bf16=0), call(M, N, K, act=rules.ACT_GELU, res=1),
                call(M, N, K, gamma=1, res=1), call(M, N, K, ln=1, act=rules.ACT_GELU), call(M, N, K, ldc=N + 8, lda=K + 8)]
        for mode, (H, W, ws) in ((1, (64, 64, 8)), (2, (64, 64, 16)), (1, (60, 64, 8)), (1, (48, 48, 16)), (2, (56, 56, 7))):
            B = max(1, M // (-(-H // ws) * -(-W // ws) * ws * ws))
            out.append(call(B * -(-H // ws) * -(-W // ws) * ws * ws, N, K, wmode=mode, H=H, W=W, ws=ws))
    return out


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "gemm_route_plan")
    src = os.path.join(ROOT, "tests", "gemm_route_plan_main.cpp")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", src, "-o", exe])
    calls = [c for c, _ in LITERAL] + grid_calls()
    out = subprocess.run([exe], input="".join(c.line() + "\n" for c in calls), capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) == len(calls) + 1 and out[-1] == ""
    return calls, out[:-1]


def test_plan_matches_the_launchers_rules(printed):
    calls, out = printed
    assert len(calls) > 100000
    bad = [(c, o, w) for c, o, w in ((c, o, " ".join(str(v) for v in rules.plan(c))) for c, o in zip(calls, out)) if o != w]
    assert not bad, (len(bad), bad[:4])
    assert {o.split()[0] for o in out} == set(rules.CODE)


@pytest.mark.parametrize("i", range(len(LITERAL)))
def test_plan_by_value(printed, i):
    c, want = LITERAL[i]
    assert printed[1][i] == want, c
    assert " ".join(str(v) for v in rules.plan(c)) == want, c
