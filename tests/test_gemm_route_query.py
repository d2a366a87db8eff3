"""vg_gemm_route against the launcher's rules (tests/_gemm_route_rules.py) over a grid of shapes, both input dtypes, a_op 0 / 1, windowed 0 / 1, under
every knob setting.  bench.py attributes launch times with the query, ops.linear decides its tail split with it and ops.linear_ln its fused form:
an answer that is not what launch_gemm runs misleads all three.  No GPU: the query launches nothing.  The knobs are read once per process, so one
child process per setting prints the whole grid."""
import json
import os
import subprocess
import sys

import pytest

import _gemm_route_rules as rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = [(1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (0, 1), (2, 1)]          # (VG_GEMM_RR, VG_GEMM_P8)

_CHILD = ("import json, sys; sys.path[:0] = [%r, %r]\n"
          "import _gemm_route_rules as rules\n"
          "from videoglamm_amd import _lib\n"
          "lib = _lib.load()\n"
          "print(json.dumps([lib.vg_gemm_route(*q) for q in rules.query_grid() + [tuple(q) for q in json.loads(sys.argv[1])]]))\n")


def routes(rr, p8, extra=()):
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, here), json.dumps(list(extra))], env=dict(os.environ, VG_GEMM_RR=str(rr), VG_GEMM_P8=str(p8)),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(r.stdout.strip().split("\n")[-1])


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()


@pytest.mark.parametrize("rr,p8", KNOBS)
def test_query_answers_what_the_launcher_runs(built, rr, p8):
    grid = rules.query_grid()
    got = routes(rr, p8)
    assert len(got) == len(grid) == 2 * 2 * 2 * 13 * 15 * 16
    want = [rules.CODE[rules.plan(rules.query_call(*q, rr=rr, p8=p8)).kernel] for q in grid]
    bad = [(q, g, w) for q, g, w in zip(grid, got, want) if g != w]
    assert not bad, (len(bad), bad[:8])
    assert set(want) >= ({1, 2, 4, 5} | ({3} if p8 in (1, 2, 4) else set()) | ({6} if p8 in (1, 3) else set()) | ({7} if rr else set())), set(want)      # the grid reaches every kernel the setting allows


def test_query_follows_the_launchers_own_refusals(built):
    """Where the launcher's eligibility is stricter than the shape rules, the query answers the kernel that runs: a row-register shape over that
    kernel's LDS bound (K = 288: N > 12736; K = 144: N > 22208) goes to the 64-byte-step kernel, a 256-row shape whose A reaches 4 GiB (32-bit source
    offsets) to the 128x128 LDS-DMA kernel, as does a SwiGLU shape at K = 64 (the 256-row pipeline needs K >= 128).  The grid above holds such cells
    too (N = 14336 at K = 288; M = 524288 from K = 4096 up; a_op = 1 at K = 64): there, and only there, the query answered otherwise before it was
    built on the launcher's plan."""
    over = [(70000, 12752, 288, 1, 0, 0), (70000, 22224, 144, 1, 0, 0), (1048576, 2304, 2304, 1, 0, 0), (1697, 4096, 64, 1, 1, 0)]
    under = [(70000, 12736, 288, 1, 0, 0), (70000, 22208, 144, 1, 0, 0), (524288, 2304, 2304, 1, 0, 0), (1697, 4096, 128, 1, 1, 0)]
    n = len(rules.query_grid())
    got = routes(1, 1, over + under)[n:]
    assert got[:4] == [2, 2, 1, 1], got
    assert got[4:] == [7, 7, 3, 3], got
    assert [rules.CODE[rules.plan(rules.query_call(*q)).kernel] for q in over + under] == got
