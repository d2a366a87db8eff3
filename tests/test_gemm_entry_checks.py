"""What the GEMM entry points refuse, and how: return code and message, recorded from the library before vg_gemm, vg_gemm_window and vg_gemm_ln
shared one explicit body (they used to hand their window and LayerNorm to vg_gemm through thread-locals).

As in test_decode_entry_checks.py every case is refused BEFORE any launch, the pointers are host allocations that a refused call never touches, and
the whole module skips when a GPU is visible.  A window or LayerNorm call reports a refusal of the shared body under the name of the check that made
it: vg_gemm_window's geometry checks say `vg_gemm_window:` also when vg_gemm_ln made them, the operand checks say `vg_gemm:`."""
import pytest

from test_decode_entry_checks import ARG, BF16, BIG, BUF, F32, UNSUPPORTED, entry

OK = 0
ENTRIES = {
    "vg_gemm": entry("*A lda sA *W ldw sW *C ldc sC *bias *gamma *R ldr sR M N K batch in_dtype out_dtype act a_op *stream",
                     bias=None, gamma=None, R=None, stream=None, lda=64, ldw=64, ldc=64, M=64, N=64, K=64, batch=1, in_dtype=BF16, out_dtype=BF16),
    "vg_gemm_window": entry("*A lda *W ldw *C ldc *bias *gamma *R ldr N K in_dtype out_dtype act mode B H Wd ws *zero_row *stream",
                            bias=None, gamma=None, R=None, stream=None, lda=64, ldw=64, ldc=64, N=64, K=64, in_dtype=BF16, out_dtype=BF16, mode=1, B=1, H=8,
                            Wd=8, ws=4),
    "vg_gemm_ln": entry("*A lda *W ldw *C ldc *bias *ln_w *ln_b ln_eps M N K act window B H Wd ws *zero_row dtype *stream",
                        bias=None, stream=None, lda=144, ldw=144, ldc=64, ln_eps=1e-6, M=65536, N=64, K=144, B=1, H=8, Wd=8, ws=4, dtype=BF16),
    "vg_gemm_splitk": entry("*A lda *W ldw *C ldc *bias *gamma *R ldr M N K in_dtype out_dtype act ksplit *workspace ws_floats *stream",
                            bias=None, gamma=None, R=None, stream=None, lda=256, ldw=256, ldc=64, M=64, N=64, K=256, in_dtype=BF16, out_dtype=BF16, ksplit=2,
                            ws_floats=BIG),
    "vg_gemm_f8": entry("*A8 lda *a_scale *W8 ldw *w_scale *C ldc *bias *R ldr M N K out_dtype a_op *stream",
                        bias=None, R=None, stream=None, lda=64, ldw=64, ldc=64, M=64, N=64, K=64, out_dtype=BF16),
}

# (entry point, the arguments that differ from the table's call, return code, how the message starts)
CASES = [
    ("vg_gemm", dict(A=None), ARG, "vg_gemm: null pointer"),
    ("vg_gemm", dict(C=None), ARG, "vg_gemm: null pointer"),
    ("vg_gemm", dict(M=-1), ARG, "vg_gemm: bad shape M=-1 N=64 K=64 batch=1"),
    ("vg_gemm", dict(N=0), ARG, "vg_gemm: bad shape"),
    ("vg_gemm", dict(batch=0), ARG, "vg_gemm: bad shape"),
    ("vg_gemm", dict(M=0), OK, ""),
    ("vg_gemm", dict(a_op=2), ARG, "vg_gemm: bad a_op 2"),
    ("vg_gemm", dict(in_dtype=7), ARG, "vg_gemm: bad in_dtype 7"),
    ("vg_gemm", dict(K=60), ARG, "vg_gemm: K/lda/ldw/strides must be multiples of 8 (K=60 lda=64 ldw=64)"),
    ("vg_gemm", dict(lda=68), ARG, "vg_gemm: K/lda/ldw/strides must be multiples of 8"),
    ("vg_gemm", dict(sW=4), ARG, "vg_gemm: K/lda/ldw/strides must be multiples of 8"),
    ("vg_gemm", dict(in_dtype=F32, out_dtype=F32, K=62), ARG, "vg_gemm: K/lda/ldw/strides must be multiples of 4"),
    ("vg_gemm", dict(A=BUF + 8), ARG, "vg_gemm: A/W must be 16-byte aligned"),
    ("vg_gemm", dict(W=BUF + 2), ARG, "vg_gemm: A/W must be 16-byte aligned"),
    ("vg_gemm", dict(a_op=1, R=BUF), UNSUPPORTED, "vg_gemm: a_op=1 with M > 16 needs"),
    ("vg_gemm", dict(a_op=1, gamma=BUF), UNSUPPORTED, "vg_gemm: a_op=1 with M > 16 needs"),
    ("vg_gemm", dict(a_op=1, act=1), UNSUPPORTED, "vg_gemm: a_op=1 with M > 16 needs"),
    ("vg_gemm", dict(a_op=1, batch=2), UNSUPPORTED, "vg_gemm: a_op=1 with M > 16 needs"),
    ("vg_gemm", dict(a_op=1, ldc=60), UNSUPPORTED, "vg_gemm: a_op=1 with M > 16 needs"),
    ("vg_gemm", dict(out_dtype=7), UNSUPPORTED, "vg_gemm: unsupported dtype combination 1 -> 7"),
    ("vg_gemm_window", dict(mode=3), ARG, "vg_gemm_window: bad window mode=3 B=1 H=8 W=8 ws=4"),
    ("vg_gemm_window", dict(mode=0), ARG, "vg_gemm_window: bad window mode=0"),
    ("vg_gemm_window", dict(ws=0), ARG, "vg_gemm_window: bad window mode=1 B=1 H=8 W=8 ws=0"),
    ("vg_gemm_window", dict(B=0), ARG, "vg_gemm_window: bad window"),
    ("vg_gemm_window", dict(zero_row=None), ARG, "vg_gemm_window: mode 1 needs a row of K zeros"),
    ("vg_gemm_window", dict(H=4, Wd=4), UNSUPPORTED, "vg_gemm_window: 16 rows"),
    ("vg_gemm_window", dict(B=32768, H=256, Wd=256, ws=8), UNSUPPORTED, "vg_gemm_window: 2147483648 rows"),
    ("vg_gemm_window", dict(mode=2, ldc=60), UNSUPPORTED, "vg_gemm_window: scattered C/R rows must be 16-byte aligned (ldc=60 ldr=0)"),
    ("vg_gemm_window", dict(mode=2, R=BUF, ldr=68), UNSUPPORTED, "vg_gemm_window: scattered C/R rows must be 16-byte aligned (ldc=64 ldr=68)"),
    ("vg_gemm_window", dict(A=None), ARG, "vg_gemm: null pointer"),
    ("vg_gemm_window", dict(K=60), ARG, "vg_gemm: K/lda/ldw/strides must be multiples of 8"),
    ("vg_gemm_window", dict(W=BUF + 8), ARG, "vg_gemm: A/W must be 16-byte aligned"),
    ("vg_gemm_window", dict(in_dtype=7), ARG, "vg_gemm: bad in_dtype 7"),
    ("vg_gemm_window", dict(out_dtype=7), UNSUPPORTED, "vg_gemm: unsupported dtype combination 1 -> 7"),
    ("vg_gemm_ln", dict(ln_w=None), ARG, "vg_gemm_ln: LayerNorm weight / bias missing"),
    ("vg_gemm_ln", dict(ln_b=None), ARG, "vg_gemm_ln: LayerNorm weight / bias missing"),
    ("vg_gemm_ln", dict(dtype=F32), UNSUPPORTED, "vg_gemm_ln: bf16 only (dtype 0)"),
    ("vg_gemm_ln", dict(M=0), ARG, "vg_gemm_ln: 0 rows"),
    ("vg_gemm_ln", dict(M=1 << 31), ARG, "vg_gemm_ln: 2147483648 rows"),
    ("vg_gemm_ln", dict(K=64, lda=64, ldw=64), UNSUPPORTED, "vg_gemm_ln: M=65536 N=64 K=64 is not a row-register shape"),
    ("vg_gemm_ln", dict(M=4096), UNSUPPORTED, "vg_gemm_ln: M=4096 N=64 K=144 is not a row-register shape"),
    ("vg_gemm_ln", dict(N=72, ldc=72), UNSUPPORTED, "vg_gemm_ln: M=65536 N=72 K=144 is not a row-register shape"),
    ("vg_gemm_ln", dict(ldc=60), UNSUPPORTED, "vg_gemm_ln: M=65536 N=64 K=144 is not a row-register shape"),
    ("vg_gemm_ln", dict(act=2), UNSUPPORTED, "vg_gemm_ln: M=65536 N=64 K=144 is not a row-register shape"),
    ("vg_gemm_ln", dict(M=70000, N=12752, ldc=12752, K=288, lda=288, ldw=288), UNSUPPORTED, "vg_gemm_ln: M=70000 N=12752 K=288 is not a row-register shape"),
    ("vg_gemm_ln", dict(window=1), UNSUPPORTED, "vg_gemm_ln: M=64 N=64 K=144 is not a row-register shape"),
    ("vg_gemm_ln", dict(window=1, ws=0), ARG, "vg_gemm_window: bad window mode=1 B=1 H=8 W=8 ws=0"),
    ("vg_gemm_ln", dict(window=1, zero_row=None), ARG, "vg_gemm_window: mode 1 needs a row of K zeros"),
    ("vg_gemm_ln", dict(window=1, H=4, Wd=4), UNSUPPORTED, "vg_gemm_window: 16 rows"),
    ("vg_gemm_ln", dict(A=None), ARG, "vg_gemm: null pointer"),
    ("vg_gemm_ln", dict(window=1, W=None), ARG, "vg_gemm: null pointer"),
    ("vg_gemm_ln", dict(N=0), ARG, "vg_gemm: bad shape M=65536 N=0 K=144 batch=1"),
    ("vg_gemm_ln", dict(K=140, lda=140, ldw=140), ARG, "vg_gemm: K/lda/ldw/strides must be multiples of 8"),
    ("vg_gemm_ln", dict(A=BUF + 8), ARG, "vg_gemm: A/W must be 16-byte aligned"),
    ("vg_gemm_splitk", dict(A=None), ARG, "vg_gemm_splitk: null pointer"),
    ("vg_gemm_splitk", dict(workspace=None), ARG, "vg_gemm_splitk: null pointer"),
    ("vg_gemm_splitk", dict(M=16), ARG, "vg_gemm_splitk: bad shape M=16 N=64 K=256 ksplit=2"),
    ("vg_gemm_splitk", dict(N=60), ARG, "vg_gemm_splitk: bad shape"),
    ("vg_gemm_splitk", dict(ksplit=1), ARG, "vg_gemm_splitk: bad shape"),
    ("vg_gemm_splitk", dict(ksplit=17), ARG, "vg_gemm_splitk: bad shape"),
    ("vg_gemm_splitk", dict(in_dtype=7), ARG, "vg_gemm_splitk: bad in_dtype 7"),
    ("vg_gemm_splitk", dict(K=252), ARG, "vg_gemm_splitk: K / lda / ldw must be multiples of 8"),
    ("vg_gemm_splitk", dict(in_dtype=F32, out_dtype=F32, ldw=254), ARG, "vg_gemm_splitk: K / lda / ldw must be multiples of 4"),
    ("vg_gemm_splitk", dict(workspace=BUF + 8), ARG, "vg_gemm_splitk: K / lda / ldw must be multiples of 8"),
    ("vg_gemm_splitk", dict(ldc=60), ARG, "vg_gemm_splitk: C rows must be 16-byte aligned"),
    ("vg_gemm_splitk", dict(C=BUF + 8), ARG, "vg_gemm_splitk: C rows must be 16-byte aligned"),
    ("vg_gemm_splitk", dict(ws_floats=100), ARG, "vg_gemm_splitk: workspace 100 < 8192 floats"),
    ("vg_gemm_splitk", dict(in_dtype=F32, out_dtype=BF16), UNSUPPORTED, "vg_gemm_splitk: unsupported dtype combination 0 -> 1"),
    ("vg_gemm_f8", dict(A8=None), ARG, "vg_gemm_f8: bad args M=64 N=64 K=64 (M > 16)"),
    ("vg_gemm_f8", dict(w_scale=None), ARG, "vg_gemm_f8: bad args"),
    ("vg_gemm_f8", dict(M=16), ARG, "vg_gemm_f8: bad args M=16"),
    ("vg_gemm_f8", dict(K=72), ARG, "vg_gemm_f8: K / lda / ldw must be multiples of 16"),
    ("vg_gemm_f8", dict(lda=72), ARG, "vg_gemm_f8: K / lda / ldw must be multiples of 16"),
    ("vg_gemm_f8", dict(W8=BUF + 8), ARG, "vg_gemm_f8: K / lda / ldw must be multiples of 16"),
    ("vg_gemm_f8", dict(out_dtype=7), ARG, "vg_gemm_f8: bad out_dtype 7"),
    ("vg_gemm_f8", dict(a_op=2), ARG, "vg_gemm_f8: a_op 2"),
    ("vg_gemm_f8", dict(a_op=1, R=BUF, ldr=64), ARG, "vg_gemm_f8: a_op 1"),
    ("vg_gemm_f8", dict(N=60), UNSUPPORTED, "vg_gemm_f8: C / R rows must be 16-byte aligned and N a multiple of 8"),
    ("vg_gemm_f8", dict(ldc=60), UNSUPPORTED, "vg_gemm_f8: C / R rows must be 16-byte aligned"),
    ("vg_gemm_f8", dict(R=BUF + 8, ldr=64), UNSUPPORTED, "vg_gemm_f8: C / R rows must be 16-byte aligned"),
]


@pytest.fixture(scope="module")
def lib():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: calls with host pointers are made only where nothing can launch")
    import __graft_entry__ as g

    g.build()
    from videoglamm_amd import _lib

    return _lib.load()


def test_every_entry_point_has_cases():
    by = {}
    for name, over, _, _ in CASES:
        assert name in ENTRIES and set(over) <= set(ENTRIES[name][0]), (name, over)
        by.setdefault(name, []).append(over)
    assert set(by) == set(ENTRIES)
    for name, overs in by.items():
        assert any(v is None for o in overs for v in o.values()), name + ": no null-pointer case"


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_refused_before_any_launch(lib, name):
    names, base = ENTRIES[name]
    for case, over, code, start in CASES:
        if case != name:
            continue
        args = dict(base, **over)
        rc = getattr(lib, name)(*[args[n] for n in names])
        msg = lib.vg_last_error().decode()
        assert rc == code, (over, rc, msg)
        assert code == OK or msg.startswith(start), (over, msg)
