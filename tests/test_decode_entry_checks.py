"""What the decode entry points refuse, and how: return code and message, recorded from the library before the launch code was shared.

Every case is refused BEFORE any launch, the pointers are host allocations that a refused call never touches, and the whole module skips when a
GPU is visible — so a regression that stops refusing fails here and can never launch with host pointers on a real device."""
import ctypes

import pytest

ARG, UNSUPPORTED = -1, -3
F32, BF16 = 0, 1

_arena = ctypes.create_string_buffer(1 << 16)
BUF = (ctypes.addressof(_arena) + 255) & ~255          # 256-byte aligned; every pointer argument may alias it: nothing is read or written
BIG = 1 << 40                                          # a workspace size no shape exceeds


def entry(params, **defaults):
    """params: the C parameters in order, pointers marked '*'.  Pointers default to BUF, everything else to 0, unless given."""
    names = [p.lstrip("*") for p in params.split()]
    base = {p.lstrip("*"): (BUF if p.startswith("*") else 0) for p in params.split()}
    base.update(defaults)
    assert set(base) == set(names), set(base) ^ set(names)
    return names, base


_GEMV = dict(R=None, stream=None, norm_w=None, N=4096, K=4096, out_dtype=BF16)
_ROWS = dict(_GEMV, ldx=4096, ldy=4096, B=2)
_ROPE = dict(stream=None, norm_w=None, ldw=4096, H=32, Hkv=8, D=128, K=4096, dtype=BF16)
_ROPE_ROWS = dict(_ROPE, ldx=4096, ldq=4096, slot_stride=64 * 8 * 128, slot_rows=64, B=2)
_ATTN = dict(stream=None, H=32, Hkv=8, D=128, max_len=256, scale=0.1, ws_floats=BIG, dtype=BF16)
_ATTN_ROWS = dict(stream=None, ldqkv=3 * 32 * 96, max_len=256, slot_stride=128 * 32 * 96, slot_rows=128, H=32, Hkv=32, D=96, n_bound=64, scale=0.1,
                  ws_floats=BIG, B=2, dtype=BF16)
_ATTN2_ROWS = dict(stream=None, max_len=256, slot_stride=128 * 8 * 128, slot_rows=128, H=32, Hkv=8, D=128, n_bound=64, scale=0.1, ws_floats=BIG,
                   keys_per_wg=128, B=2, dtype=BF16)
_P_ROWS = "*x ldx *W ldw *y ldy *norm_w eps *R ldr N K B glu out_dtype *stream"
_P_W8_ROWS = "*x ldx *W8 ldw *wscale *y ldy *norm_w eps *R ldr N K B glu out_dtype *stream"
_P_ROPE = "*x *Wqkv ldw *norm_w eps *q_out *k_cache *v_cache *rope_cs *pos_dev H Hkv D K dtype *stream"
_P_ROPE_ROWS = "*x ldx *Wqkv ldw *norm_w eps *q_out ldq *k_slots *v_slots slot_stride row0 slot_rows *rope_cs *pos H Hkv D K B dtype *stream"
_P_ATTN = "*qkv *k_cache *v_cache *cos *sin *out H Hkv D max_len window scale *pos_dev *workspace ws_floats keys_per_wg dtype *stream"
_P_ATTN_ROWS = ("*qkv ldqkv *k_cache *v_cache max_len *k_slots *v_slots slot_stride row0 slot_rows *cos *sin *out H Hkv D n_bound window scale *pos "
                "kpw_min *workspace ws_floats B dtype *stream")
_P_ATTN2 = "*q *k_cache *v_cache *out H Hkv D max_len window scale *pos_dev *workspace ws_floats keys_per_wg dtype *stream"
_P_ATTN2_ROWS = ("*q *k_cache *v_cache max_len *k_slots *v_slots slot_stride row0 slot_rows *out H Hkv D n_bound window scale *pos *workspace "
                 "ws_floats keys_per_wg B dtype *stream")

ENTRIES = {
    "vg_decode_gemv": entry("*x *W ldw *y *norm_w eps *R N K glu in_dtype out_dtype *stream", **dict(_GEMV, ldw=4096, in_dtype=BF16)),
    "vg_decode_gemv_w8": entry("*x *W8 ldw *wscale *y *norm_w eps *R N K glu out_dtype *stream", **dict(_GEMV, ldw=4096)),
    "vg_decode_gemv_p13": entry("*x *W ldw *packed *scale *raw nraw *y *norm_w eps *R N K glu out_dtype *stream", **dict(_GEMV, ldw=4096, raw=None)),
    "vg_decode_gemv_w4": entry("*x *W4 ldw_bytes *scales *y *norm_w eps *R N K glu out_dtype *stream", **dict(_GEMV, ldw_bytes=128 + 2048, scales=None)),
    "vg_decode_qkv_rope": entry(_P_ROPE, **_ROPE),
    "vg_decode_qkv_rope_kv8": entry(_P_ROPE, **_ROPE),
    "vg_decode_gemv_rows": entry(_P_ROWS.replace("out_dtype", "dtype"), R=None, stream=None, norm_w=None, N=4096, K=4096, ldx=4096, ldw=4096, ldy=4096, B=2,
                                 dtype=BF16),
    "vg_decode_gemv_w8_rows": entry(_P_W8_ROWS, **dict(_ROWS, ldw=4096)),
    "vg_decode_gemv_w4_rows": entry(_P_ROWS.replace("*W ldw", "*W4 ldw_bytes"), **dict(_ROWS, ldw_bytes=128 + 2048)),
    "vg_decode_gemm_rows": entry(_P_ROWS, **dict(_ROWS, ldw=4096)),
    "vg_decode_gemm_w8_rows": entry(_P_W8_ROWS, **dict(_ROWS, ldw=4096)),
    "vg_decode_gemm_w4_rows": entry(_P_ROWS.replace("*W ldw", "*W4 ldw_bytes"), **dict(_ROWS, ldw_bytes=128 + 2048)),
    "vg_decode_qkv_rope_rows": entry(_P_ROPE_ROWS, **_ROPE_ROWS),
    "vg_decode_qkv_rope_rows_kv8": entry(_P_ROPE_ROWS, **_ROPE_ROWS),
    "vg_decode_attention": entry(_P_ATTN, **_ATTN),
    "vg_decode_attention_kv8": entry(_P_ATTN, **_ATTN),
    "vg_decode_attention_rows": entry(_P_ATTN_ROWS, **_ATTN_ROWS),
    "vg_decode_attention_rows_kv8": entry(_P_ATTN_ROWS, **_ATTN_ROWS),
    "vg_decode_attention2": entry(_P_ATTN2, **dict(_ATTN, keys_per_wg=128)),
    "vg_decode_attention2_kv8": entry(_P_ATTN2, **dict(_ATTN, keys_per_wg=128)),
    "vg_decode_attention2_rows": entry(_P_ATTN2_ROWS, **_ATTN2_ROWS),
    "vg_decode_attention2_rows_kv8": entry(_P_ATTN2_ROWS, **_ATTN2_ROWS),
    "vg_decode_layer": entry(
        "*qkv *k_cache *v_cache *cos *sin *attn_out H Hkv D max_len window scale *pos_dev *workspace ws_floats *flags *Wo ldo *resid *y_o *norm_w eps "
        "*Wgu ldgu *act *Wdown lddown *y hidden inter dtype *stream",
        stream=None, H=32, Hkv=8, D=128, max_len=256, scale=0.1, ws_floats=BIG, ldo=4096, ldgu=4096, lddown=14336, hidden=4096, inter=14336, dtype=BF16),
}

# (entry point, the arguments that differ from a call it would accept, return code, a piece of the message behind the entry point's name)
CASES = [
    ("vg_decode_gemv", dict(x=None), ARG, "bad args"),
    ("vg_decode_gemv", dict(N=0), ARG, "bad args"),
    ("vg_decode_gemv", dict(in_dtype=7), ARG, "bad in_dtype"),
    ("vg_decode_gemv", dict(K=4100), ARG, "multiples of 8"),
    ("vg_decode_gemv", dict(ldw=4100), ARG, "multiples of 8"),
    ("vg_decode_gemv", dict(W=BUF + 8), ARG, "16-byte aligned"),
    ("vg_decode_gemv", dict(K=65536, ldw=65536), UNSUPPORTED, "does not fit the LDS staging"),
    ("vg_decode_gemv", dict(in_dtype=F32, out_dtype=BF16), UNSUPPORTED, "unsupported dtype combination"),
    ("vg_decode_gemv_w8", dict(wscale=None), ARG, "bad args"),
    ("vg_decode_gemv_w8", dict(K=4104), ARG, "multiples of 16"),
    ("vg_decode_gemv_w8", dict(x=BUF + 2), ARG, "16-byte aligned"),
    ("vg_decode_gemv_w8", dict(K=40000, ldw=40000), UNSUPPORTED, "does not fit the LDS staging"),
    ("vg_decode_gemv_w8", dict(out_dtype=2), ARG, "bad out_dtype"),
    ("vg_decode_gemv_w8", dict(K=2048, ldw=2048), UNSUPPORTED, "not one of the supported row lengths"),
    ("vg_decode_gemv_p13", dict(packed=None), ARG, "bad args"),
    ("vg_decode_gemv_p13", dict(nraw=1), ARG, "bad args"),
    ("vg_decode_gemv_p13", dict(K=8192, ldw=8192), UNSUPPORTED, "not one of the supported row lengths"),
    ("vg_decode_gemv_p13", dict(ldw=4088), ARG, "at least K"),
    ("vg_decode_gemv_p13", dict(packed=BUF + 8), ARG, "16-byte aligned"),
    ("vg_decode_gemv_p13", dict(out_dtype=2), ARG, "bad out_dtype"),
    ("vg_decode_gemv_w4", dict(W4=None), ARG, "bad args"),
    ("vg_decode_gemv_w4", dict(K=2048), UNSUPPORTED, "not one of the supported row lengths"),
    ("vg_decode_gemv_w4", dict(ldw_bytes=2048), ARG, "packed rows"),
    ("vg_decode_gemv_w4", dict(ldw_bytes=2040, scales=BUF), ARG, "separate scales"),
    ("vg_decode_gemv_w4", dict(norm_w=BUF + 4), ARG, "16-byte aligned"),
    ("vg_decode_gemv_w4", dict(out_dtype=2), ARG, "bad out_dtype"),
    ("vg_decode_qkv_rope", dict(pos_dev=None), ARG, "null pointer"),
    ("vg_decode_qkv_rope", dict(D=96), UNSUPPORTED, "not covered"),
    ("vg_decode_qkv_rope", dict(K=8192), UNSUPPORTED, "not covered"),
    ("vg_decode_qkv_rope", dict(K=2048, dtype=F32), UNSUPPORTED, "not covered"),
    ("vg_decode_qkv_rope", dict(ldw=4100), ARG, "ldw a multiple of 8"),
    ("vg_decode_qkv_rope", dict(ldw=4098, dtype=F32), ARG, "ldw a multiple of 4"),
    ("vg_decode_qkv_rope", dict(Wqkv=BUF + 8), ARG, "alignment"),
    ("vg_decode_qkv_rope_kv8", dict(k_cache=None), ARG, "null pointer"),
    ("vg_decode_qkv_rope_kv8", dict(dtype=F32), UNSUPPORTED, "not covered (bf16 only)"),
    ("vg_decode_qkv_rope_kv8", dict(K=8192), UNSUPPORTED, "not covered (bf16 only)"),
    ("vg_decode_qkv_rope_kv8", dict(ldw=4100), ARG, "ldw a multiple of 8"),
    ("vg_decode_qkv_rope_kv8", dict(x=BUF + 8), ARG, "alignment"),
    ("vg_decode_gemv_rows", dict(y=None), ARG, "bad args"),
    ("vg_decode_gemv_rows", dict(B=0), ARG, "bad args"),
    ("vg_decode_gemv_rows", dict(B=17), ARG, "bad args"),
    ("vg_decode_gemv_rows", dict(K=5120), UNSUPPORTED, "bf16 rows of K"),
    ("vg_decode_gemv_rows", dict(dtype=F32), UNSUPPORTED, "bf16 rows of K"),
    ("vg_decode_gemv_rows", dict(ldx=4100), ARG, "alignment"),
    ("vg_decode_gemv_rows", dict(x=BUF + 8), ARG, "alignment"),
    ("vg_decode_gemv_rows", dict(norm_w=BUF, B=9, K=8192), UNSUPPORTED, "16-row bucket"),
    ("vg_decode_gemv_rows", dict(norm_w=BUF, B=5, K=14336), UNSUPPORTED, "8-row bucket"),
    ("vg_decode_gemv_w8_rows", dict(wscale=None), ARG, "bad args"),
    ("vg_decode_gemv_w8_rows", dict(B=0), ARG, "bad args"),
    ("vg_decode_gemv_w8_rows", dict(B=17), ARG, "bad args"),
    ("vg_decode_gemv_w8_rows", dict(K=2048), UNSUPPORTED, "not one of the supported row lengths"),
    ("vg_decode_gemv_w8_rows", dict(out_dtype=2), ARG, "bad out_dtype"),
    ("vg_decode_gemv_w8_rows", dict(ldw=4104), ARG, "alignment"),
    ("vg_decode_gemv_w8_rows", dict(norm_w=BUF, B=16, K=8192), UNSUPPORTED, "16-row bucket"),
    ("vg_decode_gemv_w8_rows", dict(norm_w=BUF, B=8, K=14336), UNSUPPORTED, "8-row bucket"),
    ("vg_decode_gemv_w4_rows", dict(x=None), ARG, "bad args"),
    ("vg_decode_gemv_w4_rows", dict(B=0), ARG, "bad args"),
    ("vg_decode_gemv_w4_rows", dict(B=17), ARG, "bad args"),
    ("vg_decode_gemv_w4_rows", dict(K=2048), UNSUPPORTED, "not one of the supported row lengths"),
    ("vg_decode_gemv_w4_rows", dict(out_dtype=2), ARG, "bad out_dtype"),
    ("vg_decode_gemv_w4_rows", dict(ldw_bytes=2048), ARG, "packed rows"),
    ("vg_decode_gemv_w4_rows", dict(ldx=4100), ARG, "alignment"),
    ("vg_decode_gemv_w4_rows", dict(norm_w=BUF, B=16, K=8192, ldw_bytes=256 + 4096), UNSUPPORTED, "16-row bucket"),
    ("vg_decode_gemm_rows", dict(B=0), ARG, "bad args"),
    ("vg_decode_gemm_rows", dict(B=17), ARG, "bad args"),
    ("vg_decode_gemm_rows", dict(W=None), ARG, "bad args"),
    ("vg_decode_gemm_rows", dict(K=2048), UNSUPPORTED, "K one of"),
    ("vg_decode_gemm_rows", dict(norm_w=BUF, K=8192, ldw=8192), UNSUPPORTED, "the norm form"),
    ("vg_decode_gemm_w8_rows", dict(B=0), ARG, "bad args"),
    ("vg_decode_gemm_w8_rows", dict(B=17), ARG, "bad args"),
    ("vg_decode_gemm_w8_rows", dict(wscale=None), ARG, "bad args"),
    ("vg_decode_gemm_w8_rows", dict(ldw=4104), ARG, "alignment"),
    ("vg_decode_gemm_w4_rows", dict(B=0), ARG, "bad args"),
    ("vg_decode_gemm_w4_rows", dict(B=17), ARG, "bad args"),
    ("vg_decode_gemm_w4_rows", dict(y=None), ARG, "bad args"),
    ("vg_decode_gemm_w4_rows", dict(ldw_bytes=2048), ARG, "packed rows"),
    ("vg_decode_qkv_rope_rows", dict(pos=None), ARG, "bad args"),
    ("vg_decode_qkv_rope_rows", dict(B=0), ARG, "bad args"),
    ("vg_decode_qkv_rope_rows", dict(B=17), ARG, "bad args"),
    ("vg_decode_qkv_rope_rows", dict(slot_rows=0), ARG, "bad args"),
    ("vg_decode_qkv_rope_rows", dict(K=8192), UNSUPPORTED, "not covered"),
    ("vg_decode_qkv_rope_rows", dict(dtype=F32), UNSUPPORTED, "not covered"),
    ("vg_decode_qkv_rope_rows", dict(ldx=4100), ARG, "ldx / ldw multiples of 8"),
    ("vg_decode_qkv_rope_rows", dict(Wqkv=BUF + 8), ARG, "ldx / ldw multiples of 8"),
    ("vg_decode_qkv_rope_rows_kv8", dict(v_slots=None), ARG, "bad args"),
    ("vg_decode_qkv_rope_rows_kv8", dict(B=0), ARG, "bad args"),
    ("vg_decode_qkv_rope_rows_kv8", dict(B=17), ARG, "bad args"),
    ("vg_decode_qkv_rope_rows_kv8", dict(K=8192), UNSUPPORTED, "not covered"),
    ("vg_decode_qkv_rope_rows_kv8", dict(dtype=F32), UNSUPPORTED, "not covered"),
    ("vg_decode_qkv_rope_rows_kv8", dict(ldw=4100), ARG, "slots must not overlap"),
    ("vg_decode_qkv_rope_rows_kv8", dict(slot_stride=64 * 8 * 128 - 8), ARG, "slots must not overlap"),
    ("vg_decode_qkv_rope_rows_kv8", dict(slot_stride=64 * 8 * 128 + 4), ARG, "slots must not overlap"),
    ("vg_decode_attention", dict(sin=None), ARG, "null pointer"),
    ("vg_decode_attention", dict(keys_per_wg=32), ARG, "keys_per_wg 32 not in"),
    ("vg_decode_attention", dict(H=30), ARG, "bad shape"),
    ("vg_decode_attention", dict(max_len=0), ARG, "bad shape"),
    ("vg_decode_attention", dict(dtype=7), ARG, "bad dtype"),
    ("vg_decode_attention", dict(window=-1), ARG, "window -1 < 0"),
    ("vg_decode_attention", dict(D=132), UNSUPPORTED, "head_dim 132 unsupported"),
    ("vg_decode_attention", dict(D=264), UNSUPPORTED, "head_dim 264 unsupported"),
    ("vg_decode_attention", dict(D=132, dtype=F32), UNSUPPORTED, "head_dim 132 unsupported"),
    ("vg_decode_attention", dict(k_cache=BUF + 8), ARG, "16-byte aligned"),
    ("vg_decode_attention", dict(ws_floats=100), ARG, "workspace 100 <"),
    ("vg_decode_attention", dict(max_len=8200), UNSUPPORTED, "max_len 8200 > 8192"),
    ("vg_decode_attention", dict(H=24), UNSUPPORTED, "H/Hkv = 3 not in"),
    ("vg_decode_attention_kv8", dict(out=None), ARG, "null pointer"),
    ("vg_decode_attention_kv8", dict(keys_per_wg=32), ARG, "keys_per_wg 32 not in"),
    ("vg_decode_attention_kv8", dict(max_len=0), ARG, "bad max_len"),
    ("vg_decode_attention_kv8", dict(window=-1), ARG, "bad max_len"),
    ("vg_decode_attention_kv8", dict(dtype=F32), UNSUPPORTED, "not covered (bf16"),
    ("vg_decode_attention_kv8", dict(H=30), UNSUPPORTED, "not covered (bf16"),
    ("vg_decode_attention_kv8", dict(H=24), UNSUPPORTED, "not covered (bf16"),
    ("vg_decode_attention_kv8", dict(D=264), UNSUPPORTED, "not covered (bf16"),
    ("vg_decode_attention_kv8", dict(D=132), UNSUPPORTED, "not covered (bf16"),
    ("vg_decode_attention_kv8", dict(v_cache=BUF + 4), ARG, "8-byte aligned"),
    ("vg_decode_attention_kv8", dict(ws_floats=100), ARG, "workspace 100 <"),
    ("vg_decode_attention_kv8", dict(max_len=8200), UNSUPPORTED, "max_len 8200 > 8192"),
    # both entry points of this pair report under the first one's name
    ("vg_decode_attention_rows", dict(B=0), ARG, "bad args"),
    ("vg_decode_attention_rows", dict(B=17), ARG, "bad args"),
    ("vg_decode_attention_rows", dict(qkv=None), ARG, "bad args"),
    ("vg_decode_attention_rows", dict(D=128), UNSUPPORTED, "not covered"),
    ("vg_decode_attention_rows_kv8", dict(B=0), ARG, "bad args"),
    ("vg_decode_attention_rows_kv8", dict(B=17), ARG, "bad args"),
    ("vg_decode_attention_rows_kv8", dict(v_cache=None), ARG, "bad args"),
    ("vg_decode_attention_rows_kv8", dict(dtype=F32), UNSUPPORTED, "not covered"),
    ("vg_decode_attention_rows_kv8", dict(slot_stride=128 * 32 * 96 - 8), ARG, "slots must not overlap"),
    ("vg_decode_attention2", dict(q=None), ARG, "null pointer"),
    ("vg_decode_attention2", dict(D=96), UNSUPPORTED, "not covered"),
    ("vg_decode_attention2", dict(keys_per_wg=64), ARG, "keys_per_wg 64 not in"),
    ("vg_decode_attention2", dict(max_len=0), ARG, "bad max_len"),
    ("vg_decode_attention2", dict(k_cache=BUF + 8), ARG, "caches: 16 bytes"),
    ("vg_decode_attention2", dict(ws_floats=100), ARG, "workspace 100 <"),
    ("vg_decode_attention2_kv8", dict(workspace=None), ARG, "null pointer"),
    ("vg_decode_attention2_kv8", dict(dtype=F32), UNSUPPORTED, "not covered"),
    ("vg_decode_attention2_kv8", dict(keys_per_wg=64), ARG, "keys_per_wg 64 not in"),
    ("vg_decode_attention2_kv8", dict(k_cache=BUF + 4), ARG, "caches: 8 bytes"),
    ("vg_decode_attention2_kv8", dict(ws_floats=100), ARG, "workspace 100 <"),
    ("vg_decode_attention2_rows", dict(B=0), ARG, "bad args"),
    ("vg_decode_attention2_rows", dict(B=17), ARG, "bad args"),
    ("vg_decode_attention2_rows", dict(k_slots=None), ARG, "bad args"),
    ("vg_decode_attention2_rows", dict(D=96), UNSUPPORTED, "not covered"),
    ("vg_decode_attention2_rows", dict(keys_per_wg=64), ARG, "keys_per_wg 64 not in"),
    ("vg_decode_attention2_rows", dict(row0=64), ARG, "row0=64"),
    ("vg_decode_attention2_rows", dict(v_slots=BUF + 8), ARG, "caches and slots: 16 bytes"),
    ("vg_decode_attention2_rows", dict(ws_floats=100), ARG, "workspace 100 <"),
    ("vg_decode_attention2_rows_kv8", dict(B=0), ARG, "bad args"),
    ("vg_decode_attention2_rows_kv8", dict(B=17), ARG, "bad args"),
    ("vg_decode_attention2_rows_kv8", dict(pos=None), ARG, "bad args"),
    ("vg_decode_attention2_rows_kv8", dict(dtype=F32), UNSUPPORTED, "not covered"),
    ("vg_decode_attention2_rows_kv8", dict(slot_stride=128 * 8 * 128 + 4), ARG, "caches and slots: 8 bytes"),
    ("vg_decode_attention2_rows_kv8", dict(ws_floats=100), ARG, "workspace 100 <"),
    ("vg_decode_layer", dict(flags=None), ARG, "null pointer"),
    ("vg_decode_layer", dict(hidden=2048), UNSUPPORTED, "0 role(s) available, 3 asked for"),
    ("vg_decode_layer", dict(inter=8192), UNSUPPORTED, "1 role(s) available, 3 asked for"),
    ("vg_decode_layer", dict(norm_w=None), ARG, "the MLP roles need"),
    ("vg_decode_layer", dict(window=-1), ARG, "bad window / max_len"),
    ("vg_decode_layer", dict(ldo=4100), ARG, "multiples of 8"),
    ("vg_decode_layer", dict(flags=BUF + 64), ARG, "flags 128"),
    ("vg_decode_layer", dict(Wdown=BUF + 8), ARG, "flags 128"),
    ("vg_decode_layer", dict(ws_floats=100), ARG, "workspace 100 <"),
    ("vg_decode_layer", dict(max_len=8200), UNSUPPORTED, "max_len 8200 > 8192"),
]
PREFIX = {"vg_decode_attention_rows_kv8": "vg_decode_attention_rows"}


@pytest.fixture(scope="module")
def lib():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: calls with host pointers are made only where nothing can launch")
    import __graft_entry__ as g

    g.build()
    from videoglamm_amd import _lib

    return _lib.load()


def test_every_touched_entry_point_has_the_named_cases():
    by = {}
    for name, over, _, _ in CASES:
        assert name in ENTRIES and set(over) <= set(ENTRIES[name][0]), (name, over)
        by.setdefault(name, []).append(over)
    assert set(by) == set(ENTRIES)
    for name, overs in by.items():
        assert any(v is None for o in overs for v in o.values()), name + ": no null-pointer case"
        if "B" in ENTRIES[name][0]:
            assert {0, 17} <= {o.get("B") for o in overs}, name + ": B = 0 and 17"


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_refused_before_any_launch(lib, name):
    names, base = ENTRIES[name]
    for case, over, code, piece in CASES:
        if case != name:
            continue
        args = dict(base, **over)
        rc = getattr(lib, name)(*[args[n] for n in names])
        msg = lib.vg_last_error().decode()
        assert rc == code, (over, rc, msg)
        assert msg.startswith(PREFIX.get(name, name) + ": "), (over, msg)
        assert piece in msg, (over, msg)
