"""The decode launchers' work split (row pairs per wave, workgroups) and the B-row bucket ladder, pinned without a GPU.

tests/decode_launch_split_main.cpp is built with the host compiler alone and prints `ppw blocks` for every case; the expected values are a
transcription of the launchers' formulas below, plus the real decoder shapes by literal value.  A wrong split is invisible to the bit-identity
tests (which wave owns which pair does not enter the sums) and only costs time, so it is pinned here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")       # the Makefile's compiler; -x c++: host code only
NPAIR = 66000
PAIR_CAPS = (64, 64, 8)          # DEC_MAX_PPW, DEC4_MAX_PPW, and a cap that binds inside the range
ROWS_CAP = 8                     # DEC_ROWS_PPW = DEC4_ROWS_PPW


def pair_split(npair, wg_per_cu, max_ppw):
    """launch_decode_gemv's split: spread the pairs over wg_per_cu workgroups per CU (256 CUs, 4 waves), prefer whole rounds of 256 workgroups."""
    maxw = 256 * wg_per_cu * 4
    ppw = (npair + maxw - 1) // maxw
    for c in range(ppw, 2 * ppw + 1):
        if ((npair + 4 * c - 1) // (4 * c)) % 256 == 0 and npair % (4 * c) == 0:
            ppw = c
            break
    ppw = min(ppw, max_ppw)
    return ppw, (npair + 4 * ppw - 1) // (4 * ppw)


def rows_split(npair, phased, max_ppw):
    """launch_rows_b's split: ~2 workgroups per CU, one pair per wave when the x rows are staged in phases."""
    ppw = 1 if phased else min((npair + 2047) // 2048, max_ppw)
    return ppw, (npair + 4 * ppw - 1) // (4 * ppw)


def bucket(B):
    return 1 if B <= 1 else 2 if B <= 2 else 4 if B <= 4 else 8 if B <= 8 else 16


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("split") / "decode_launch_split")
    src = os.path.join(ROOT, "tests", "decode_launch_split_main.cpp")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-Wall", src, "-o", exe])
    return subprocess.check_output([exe]).decode().split("\n")


def test_every_split_and_the_ladder_match_the_formulas(printed):
    want = []
    for wg in (2, 4):
        for cap in PAIR_CAPS:
            for n in range(1, NPAIR + 1):
                ppw, blocks = pair_split(n, wg, cap)
                assert 1 <= ppw <= cap and 4 * ppw * blocks >= n and 4 * ppw * (blocks - 1) < n, (n, wg, cap, ppw, blocks)
                want.append("%d %d" % (ppw, blocks))
    for phased in (0, 1):
        for n in range(1, NPAIR + 1):
            ppw, blocks = rows_split(n, phased, ROWS_CAP)
            assert 1 <= ppw <= ROWS_CAP and 4 * ppw * blocks >= n and 4 * ppw * (blocks - 1) < n, (n, phased, ppw, blocks)
            want.append("%d %d" % (ppw, blocks))
    want += [str(bucket(B)) for B in range(1, 17)]
    want.append("")          # the last newline
    assert len(printed) == len(want)
    bad = [i for i, (a, b) in enumerate(zip(printed, want)) if a != b]
    assert not bad, (len(bad), bad[0], printed[bad[0]], want[bad[0]])


# (npair, 2 workgroups per CU: bf16 / p13 / q|k|v rope / chain roles, 4 per CU: fp8 / MXFP4, B-row whole rows, B-row phased)
REAL = {
    "llama3_o_4096": (2048, (1, 512), (1, 512), (1, 512), (1, 512)),
    "llama3_qkv_6144": (3072, (3, 256), (1, 768), (2, 384), (1, 768)),
    "llama3_gate_up_14336_glu": (14336, (7, 512), (7, 512), (7, 512), (1, 3584)),
    "llama3_lm_head_128256": (64128, (32, 501), (16, 1002), (8, 2004), (1, 16032)),
    "phi3_o_3072": (1536, (1, 384), (1, 384), (1, 384), (1, 384)),
    "phi3_qkv_9216": (4608, (3, 384), (2, 576), (3, 384), (1, 1152)),
    "phi3_gate_up_8192_glu": (8192, (4, 512), (2, 1024), (4, 512), (1, 2048)),
    "phi3_lm_head_32064": (16032, (8, 501), (4, 1002), (8, 501), (1, 4008)),
}


@pytest.mark.parametrize("shape", sorted(REAL))
def test_real_decoder_shapes_by_value(printed, shape):
    npair, wg2, wg4, whole, phased = REAL[shape]
    line = lambda block, n: tuple(int(v) for v in printed[block * NPAIR + n - 1].split())
    assert line(0, npair) == wg2 and line(1, npair) == wg2          # 2 per CU, cap 64 (both names)
    assert line(3, npair) == wg4 and line(4, npair) == wg4          # 4 per CU
    assert line(6, npair) == whole and line(7, npair) == phased
    assert pair_split(npair, 2, 64) == wg2 and pair_split(npair, 4, 64) == wg4
    assert rows_split(npair, 0, ROWS_CAP) == whole and rows_split(npair, 1, ROWS_CAP) == phased


def test_bucket_ladder_by_value(printed):
    assert [int(v) for v in printed[8 * NPAIR:8 * NPAIR + 16]] == [1, 2, 4, 4, 8, 8, 8, 8, 16, 16, 16, 16, 16, 16, 16, 16]
