"""The B-row MXFP4 GEMV's row-length query (host code of the library: no GPU): prompts.generate_prompts opens the batched route of an mxfp4
decoder from it, so it must name exactly the four row lengths of the format's kernels."""
from videoglamm_amd import ops


def test_w4_rows_supported_row_lengths():
    for K in (3072, 4096, 8192, 14336):
        assert ops.decode_gemv_w4_rows_supported(K) is True
    for K in (1024, 2048, 5120, 6144, 16384):
        assert ops.decode_gemv_w4_rows_supported(K) is False


def test_w4_rows_row_lengths_are_the_single_row_kernels():
    assert sorted(ops.MXFP4_K) == [K for K in range(1024, 16385, 1024) if ops.decode_gemv_w4_rows_supported(K)]
