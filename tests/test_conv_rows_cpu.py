"""CPU: the row-sparse convolution gradients -- their names in SIGNATURES of jdet_amd/_lib.py and the argument checks of
the three entry points, which return before any launch (no GPU here)."""
import ctypes
import os

import pytest



@pytest.fixture(scope="module")
def built_lib():
    from jdet_amd import _lib
    import shutil
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        _lib.build()
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libjdet_hip.so not built and hipcc absent")
    return _lib


def test_header_signatures_and_exports_agree(built_lib):
    assert {"jdet_rows_nonzero_workspace", "jdet_rows_nonzero", "jdet_conv3x3_rows_supported", "jdet_conv3x3_wgrad_rows",
            "jdet_conv3x3_wgrad_rows_workers", "jdet_conv3x3_dgrad_rows"} <= set(built_lib.SIGNATURES)


def test_argument_checks_return_before_any_launch(built_lib):
    lib = built_lib.lib()
    N = None
    one = ctypes.create_string_buffer(64)
    p = ctypes.addressof(one) & ~15
    assert lib.jdet_rows_nonzero_workspace(0, 8, 8) == 0
    assert lib.jdet_rows_nonzero_workspace(2, 13, 17) == 448 + 2 * 4 * 2          # P rounded up to 16 + 2 counts per 256 rows
    assert lib.jdet_rows_nonzero_workspace(2, 128, 128) == 32768 + 8 * 128
    assert lib.jdet_rows_nonzero(N, 0, 8, 8, 64, N, N, N, N, N, 0, N) == -1                  # N <= 0
    assert lib.jdet_rows_nonzero(N, 1, 8, 8, 6, N, N, N, N, N, 0, N) == -2                   # C % 4
    assert lib.jdet_rows_nonzero(N, 1, 8, 8, 64, N, N, N, N, N, 0, N) == -1                  # null pointers
    assert lib.jdet_rows_nonzero(N, 64, 512, 512, 256, N, N, N, N, N, 0, N) == -2            # P * C >= 2^30
    assert lib.jdet_rows_nonzero(p, 1, 8, 8, 64, p, p, p, p, N, 0, N) == -3                  # no workspace
    assert lib.jdet_rows_nonzero(p, 1, 8, 8, 64, p, p, p, p, p, 71, N) == -3                 # one byte short of 64 + 8
    assert lib.jdet_conv3x3_rows_supported(256, 256) == 1 and lib.jdet_conv3x3_rows_supported(32, 64) == 1
    assert lib.jdet_conv3x3_rows_supported(6, 64) == 0 and lib.jdet_conv3x3_rows_supported(64, 8) == 0
    assert lib.jdet_conv3x3_wgrad_rows_workers(256, 256) == 16 and lib.jdet_conv3x3_wgrad_rows_workers(64, 8) == 0
    assert 8 <= lib.jdet_conv3x3_wgrad_rows_workers(64, 64) <= 64
    assert lib.jdet_conv3x3_wgrad_rows(N, N, N, N, 1, 8, 8, 64, 8, N, N) == -2               # Cout % 16
    assert lib.jdet_conv3x3_wgrad_rows(N, N, N, N, 1, 8, 8, 64, 64, N, N) == -1              # null pointers
    assert lib.jdet_conv3x3_wgrad_rows(N, N, N, N, 1, 0, 8, 64, 64, N, N) == -1              # H <= 0
    assert lib.jdet_conv3x3_wgrad_rows(p, p, p, p, 64, 512, 512, 256, 256, p, N) == -2       # 32-bit byte offsets
    assert lib.jdet_conv3x3_dgrad_rows(N, N, N, N, 1, 8, 8, 6, 64, 1, N, N) == -2            # Cin % 4
    assert lib.jdet_conv3x3_dgrad_rows(N, N, N, N, 1, 8, 8, 64, 64, 1, N, N) == -1           # null pointers
    assert lib.jdet_conv3x3_dgrad_rows(p + 4, p, p, p, 1, 8, 8, 64, 64, 1, p, N) == -1       # gy not 16-byte aligned
    assert lib.jdet_conv3x3_dgrad_rows(p, p, p, p, 64, 512, 512, 256, 256, 1, p, N) == -2    # 32-bit byte offsets


def test_row_sparse_flag_is_set_on_the_regression_towers_only():
    """S2ANetHead: fam_reg_convs / odm_reg_convs carry the routing hint, the classification towers do not; the module
    switch follows JDET_CONV_ROWS (default on)"""
    from jdet_amd.config.named import S2ANET_CFG
    from jdet_amd.models.utils.modules import ConvModule
    from jdet_amd.ops import conv_igemm as CI
    from jdet_amd.utils.registry import MODELS, build_from_cfg
    assert ConvModule(8, 8, 3, padding=1).row_sparse_grad is False
    head = build_from_cfg(S2ANET_CFG["model"], MODELS).bbox_head
    assert all(m.row_sparse_grad for m in list(head.fam_reg_convs) + list(head.odm_reg_convs))
    assert not any(m.row_sparse_grad for m in list(head.fam_cls_convs) + list(head.odm_cls_convs))
    assert CI.ROWS == (os.environ.get("JDET_CONV_ROWS", "1") == "1")
