"""CPU: the row-sparse convolution forward -- its names in SIGNATURES of jdet_amd/_lib.py and the
argument checks of its entry points, which return before any launch (no GPU here)."""
import ctypes
import os

import pytest

NAMES = {"jdet_rows_from_flags_workspace", "jdet_rows_from_flags", "jdet_conv3x3_rows_forward_supported",
         "jdet_conv3x3_rows_forward"}


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
    assert NAMES <= set(built_lib.SIGNATURES)


def test_argument_checks_return_before_any_launch(built_lib):
    lib = built_lib.lib()
    N = None
    one = ctypes.create_string_buffer(64)
    p = ctypes.addressof(one) & ~15
    if p < ctypes.addressof(one):
        p += 16
    # ---- jdet_rows_from_flags ----
    assert lib.jdet_rows_from_flags_workspace(0, 8, 8) == 0
    assert lib.jdet_rows_from_flags_workspace(2, 13, 17) == 2 * 448 + 4 * 4 * 2   # two dilated flag maps + 4 counts per 256 rows
    assert lib.jdet_rows_from_flags_workspace(2, 128, 128) == 2 * 32768 + 16 * 128
    assert lib.jdet_rows_from_flags(N, 0, 8, 8, N, N, N, N, N, 0, N) == -1                   # N <= 0
    assert lib.jdet_rows_from_flags(N, 1, 8, 8, N, N, N, N, N, 0, N) == -1                   # null pointers
    assert lib.jdet_rows_from_flags(p, 1, 8, 8, p, p, N, p, p, 1 << 20, N) == -1             # one null list
    assert lib.jdet_rows_from_flags(p, 1 << 10, 1 << 10, 1 << 10, p, p, p, p, p, 1 << 40, N) == -2   # P >= 2^30
    assert lib.jdet_rows_from_flags(p, 1, 8, 8, p + 2, p, p, p, p, 1 << 20, N) == -1         # a list not 4-byte aligned
    assert lib.jdet_rows_from_flags(p, 1, 8, 8, p, p, p, p, N, 0, N) == -3                   # no workspace
    assert lib.jdet_rows_from_flags(p, 1, 8, 8, p, p, p, p, p, 2 * 64 + 16 - 1, N) == -3     # one byte short of 128 + 16
    # ---- jdet_conv3x3_rows_forward ----
    sup = lib.jdet_conv3x3_rows_forward_supported
    assert sup(256, 256) == 1 and sup(32, 64) == 1 and sup(16, 16) == 1
    assert sup(6, 64) == 0 and sup(64, 8) == 0 and sup(0, 64) == 0
    fwd = lib.jdet_conv3x3_rows_forward
    assert fwd(N, N, N, 1, N, N, N, 0, 8, 8, 64, 64, 1, N, N) == -1                          # N <= 0
    assert fwd(N, N, N, 1, N, N, N, 1, 8, 8, 6, 64, 1, N, N) == -2                           # C % 4
    assert fwd(N, N, N, 1, N, N, N, 1, 8, 8, 64, 24, 1, N, N) == -2                          # Cout % 16
    assert fwd(N, N, N, 1, N, N, N, 1, 8, 8, 64, 64, 1, N, N) == -1                          # null pointers
    assert fwd(p, p, N, 1, N, p, N, 1, 8, 8, 64, 64, 1, p, N) == -1                          # no count
    assert fwd(p, p, N, 1, N, p, p, 1, 8, 8, 64, 64, 1, N, N) == -1                          # no output
    assert fwd(p + 4, p, N, 1, N, p, p, 1, 8, 8, 64, 64, 1, p, N) == -1                      # x not 16-byte aligned
    assert fwd(p, p, N, 1, N, p, p, 64, 512, 512, 256, 256, 1, p, N) == -2                   # P * C >= 2^30
    assert fwd(p, p, N, 1, N, p, p, 64, 512, 512, 64, 256, 1, p, N) == -2                    # P * Cout >= 2^30


def test_switches_follow_the_environment():
    """JDET_CONV_ROWS_FWD (default on) switches the forward route alone; the route also needs JDET_CONV_ROWS"""
    from jdet_amd.ops import conv_igemm as CI
    assert CI.ROWS_FWD == (os.environ.get("JDET_CONV_ROWS_FWD", "1") == "1")
    import torch
    conv = torch.nn.Conv2d(64, 64, 3, padding=1)
    assert CI.rows_tower_applicable([conv], torch.zeros(1, 64, 8, 8)) is False          # a CPU tensor: the dense route
