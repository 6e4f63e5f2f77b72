"""CPU: the bf16x3 convolution forward -- its names in SIGNATURES of jdet_amd/_lib.py, the argument
checks of the entry point (they return before any launch: no GPU here), and the numerics of csrc/conv_bf16x3.hip on a
numpy restatement (tests/bf16x3_cases.py): the split is exact, and the three exactness probes pass on the six-term form
and, between them, fail when any one term is removed."""
import ctypes
import os

import numpy as np
import pytest

from tests import bf16x3_cases as BC

NAMES = {"jdet_conv3x3_bf16x3_supported", "jdet_conv3x3_bf16x3_forward"}


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
    p = (ctypes.addressof(one) + 15) & ~15
    sup = lib.jdet_conv3x3_bf16x3_supported
    assert sup(256, 256) == 1 and sup(32, 15) == 1 and sup(96, 200) == 1
    assert sup(48, 64) == 0 and sup(16, 64) == 0 and sup(0, 64) == 0 and sup(64, 0) == 0
    fwd = lib.jdet_conv3x3_bf16x3_forward
    assert fwd(p, -1, 8, 8, 64, p, 64, N, 1, N, p, N) == -1                          # N < 0
    assert fwd(p, 1, 0, 8, 64, p, 64, N, 1, N, p, N) == -1                           # H <= 0
    assert fwd(p, 1, 8, 8, 48, p, 64, N, 1, N, p, N) == -2                           # Cin % 32
    assert fwd(N, 0, 8, 8, 64, N, 64, N, 1, N, N, N) == 0                            # N == 0: nothing to do
    assert fwd(N, 1, 8, 8, 64, p, 64, N, 1, N, p, N) == -1                           # null pointers
    assert fwd(p, 1, 8, 8, 64, N, 64, N, 1, N, p, N) == -1
    assert fwd(p, 1, 8, 8, 64, p, 64, N, 1, N, N, N) == -1
    assert fwd(p + 4, 1, 8, 8, 64, p, 64, N, 1, N, p, N) == -1                       # x not 16-byte aligned
    assert fwd(p, 1, 8, 8, 64, p + 8, 64, N, 1, N, p, N) == -1                       # w not 16-byte aligned
    assert fwd(p, 1, 8, 8, 64, p, 64, N, 1, N, p + 2, N) == -1                       # y not 4-byte aligned
    assert fwd(p, 64, 512, 512, 64, p, 64, N, 1, N, p, N) == -2                      # positions * channels >= 2^30
    assert fwd(p, 64, 512, 512, 32, p, 64, N, 1, N, p, N) == -2                      # ... by Cout
    assert fwd(p, 1, 8, 8, 1 << 14, p, 1 << 14, N, 1, N, p, N) == -2                 # the weight tensor >= 2^30 elements


def test_switches_follow_the_environment():
    from jdet_amd.ops import conv_igemm as CI
    for name, value in (("JDET_CONV_BF16X3", CI.BF16X3), ("JDET_CONV_BF16X3_DGRAD", CI.BF16X3_DGRAD)):
        assert isinstance(value, bool)
        if name in os.environ:
            assert value == (os.environ[name] == "1")
    # the route takes the fp32 kernel's `big` shapes with Cin % 32 == 0 only
    assert CI.bf16x3_big(2 * 128 * 128, 256, 256) and not CI.bf16x3_big(2 * 64 * 64, 256, 256)
    assert not CI.bf16x3_big(2 * 128 * 128, 48, 256) and CI.bf16x3_big(4 * 128 * 128, 256, 15)


def test_split_is_exact_bf16_and_same_signed():
    rng = np.random.default_rng(7)
    x = np.concatenate([
        rng.standard_normal(20000).astype(np.float32),
        (rng.standard_normal(20000) * np.exp2(rng.integers(-60, 40, 20000))).astype(np.float32),
        np.asarray([0.0, -0.0, 1.0, -1.0, 1 + 2.0 ** -23, -(2 - 2.0 ** -23), 2.0 ** -100, 3.0e38], np.float32)])
    a1, a2, a3 = BC.split3(x)
    for a in (a1, a2, a3):
        assert BC.is_bf16(a)
        assert np.all((a == 0) | (np.signbit(a) == np.signbit(x)))
    assert np.array_equal(a1.astype(np.float64) + a2.astype(np.float64) + a3.astype(np.float64), x.astype(np.float64))
    assert np.array_equal((a1 + a2) + a3, x)                       # ... and in fp32, largest parts first
    assert np.all(np.abs(a2) <= np.abs(a1) * 2.0 ** -7) and np.all(np.abs(a3) <= np.abs(a1) * 2.0 ** -15)


@pytest.mark.parametrize("which", ["i", "ii", "iii"])
def test_probe_is_exact_on_the_restatement(which):
    x, w, ref = BC.probe(which)
    assert np.array_equal(BC.conv_restated(x, w).astype(np.float64), ref)


def test_probes_between_them_miss_no_term():
    """(i) needs a1b1, a2b1, a3b1; (ii) a1b1, a1b2, a1b3; (iii) a1b1, a1b2, a2b1, a2b2"""
    want = {"i": {(0, 0), (1, 0), (2, 0)}, "ii": {(0, 0), (0, 1), (0, 2)}, "iii": {(0, 0), (0, 1), (1, 0), (1, 1)}}
    caught = set()
    for which, terms in want.items():
        x, w, ref = BC.probe(which)
        for t in terms:
            y = BC.conv_restated(x, w, tuple(u for u in BC.TERMS if u != t))
            assert not np.array_equal(y.astype(np.float64), ref), (which, t)
            caught.add(t)
    assert caught == set(BC.TERMS)


def test_restatement_is_as_accurate_as_an_fp32_chain():
    """case (d), signed data: the six-term form against float64 stays inside the project bound with the headroom the
    kernel's header states, and dropping a2b2 is several times worse"""
    x, w, _, _ = BC.inputs("d")
    ref = BC.reference("d", False)
    err6 = np.abs(BC.conv_restated(x, w) - ref).max()
    err5 = np.abs(BC.conv_restated(x, w, tuple(t for t in BC.TERMS if t != (1, 1))) - ref).max()
    bound = BC.BOUND[0] * np.abs(ref).max() + BC.BOUND[1]
    print("six terms %.3e, without a2b2 %.3e, bound %.3e" % (err6, err5, bound))
    assert err6 <= bound / 5 and err5 > 2 * err6
