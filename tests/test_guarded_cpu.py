"""tests/guarded.py bites: a fake entry point written with torch CPU ops passes the protocol, and each of its mutants --
a store past the output, a store before it, an unwritten last row, an over-read that enters the arithmetic with weight
zero, a store into an input, scratch assumed zero, a too-small workspace accepted -- fails it with the matching
message.  And nothing is left out: every symbol of the C ABI is a row of tests/abi_cases.py or one of the fixed
exemptions."""
import fnmatch

import numpy as np
import pytest
import torch

from tests import guarded as G

ROWS, COLS = 5, 3            # a 60-byte output: no multiple of 16


def _raw(t, first, n):
    """n elements of t's ALLOCATION starting `first` elements from the payload's start (negative: the lead guard)"""
    return torch.as_strided(t, (n,), (1,), t.storage_offset() + first)


def _fake(mutant=None, zero_ws=False, accept_small_ws=False):
    """out (ROWS, COLS) = 2 * x + bias[col], staged through a workspace like a two-pass kernel"""
    x0 = np.arange(ROWS * COLS, dtype=np.float32).reshape(ROWS, COLS) - 4.0
    bias0 = np.asarray([0.5, -1.0, 2.0], np.float32)

    def fn(run):
        x = run.inp("x", x0)
        bias = run.inp("bias", bias0)
        out = run.out("out", (ROWS, COLS))
        ws, ws_bytes = run.ws("scratch", 4 * ROWS * COLS)
        if ws_bytes < 4 * ROWS * COLS and not accept_small_ws:
            run.ok(G.E_WORKSPACE, "fake")
        stage = ws.view(torch.float32).view(ROWS, COLS)
        if zero_ws:
            stage += 2 * x                      # a partial-sum buffer nobody cleared
        else:
            stage.copy_(2 * x)
        rows = ROWS - 1 if mutant == "skip_last_row" else ROWS
        out[:rows] = stage[:rows] + bias
        if mutant == "write_past":
            _raw(out, ROWS * COLS, 1)[0] = 1.0
        if mutant == "write_before":
            _raw(out, -1, 1)[0] = 1.0
        if mutant == "zero_times_neighbour":
            out[0, 0] += 0.0 * _raw(x, -1, 1)[0]       # a tap with weight zero just outside the input
        if mutant == "write_input":
            x[1, 1] = 7.0
        run.ok(0, "fake")
        return G.Result({"out": out}, lambda: {"out": (2.0 * x0.astype(np.float64) + bias0, 0.0)})

    return fn


def _run(fn):
    lines = []
    G.run_case("fake_entry", "(5,3)", fn, "cpu", report=lines.append)
    return lines


def test_correct_fake_passes_and_prints_one_line():
    (line,) = _run(_fake())
    assert "fake_entry" in line and "B==A yes" in line and "bound" in line


@pytest.mark.parametrize("mutant,message", [
    ("write_past", r"guard after out 'out' overwritten: 4 bytes, nearest at byte \+0 of the payload's end"),
    ("write_before", r"guard before out 'out' overwritten: 4 bytes, nearest at byte -1 of the payload's start"),
    ("skip_last_row", r"canary left in output 'out': 3 of 15 elements unwritten, first at flat index 12"),
    ("zero_times_neighbour", r"'out' differs from the reference: max error nan"),
    ("write_input", r"input 'x' was written: 2 bytes, first at byte 18"),
])
def test_mutant_is_rejected_for_the_right_reason(mutant, message):
    with pytest.raises(AssertionError, match=message):
        _run(_fake(mutant))


def test_fake_that_needs_a_zeroed_workspace_is_rejected():
    with pytest.raises(AssertionError, match=r"run B: 'out' differs from the reference: max error nan"):
        _run(_fake(zero_ws=True))


def test_fake_that_accepts_a_short_workspace_is_rejected():
    with pytest.raises(AssertionError, match="one byte below the query was not refused"):
        _run(_fake(accept_small_ws=True))


def test_byte_exact_guards_and_alignment():
    view, raw = G.guarded((130,), torch.uint8, "cpu", 0x07070707)
    assert raw.dtype == torch.uint8 and raw.numel() == 4096 + 130 + 4096 and view.data_ptr() == raw.data_ptr() + 4096
    assert bool((raw == 7).all()) and view.shape == (130,)
    r = G.Run("cpu", "B")
    keep = r.out("keep", (130,), torch.uint8)
    b = r.buf_of(keep)
    assert b.raw.numel() == 4096 + 130 + 4096 and keep.data_ptr() - b.raw.data_ptr() == 4096
    assert bool((keep == 0x07).all())
    b.raw[4096 + 130] = 1                  # the very first byte after an odd-sized payload
    with pytest.raises(AssertionError, match=r"guard after out 'keep' overwritten: 1 bytes, nearest at byte \+0"):
        r.finish()
    f = r.out("y", (7, 15))
    assert f.data_ptr() % 256 == r.buf_of(f).raw.data_ptr() % 256          # a 4096-byte lead keeps the alignment
    assert bool((f.view(torch.int32) == G.CANARY_WORD).all()) and bool(torch.isnan(f).all())
    idx = r.inp("order", np.arange(9, dtype=np.int32))
    assert bool((r.buf_of(idx).raw[:4096].view(torch.int32) == 0).all())   # integer guards: in range, wrong
    s = r.strided("boxes", np.ones((3, 5), np.float32), 6)
    assert bool(torch.isnan(s[:, 5]).all()) and bool((s[:, :5] == 1).all())
    w, claim = G.Run("cpu", "short").ws("ws", 64)
    assert claim == 63 and w.numel() == 64 and bool((w == 0xFF).all())


def test_same_bits_sees_signed_zero_and_nan_payloads():
    a = torch.tensor([0.0, float("nan")])
    assert G.same_bits(a, a.clone())
    assert not G.same_bits(a, torch.tensor([-0.0, float("nan")]))
    assert G.compare_runs({"y": a}, {"y": a.clone()}) == []


# the two *_rows names are size queries; a "*_rows" pattern would also take in jdet_conv3x3_wgrad_rows / _dgrad_rows,
# which launch kernels
EXEMPT_PATTERNS = ("jdet_version", "*_workspace", "*_supported", "jdet_conv_bn_sums_rows",
                   "jdet_bn_act_backward_from_output_rows", "jdet_conv3x3_wgrad_rows_workers", "*_bytes", "jdet_zero_fill",
                   "jdet_graph_replace_memset_nodes", "jdet_roi_align_*", "jdet_roi_spatial_order")


def test_every_entry_point_is_a_row_or_exempt():
    from tests import abi_cases
    from jdet_amd import _lib
    covered = set()
    for case in abi_cases.CASES:
        covered.update(case.entry_points)
    assert covered <= set(_lib.SIGNATURES), sorted(covered - set(_lib.SIGNATURES))
    exempt = {n for n in _lib.SIGNATURES if any(fnmatch.fnmatchcase(n, p) for p in EXEMPT_PATTERNS)}
    missing = sorted(set(_lib.SIGNATURES) - covered - exempt)
    assert not missing, "entry points without a row in tests/abi_cases.py: %s" % missing
    ids = [c.id for c in abi_cases.CASES]
    assert len(ids) == len(set(ids))


class _DryLib:
    """libjdet_hip.so with every launching entry point replaced by an argument check against _lib.SIGNATURES that
    reports success; the host-only size and capability queries are the real ones"""

    def __init__(self, real, signatures, called):
        self._real, self._sig, self._called = real, signatures, called

    def __getattr__(self, name):
        if any(fnmatch.fnmatchcase(name, p) for p in EXEMPT_PATTERNS):
            return getattr(self._real, name)
        _, argtypes = self._sig[name]

        def call(*args):
            assert len(args) == len(argtypes), "%s: %d arguments for %d parameters" % (name, len(args), len(argtypes))
            for k, (a, t) in enumerate(zip(args, argtypes)):
                try:
                    t.from_param(a)
                except Exception as e:  # noqa: BLE001
                    raise AssertionError("%s: argument %d (%r) is no %s: %s" % (name, k, a, t.__name__, e))
            self._called.add(name)
            return 0
        return call


def test_every_row_builds_without_a_gpu_and_calls_what_it_names(monkeypatch):
    """each builder runs on host buffers against the argument checker: the argument lists fit the ctypes signatures,
    the reference evaluates, and it has the size of the outputs with finite non-negative bounds"""
    from tests import abi_cases
    from jdet_amd import _lib
    _lib.build()
    for case in abi_cases.CASES:
        called = set()
        monkeypatch.setattr(abi_cases, "lib", lambda called=called: _DryLib(_lib.lib(), _lib.SIGNATURES, called))
        run = G.Run("cpu", "A")
        res = case.fn(run)
        assert called == set(case.entry_points), (case.id, sorted(called))
        refs = res.ref()
        assert set(refs) == set(res.outs), case.id
        for k, (ref, bound) in refs.items():
            b = np.asarray(bound, np.float64)
            assert np.isfinite(b).all() and (b >= 0).all(), (case.id, k)
            if callable(ref):                # the case's own error measure: one error per bound
                err = np.asarray(ref(np.zeros(tuple(res.outs[k].shape))))
                assert b.ndim == 0 or b.size == err.size, (case.id, k)
                continue
            assert np.asarray(ref).size == res.outs[k].numel(), (case.id, k, np.asarray(ref).shape, tuple(res.outs[k].shape))
            assert b.ndim == 0 or b.size == res.outs[k].numel(), (case.id, k)
            assert np.isfinite(np.asarray(ref, np.float64)).all(), (case.id, k)
        run.bufs[0].check_guards()
