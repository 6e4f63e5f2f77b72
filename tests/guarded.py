"""Guard-band / poison harness for the buffer promises of include/jdet_hip.h: inputs are never written, outputs are
fully overwritten, workspaces may hold any content, nothing is written outside a buffer.

Every buffer of a call is the middle of ONE uint8 allocation of GUARD + nbytes + GUARD bytes; the trailing guard starts
at the first byte after the payload (a 130-byte `keep` is followed by its guard at byte 130, not 132) and the GUARD-byte
lead keeps the payload 256-byte aligned.  A case is a function `fn(run)` that takes its buffers from a `Run`, calls the
entry point and returns a `Result`; `run_case` executes it twice --

  run A (clean)   outputs and workspaces zero, input guards poisoned
  run B (hostile) outputs and their guards hold a canary, workspaces 0xFF bytes (NaN as float, -1 as int), the unused
                  columns of strided inputs NaN

-- and asserts on B: guards untouched, no canary word left in an output, inputs bit-identical to their snapshot, B equal
to A bit for bit (deterministic kernels) and both within the case's bound of its reference.  A third run claims one
byte less than the workspace query while passing the full buffer: JDET_E_WORKSPACE and untouched outputs.

Fills: float input guards are quiet NaN (NaN fails every range comparison, so a stray read cannot become a wild
address); integer input guards are a small in-range value (0, or what the case passes), never a large one.

Limit: a write MORE than GUARD = 4096 bytes outside a buffer is not seen.  The targets are tile tails, vector widths
and off-by-one rows.  Works on any torch device (tests/test_guarded_cpu.py runs it on the CPU)."""
import numpy as np
import torch

GUARD = 4096
E_WORKSPACE = -3
CANARY_WORD = 0x7FC5A5A5                 # a NaN no arithmetic produces; outputs and their guards (float)
CANARY_BYTE = 0x07                       # uint8 / int32 outputs: no keep flag, label, index or count is 0x07 / 0x07070707
WS_GUARD_BYTE = 0xC3
QNAN_WORD = 0x7FC00000


class WorkspaceTooSmall(Exception):
    """raised by Run.ok in the short-workspace run when the entry point answers JDET_E_WORKSPACE"""


def _pattern(nbytes, word, dev):
    """nbytes of the little-endian 32-bit `word`, phase 0 at byte 0"""
    b = torch.tensor([(word >> (8 * k)) & 255 for k in range(4)], dtype=torch.uint8)
    return b.repeat((nbytes + 3) // 4)[:nbytes].to(dev)


def _word_of_byte(b):
    return b | (b << 8) | (b << 16) | (b << 24)


def _as_tensor(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().contiguous()
    return torch.from_numpy(np.ascontiguousarray(a))


def guarded(shape, dtype, device, fill):
    """ONE uint8 tensor of GUARD + nbytes + GUARD bytes, every byte of it the 32-bit pattern `fill`; returns
    (the middle as a `dtype` view of `shape`, the whole allocation).  The trailing guard starts at the first byte after
    the payload, whatever its size; the payload keeps the 256-byte alignment of the allocation."""
    shape = tuple(int(s) for s in shape)
    nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    raw = _pattern(GUARD + nbytes + GUARD, fill, device)
    view = raw[GUARD:GUARD + nbytes].view(dtype).view(shape) if nbytes else torch.empty(shape, dtype=dtype, device=device)
    return view, raw


class Buf:
    """one guarded allocation; `.t` is the typed payload view"""

    def __init__(self, name, kind, shape, dtype, dev, guard_word, payload_word=None, payload=None):
        self.name, self.kind, self.dtype = name, kind, dtype
        self.t, raw = guarded(shape, dtype, dev, guard_word)
        self.raw = raw
        self.nbytes = raw.numel() - 2 * GUARD
        mid = raw[GUARD:GUARD + self.nbytes]
        if payload is not None:
            mid.copy_(_as_tensor(payload).reshape(-1).view(torch.uint8).to(dev))
        elif payload_word is not None:
            mid.copy_(_pattern(self.nbytes, payload_word, dev))
        self.lead0 = raw[:GUARD].clone()
        self.trail0 = raw[GUARD + self.nbytes:].clone()
        self.snap = mid.clone() if kind in ("in", "acc") else None
        self.canary = payload_word if kind == "out" else None

    # ---- checks -------------------------------------------------------------------------------------------------
    def check_guards(self):
        for where, now, was in (("before", self.raw[:GUARD], self.lead0), ("after", self.raw[GUARD + self.nbytes:], self.trail0)):
            bad = (now != was).nonzero()
            if bad.numel():
                first = int(bad[0]) if where == "after" else int(bad[-1]) - GUARD
                raise AssertionError("guard %s %s '%s' overwritten: %d bytes, nearest at byte %+d of the payload's %s"
                                     % (where, self.kind, self.name, bad.numel(), first,
                                        "end" if where == "after" else "start"))

    def check_input(self):
        if self.kind == "in" and not torch.equal(self.raw[GUARD:GUARD + self.nbytes], self.snap):
            bad = (self.raw[GUARD:GUARD + self.nbytes] != self.snap).nonzero()
            raise AssertionError("input '%s' was written: %d bytes, first at byte %d" % (self.name, bad.numel(), int(bad[0])))

    def canary_left(self):
        """number of payload elements that still hold the canary"""
        if self.canary is None or self.nbytes == 0:
            return 0, -1
        mid = self.raw[GUARD:GUARD + self.nbytes]
        if self.dtype == torch.uint8:
            hit = mid == (self.canary & 255)
        else:
            want = self.canary - (1 << 32) if self.canary >= (1 << 31) else self.canary
            hit = mid.view(torch.int32) == want
        n = int(hit.sum())
        return n, (int(hit.nonzero()[0]) if n else -1)

    def check_written(self):
        n, first = self.canary_left()
        if n:
            raise AssertionError("canary left in output '%s': %d of %d elements unwritten, first at flat index %d"
                                 % (self.name, n, self.t.numel(), first))

    def check_untouched(self):
        n, _ = self.canary_left()
        if self.canary is not None and n != self.t.numel():
            raise AssertionError("output '%s' was touched by a call that reported an error (%d of %d elements changed)"
                                 % (self.name, self.t.numel() - n, self.t.numel()))

    def value(self):
        """what the call produced: the payload (accumulating outputs: payload - base, in float64 / exact ints)"""
        if self.kind != "acc":
            return self.t.clone()
        base = self.snap.view(self.dtype).view(self.t.shape)
        return self.t.double() - base.double() if self.dtype.is_floating_point else self.t - base


class Run:
    """hands out the buffers of one execution of a case.  mode: 'A' clean, 'B' hostile, 'short' = B with a workspace
    claim one byte too small"""

    def __init__(self, dev, mode):
        assert mode in ("A", "B", "short")
        self.dev, self.mode, self.bufs, self.ws_needs = torch.device(dev), mode, [], []

    @property
    def hostile(self):
        return self.mode != "A"

    def _add(self, b):
        self.bufs.append(b)
        return b.t

    def inp(self, name, array, guard=None):
        """guarded input holding `array`; guard: float -> quiet NaN, integer -> `guard` (default 0) in every element"""
        a = _as_tensor(array)
        if a.dtype.is_floating_point:
            word = QNAN_WORD
        else:
            g = int(guard or 0)
            assert 0 <= g < 128, "an integer guard is a small in-range value"
            word = _word_of_byte(g) if a.dtype == torch.uint8 else g
        return self._add(Buf(name, "in", a.shape, a.dtype, self.dev, word, payload=a))

    def strided(self, name, array, stride):
        """rows of `array` (n, cols) laid out with `stride` >= cols floats per row; the columns nobody may read are NaN in
        the hostile runs, 0 in run A"""
        a = np.asarray(array, np.float32)
        wide = np.full((a.shape[0], stride), np.nan if self.hostile else 0.0, np.float32)
        wide[:, :a.shape[1]] = a
        return self.inp(name, wide)

    def out(self, name, shape, dtype=torch.float32):
        """output: canary in the guards; payload canary (hostile) or zero (A)"""
        word = CANARY_WORD if dtype.is_floating_point else _word_of_byte(CANARY_BYTE)
        return self._add(Buf(name, "out", shape, dtype, self.dev, word, payload_word=word if self.hostile else 0))

    def acc(self, name, base):
        """accumulating output: a finite base the call adds onto, inside canary guards; compared as out - base"""
        a = _as_tensor(base)
        word = CANARY_WORD if a.dtype.is_floating_point else _word_of_byte(CANARY_BYTE)
        return self._add(Buf(name, "acc", a.shape, a.dtype, self.dev, word, payload=a))

    def ws(self, name, need):
        """workspace of `need` bytes (the entry point's query): (tensor, bytes to claim).  0xFF bytes when hostile"""
        need = int(need)
        self.ws_needs.append(need)
        b = Buf(name, "ws", (need,), torch.uint8, self.dev, _word_of_byte(WS_GUARD_BYTE),
                payload_word=0xFFFFFFFF if self.hostile else 0)
        return self._add(b), (need - 1 if self.mode == "short" else need)

    def ok(self, rc, what=""):
        if self.mode == "short" and rc == E_WORKSPACE:
            raise WorkspaceTooSmall(what)
        assert rc == 0, "%s returned %d" % (what or "entry point", rc)

    def buf_of(self, t):
        for b in self.bufs:
            if b.t is t:
                return b
        raise KeyError("tensor is not a buffer of this run")

    def _sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)

    def finish(self):
        self._sync()
        for b in self.bufs:
            b.check_guards()
        for b in self.bufs:
            b.check_input()
        if self.hostile:
            for b in self.bufs:
                b.check_written()

    def finish_refused(self):
        self._sync()
        for b in self.bufs:
            b.check_guards()
            b.check_input()
            b.check_untouched()


class Result:
    """what a case function returns.
    outs   : name -> output tensor (a buffer of the run; accumulating ones are compared as out - base)
    ref    : () -> {name: (reference array, bound)}; |out - ref| <= bound element-wise, bound a scalar or an array
             (atol + rtol * |ref|), 0 = equality.  The reference may be a function of the output array that returns
             the error array itself (angles compared modulo their wrap, areas of rectangles).  Evaluated once,
             after run B.
    atomic : float-atomic path: A and B are each compared with the reference instead of with each other"""

    def __init__(self, outs, ref, atomic=False):
        self.outs, self.ref, self.atomic = outs, ref, atomic


def same_bits(a, b):
    """bit-for-bit equality of two tensors (NaN payloads and signed zeros included)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def compare_runs(va, vb):
    """names of the outputs whose two runs differ in any bit"""
    return [k for k in vb if not same_bits(va[k], vb[k])]


def _judge(val, ref, bound):
    """(ok, max error, bound at that element) of |val - ref| <= bound; bound a scalar or an array of ref's shape
    (the allclose form atol + rtol * |ref|).  NaN on either side fails unless both sides are equal infinities."""
    v = val.detach().cpu().double().numpy() if isinstance(val, torch.Tensor) else np.asarray(val, np.float64)
    if callable(ref):                                      # the case's own error measure (angles modulo a wrap, areas)
        d = np.asarray(ref(v), np.float64).reshape(-1)
    else:
        r = np.asarray(ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref, np.float64)
        assert v.size == r.size, "shape %r vs reference %r" % (v.shape, r.shape)
        v, r = v.reshape(-1), r.reshape(-1)
        with np.errstate(invalid="ignore"):
            d = np.abs(v - r)
        d[v == r] = 0.0                                    # equal infinities
    if d.size == 0:
        return True, 0.0, float(np.max(bound)) if np.size(bound) else 0.0
    b = np.broadcast_to(np.asarray(bound, np.float64).reshape(-1) if np.ndim(bound) else np.float64(bound), d.shape)
    bad = ~(d <= b)                                        # NaN compares false: it fails
    if bad.any():
        k = int(np.flatnonzero(bad)[0]) if np.isnan(d[bad]).any() else int(np.argmax(np.where(bad, d - b, -np.inf)))
        if np.isnan(d).any():
            k = int(np.flatnonzero(np.isnan(d))[0])
        return False, float(d[k]), float(b[k])
    with np.errstate(divide="ignore", invalid="ignore"):
        k = int(np.argmax(np.where(b > 0, d / np.where(b > 0, b, 1.0), 0.0)))
    return True, float(d[k]), float(b[k])


def run_case(name, label, fn, dev, report=print):
    """the protocol.  Returns the printed line."""
    a = Run(dev, "A")
    ra = fn(a)
    a.finish()
    va = {k: a.buf_of(t).value() for k, t in ra.outs.items()}
    b = Run(dev, "B")
    rb = fn(b)
    b.finish()
    vb = {k: b.buf_of(t).value() for k, t in rb.outs.items()}
    differ = compare_runs(va, vb)
    refs = rb.ref()
    assert set(refs) == set(vb), "reference names %r vs outputs %r" % (sorted(refs), sorted(vb))
    worst, worst_ratio = (0.0, 0.0, ""), -1.0
    failures = []
    for run_name, vals in (("B", vb),) + ((("A", va),) if rb.atomic else ()):
        for k, (ref, bound) in refs.items():
            ok, err, at = _judge(vals[k], ref, bound)
            if not ok:
                failures.append("run %s: '%s' differs from the reference: max error %.3e > bound %.3e" % (run_name, k, err, at))
            ratio = float("inf") if not ok else (err / at if at else 0.0)
            if ratio > worst_ratio:                    # the output closest to (or furthest past) its bound
                worst, worst_ratio = (err, at, k), ratio
    line = "%-38s %-44s B==A %-5s max err %.3e (%s) bound %.3e" % (
        name, label, "n/a" if rb.atomic else ("yes" if not differ else "NO"), worst[0], worst[2], worst[1])
    report(line)
    if failures:
        raise AssertionError("%s %s: %s" % (name, label, "; ".join(failures)))
    if differ and not rb.atomic:
        raise AssertionError("%s %s: run B (poisoned buffers) differs bit for bit from run A (clean) in %r: the result "
                             "depends on the content of an output, a workspace or memory outside the inputs"
                             % (name, label, differ))
    if any(b.ws_needs):
        s = Run(dev, "short")
        try:
            fn(s)
        except WorkspaceTooSmall:
            s.finish_refused()
        else:
            raise AssertionError("%s %s: a workspace claim one byte below the query was not refused with "
                                 "JDET_E_WORKSPACE" % (name, label))
    return line
