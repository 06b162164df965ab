"""Guard-band harness for the memory contract of the C ABI (include/hmm_engine.h, "Memory contract").

Every argument of a call lives in a buffer of its own: the argument is a window, the bytes before and after it are
margins that hold a fill pattern.  The workspace window has exactly the number of bytes the size query returns.  The
call runs once per fill, and five properties are checked (Report.violations names check, argument, byte offset):

  W1  no byte outside an output or the workspace window changes (margins, holes of strided arguments, inputs)
  W2  every element of every requested output is written: no element keeps the sentinel under both output fills, and
      the outputs are bit-identical between the two fills
  W3  outputs and the diagnostic readers do not depend on what the workspace held before the call (0x00, 0xFF, random)
  R1  outputs do not depend on the bytes around the inputs (NaN, then 3e38), holes of strided inputs included
  P   outputs are bit-identical to the ordinary engine.* wrapper call on the same data

Fills come in pairs, so that no single value can pass by coincidence.  The harness is device-agnostic:
tests/test_memory_contract_cpu.py runs it on CPU tensors against fake entry points (one per kind of violation) to show
that each check can fail; tests/test_memory_contract_gpu.py runs the table of memory_contract_table.py on the device.

The stated limit: the margins are 1 MiB on each side of the workspace and of every (k,b,L,q)-sized tensor and 64 KiB on
each side of tables, A, pi, loglik and the like.  At the table's shapes one whole sequence is under 100 KiB and one
per-wave workspace piece is 1 KiB, so a write that is off by a row, a tile, a chain or a sequence lands inside a
margin.  A stray access FARTHER from its argument than the margin is not seen, and a stray READ is seen only if it
reaches a result.

Window alignment follows the header: the workspace 256 bytes, double tensors 8 bytes (256 n + 8), everything else 256
bytes — or, with Arg(shift=...), 256 n + shift for the arguments whose kernels assume element alignment only.
"""
import struct

import torch

BIG_MARGIN = 1 << 20
SMALL_MARGIN = 64 << 10
ODD_SHIFT = 4 * 1031          # an odd float offset (tests/test_largeq_sweep_gpu.py uses the same margin)


def _bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


NAN_BITS = 0x7FC00000
OUT_FILLS = (NAN_BITS, _bits(-7.0))                 # margins and windows of float (and 4- / 8-byte integer) outputs
BYTE_OUT_FILLS = (0xA5A5A5A5, 0x5A5A5A5A)            # one-byte outputs: both float sentinels hold 0x00 bytes
IN_FILLS = (NAN_BITS, _bits(3e38))                  # margins and holes of inputs
WS_FILLS = ("zeros", "ones", "random")              # the workspace window before the call
FILLS = dict(out=OUT_FILLS, inp=IN_FILLS, ws=WS_FILLS)


class Arg:
    """One pointer argument.  kind: 'inp' (data), 'out' (shape, dtype), 'inout' (data; checked as an output too),
    'ws' (nbytes).  big: 1 MiB margins instead of 64 KiB.  mask (bool, data's shape): False marks elements inside the
    window that do not belong to the argument (the unused columns of a strided view); they are filled like a margin and,
    for outputs, must stay as they were — unless loose, for lanes the header leaves without a contract (they may be
    written, with anything).  shift: the window starts at 256 n + shift bytes (default 8 for fp64, else 0)."""

    def __init__(self, name, kind, data=None, shape=None, dtype=None, nbytes=None, big=False, mask=None, shift=None,
                 loose=False):
        assert kind in ("inp", "out", "inout", "ws")
        self.name, self.kind, self.big, self.mask, self.loose = name, kind, big, mask, loose
        if kind == "ws":
            self.shape, self.dtype, self.data = (int(nbytes),), torch.uint8, None
            self.big = True
        elif kind == "out":
            self.shape, self.dtype, self.data = tuple(shape), dtype or torch.float32, None
        else:
            self.data = data.contiguous()
            self.shape, self.dtype = tuple(data.shape), data.dtype
        self.itemsize = torch.empty((), dtype=self.dtype).element_size()
        n = 1
        for s in self.shape:
            n *= s
        self.numel, self.nbytes = n, n * self.itemsize
        self.shift = (8 if self.dtype == torch.float64 else 0) if shift is None else shift
        assert self.shift % self.itemsize == 0 or self.kind == "ws"
        assert mask is None or (mask.dtype == torch.bool and tuple(mask.shape) == self.shape)


class Violation:
    def __init__(self, check, arg, offset, text):
        self.check, self.arg, self.offset, self.text = check, arg, offset, text

    def __repr__(self):
        return "%s %s @%s: %s" % (self.check, self.arg, self.offset, self.text)


class ContractViolation(AssertionError):
    pass


class _Slot:
    def __init__(self, arg, device, margin):
        self.arg, self.margin = arg, margin
        size = (2 * margin + arg.nbytes + 512 + arg.shift + 7) // 8 * 8
        self.buf = torch.empty(size, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        assert base % 8 == 0
        self.start = margin + (-(base + margin)) % 256 + arg.shift
        self.end = self.start + arg.nbytes
        self.ptr = base + self.start
        # the mask per byte of the window
        self.mask = None if arg.mask is None else \
            arg.mask.reshape(-1, 1).expand(-1, arg.itemsize).reshape(-1).contiguous().to(device)
        self.expected = None

    def window(self):
        return self.buf[self.start:self.end]

    def typed(self):
        return self.window().view(self.arg.dtype).view(self.arg.shape)

    def prepare(self, margin_bits, window):
        """Margins (and holes) <- the 4-byte pattern; window <- data, the pattern, or a workspace pre-fill."""
        a = self.arg
        self.buf.view(torch.int32).fill_(_signed(margin_bits))
        if a.kind in ("inp", "inout"):
            self.typed().copy_(a.data)
            if self.mask is not None:
                pattern = self.buf.new_full((self.buf.numel() // 4,), 0, dtype=torch.int32).fill_(_signed(margin_bits))
                self.window()[~self.mask] = pattern.view(torch.uint8)[self.start:self.end][~self.mask]
        elif a.kind == "ws":
            w = self.window()
            if window == "zeros":
                w.zero_()
            elif window == "ones":
                w.fill_(255)
            else:
                g = torch.Generator().manual_seed(20261019)
                w.copy_(torch.randint(0, 256, (a.nbytes,), dtype=torch.uint8, generator=g))
        self.expected = self.buf.clone()

    def stray(self):
        """Offset (relative to the window) of the first byte that changed although the call may not write it."""
        a, buf, exp = self.arg, self.buf, self.expected
        writable = a.kind != "inp"
        if self.mask is None:
            if torch.equal(buf[:self.start], exp[:self.start]) and torch.equal(buf[self.end:], exp[self.end:]) \
                    and (writable or torch.equal(self.window(), exp[self.start:self.end])):
                return None
        diff = buf != exp
        if writable:
            if self.mask is None or a.loose:
                diff[self.start:self.end] = False
            else:
                diff[self.start:self.end][self.mask] = False
        bad = torch.nonzero(diff)
        return None if bad.numel() == 0 else int(bad[0]) - self.start

    def result(self):
        """A copy of the window, the holes zeroed."""
        t = self.typed().clone()
        if self.mask is not None:
            t.view(-1).view(torch.uint8)[~self.mask] = 0
        return t


def _signed(bits):
    bits &= 0xFFFFFFFF
    return bits - (1 << 32) if bits >= 1 << 31 else bits


class Arena:
    """One uint8 buffer per argument; margin_bytes overrides the per-argument margins (1 MiB / 64 KiB)."""

    def __init__(self, device, margin_bytes=None):
        self.device, self.margin_bytes, self.slots = torch.device(device), margin_bytes, {}
        self.strays = []

    def add(self, arg):
        margin = self.margin_bytes if self.margin_bytes is not None else (BIG_MARGIN if arg.big else SMALL_MARGIN)
        assert margin % 8 == 0
        self.slots[arg.name] = _Slot(arg, self.device, margin)

    # --- what a call sees
    def ptr(self, name):
        """Address of the window, or None (NULL) for an argument the row does not pass."""
        s = self.slots.get(name)
        return None if s is None else s.ptr

    def view(self, name):
        return self.slots[name].typed()

    def nbytes(self, name):
        return self.slots[name].arg.nbytes

    def check(self, after=""):
        """W1 between the calls of a sequence: records every argument with a stray write."""
        self.sync()
        for name, s in self.slots.items():
            off = s.stray()
            if off is not None and not any(n == name for n, _, _ in self.strays):
                self.strays.append((name, off, after))

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8).reshape(-1),
                                                                      b.contiguous().view(torch.uint8).reshape(-1))


def _first_difference(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return -1
    d = torch.nonzero(a.contiguous().view(torch.uint8).reshape(-1) != b.contiguous().view(torch.uint8).reshape(-1))
    return int(d[0]) if d.numel() else None


def _close(a, b, tol):
    rtol, atol = tol
    a, b = a.double(), b.double()
    return bool(((a - b).abs() <= rtol * b.abs().max() + atol).all())


class Spec:
    """One row: entry (the symbols the row exercises), route (a label), args, and optionally
      wrapper()          -> {output name: tensor} from the ordinary engine.* call on the same data (check P)
      diag(arena)        -> tuple of the diagnostic readers' values after a run (check W3, and the route assertion)
      tol                (rtol of the maximum, atol): only for an entry point whose plain repeated call is not
                         bit-identical; the tolerance of its oracle test, never a new number
      intermediate       names of outputs that the host forms between the calls of a sequence (no wrapper result)
      note               remark on the row, e.g. a call sequence that keeps a workspace region between its calls by design"""

    def __init__(self, entry, route, args, wrapper=None, diag=None, tol=None, note="", intermediate=()):
        self.entry = (entry,) if isinstance(entry, str) else tuple(entry)
        self.route, self.args, self.wrapper, self.diag, self.tol, self.note = route, list(args), wrapper, diag, tol, note
        self.intermediate = set(intermediate)    # outputs the HOST forms between the calls of a sequence: not in P

    @property
    def label(self):
        return "%s [%s]" % ("+".join(self.entry), self.route)


class Report:
    def __init__(self, spec):
        self.spec, self.violations, self.outputs, self.diag = spec, [], {}, None

    def add(self, check, arg, offset, text):
        self.violations.append(Violation(check, arg, offset, "%s: %s, argument %s, %s" % (check, self.spec.label, arg, text)))

    def checks(self):
        return sorted({(v.check, v.arg) for v in self.violations})

    def raise_if_failed(self):
        if self.violations:
            raise ContractViolation("\n".join(v.text for v in self.violations))


def _unwritten(first, second, arg, fills):
    """Elements that hold the sentinel under both output fills -> index of the first, or None."""
    def held(t, bits):
        pat = torch.tensor(list(struct.pack("<I", bits & 0xFFFFFFFF)) * 2, dtype=torch.uint8, device=t.device)
        u = t.contiguous().view(torch.uint8).reshape(arg.numel, arg.itemsize)
        return (u == pat[:arg.itemsize]).all(1)
    both = held(first, fills[0]) & held(second, fills[1])
    if arg.mask is not None:
        both &= arg.mask.reshape(-1).to(both.device)
    bad = torch.nonzero(both)
    return int(bad[0]) if bad.numel() else None


def run_contract(call, spec, fills=FILLS, device="cpu", margin_bytes=None):
    """Runs call(arena) under each fill and checks W1, W2, W3, R1 and P -> Report.  call gets the Arena: ptr(name) /
    view(name) / nbytes(name) of every argument's window (the workspace's nbytes is exactly what the size query
    returned: the row put it there), and check() to verify the margins between the calls of a sequence."""
    arena = Arena(device, margin_bytes)
    for a in spec.args:
        arena.add(a)
    rep = Report(spec)
    outs = [a for a in spec.args if a.kind in ("out", "inout")]

    def out_fills(a):
        return BYTE_OUT_FILLS if a.itemsize == 1 else fills["out"]

    def run(o, i, w):
        for s in arena.slots.values():
            a = s.arg
            if a.kind == "inp" or a.kind == "inout":
                s.prepare(fills["inp"][i], None)
            elif a.kind == "out":
                s.prepare(out_fills(a)[o], None)
            else:
                s.prepare(fills["out"][o], fills["ws"][w])
        arena.strays = []
        arena.sync()
        call(arena)
        arena.check("the last call")
        for name, off, after in arena.strays:
            kind = arena.slots[name].arg.kind
            what = "input changed or byte outside it written" if kind == "inp" else "byte outside the window written"
            rep.add("W1", name, off, "%s at byte offset %d relative to the window (fills out %d, in %d, workspace %s; "
                    "seen after %s)" % (what, off, o, i, fills["ws"][w], after))
        res = {a.name: arena.slots[a.name].result() for a in outs}
        return res, (spec.diag(arena) if spec.diag else None)

    def compare(check, base, other, what, dbase=None, dother=None):
        for a in outs:
            x, y = base[a.name], other[a.name]
            if _same_bits(x, y) or (spec.tol and _close(x, y, spec.tol)):
                continue
            off = _first_difference(x, y)
            rep.add(check, a.name, off, "output differs %s, first at byte offset %s of the window" % (what, off))
        if dbase != dother:
            rep.add(check, "diagnostics", None, "the readers differ %s: %s against %s" % (what, dbase, dother))

    base, dbase = run(0, 0, 0)
    rep.outputs, rep.diag = base, dbase
    # W2
    second, d2 = run(1, 0, 0)
    for a in outs:
        if a.kind == "out":
            idx = _unwritten(base[a.name], second[a.name], a, out_fills(a))
            if idx is not None:
                rep.add("W2", a.name, idx * a.itemsize, "element %d (byte offset %d) was not written" % (idx, idx * a.itemsize))
    compare("W2", base, second, "between the two output fills", dbase, d2)
    # R1
    other, d3 = run(0, 1, 0)
    compare("R1", base, other, "between the two input-margin fills", dbase, d3)
    # W3
    for w in range(1, len(fills["ws"])):
        other, dw = run(0, 0, w)
        compare("W3", base, other, "between the workspace pre-fills %s and %s" % (fills["ws"][0], fills["ws"][w]), dbase, dw)
    # P
    if spec.wrapper is not None:
        want = spec.wrapper()
        arena.sync()
        for a in outs:
            if a.name in spec.intermediate:
                continue
            if a.name not in want:
                rep.add("P", a.name, None, "the wrapper returned no such output")
                continue
            y = want[a.name].to(arena.device).reshape(a.shape)
            if a.mask is not None:
                y = y.contiguous().clone()
                y.view(-1).view(torch.uint8)[~arena.slots[a.name].mask] = 0
            if not (_same_bits(base[a.name], y) or (spec.tol and _close(base[a.name], y, spec.tol))):
                off = _first_difference(base[a.name], y)
                rep.add("P", a.name, off, "differs from the engine wrapper's result, first at byte offset %s" % off)
    return rep
