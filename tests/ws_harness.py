"""Guard-banded, poisoned buffers for the workspace contracts of the C ABI (plain helpers: no fixtures, nothing pytest collects).

Every device entry point that takes a caller-owned workspace promises a size (`ww_*_workspace_bytes` / `ww_*_scratch_bytes`) and
nothing about the content.  Three things follow, and each is checked by bit equality:
  content independence   the outputs do not depend on what the workspace held on entry (a 0x00 fill against a 0xFF fill)
  stale independence     nor on what a larger launch left in it
  bounds                 nothing is written outside the queried size, or outside an output

`Guarded` is one uint8 buffer: [guard of 0xA5][interior of `fill`][guard of 0xA5], the interior aligned as the header asks and EXACTLY
nbytes long, so the first byte past the promise is a guard byte.  Outputs are served the same way through `view`.

Fills: 0x00 and 0xFF only.  0xFF is a negative quiet NaN as float32 / float64 and -1 as any integer: used as an index it lands in the
front guard, inside this allocation.  A large finite pattern would point far outside it and is deliberately not on the list.
"""
from __future__ import annotations

import torch

GUARD_BYTE = 0xA5
FILLS = (0x00, 0xFF)
OUT_FILL = 0xFF                  # what an output holds before the call: an element the call leaves unwritten reads back as NaN / -1


class Guarded:
    """`Guarded(nbytes, fill, align=256, guard=4096)`: [guard][interior: nbytes of `fill`][guard] in one torch.uint8 buffer on `device`.
    `.ptr` is the address of the interior (a multiple of `align`), `.interior` its uint8 view, `.intact()` true iff every byte outside
    the interior still holds 0xA5."""

    def __init__(self, nbytes, fill, align=256, guard=4096, device=None):
        nbytes, align, guard = int(nbytes), int(align), int(guard)
        if nbytes < 0 or align < 1 or guard < 1 or not 0 <= int(fill) <= 255:
            raise ValueError(f"Guarded({nbytes}, {fill}, align={align}, guard={guard})")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.nbytes, self.fill, self.align, self.guard = nbytes, int(fill), align, guard
        # `align` bytes of slack so that the interior can be aligned wherever the allocation starts; the slack counts as guard
        self.raw = torch.full((guard + nbytes + guard + align,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.start = guard + (-(self.raw.data_ptr() + guard)) % align
        self.interior = self.raw[self.start:self.start + nbytes]
        self.interior.fill_(self.fill)
        self.ptr = self.raw.data_ptr() + self.start
        assert self.ptr % align == 0 and self.start >= guard and self.start + nbytes + guard <= self.raw.numel()

    @classmethod
    def for_output(cls, shape, dtype, device=None, fill=OUT_FILL, align=256, guard=4096):
        """A guarded buffer of exactly prod(shape) elements of `dtype`: the element after the last one is a guard byte."""
        n = 1
        for s in shape:
            n *= int(s)
        g = cls(n * torch.empty(0, dtype=dtype).element_size(), fill, align=align, guard=guard, device=device)
        g.shape, g.dtype = tuple(int(s) for s in shape), dtype
        return g

    @classmethod
    def holding(cls, tensor, align=256, guard=4096):
        """A guarded copy of an input tensor (contiguous): for inputs the header says nothing writes."""
        t = tensor.contiguous()
        g = cls.for_output(t.shape, t.dtype, device=t.device, fill=0, align=align, guard=guard)
        g.view().copy_(t)
        return g

    def view(self, dtype=None, shape=None):
        """The interior as a typed tensor (no copy): of for_output's dtype and shape, or the given ones, from the interior's first byte."""
        dtype = dtype if dtype is not None else self.dtype
        shape = shape if shape is not None else self.shape
        n = 1
        for s in shape:
            n *= int(s)
        size = n * torch.empty(0, dtype=dtype).element_size()
        if size > self.nbytes:
            raise ValueError(f"a view of {size} bytes does not fit an interior of {self.nbytes}")
        return self.interior[:size].view(dtype).view(*shape)

    def refill(self, fill=None, start=0, stop=None):
        """Fill interior[start:stop] with `fill` (default: the fill it was made with)."""
        self.interior[start:self.nbytes if stop is None else stop].fill_(self.fill if fill is None else int(fill))

    def bytes(self):
        """A copy of the interior, uint8."""
        return self.interior.clone()

    def intact(self) -> bool:
        front, back = self.raw[:self.start], self.raw[self.start + self.nbytes:]
        return bool((front == GUARD_BYTE).all()) and bool((back == GUARD_BYTE).all())

    def touched(self, start=0) -> bool:
        """True iff some byte of interior[start:] no longer holds the fill: the call really used the buffer it was handed."""
        return bool((self.interior[start:] != self.fill).any())


class Case:
    """One entry point at one shape.
      name        for messages
      size_query  () -> the workspace bytes the library asks for
      call        (ws_ptr, ws_bytes, outs) -> None: the C ABI call(s) on the harness's buffers; outs = what make_outs returned
      make_outs   () -> {name: Guarded}: fresh guarded output buffers
      wrapper     () -> {name: tensor} (optional): what the ordinary wrapper returns for the same inputs; names missing here are
                  compared between the fills only
      poison_from (optional) the first interior byte the harness fills: the bytes before it are a region the CALLER writes
      prepare     (ws) -> None (optional): writes that caller-owned region
      inputs      {name: Guarded} (optional): guarded inputs that the call must leave bit for bit as they are"""

    def __init__(self, name, size_query, call, make_outs, wrapper=None, poison_from=0, prepare=None, inputs=None, align=256):
        self.name, self.size_query, self.call, self.make_outs = name, size_query, call, make_outs
        self.wrapper, self.poison_from, self.prepare, self.inputs, self.align = wrapper, int(poison_from), prepare, inputs or {}, align
        self.ws = None                                        # the workspace of the call in progress


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)


def run(case, ws, device):
    """One call of `case` on the workspace `ws` as it is (no fill here).  Asserts the bounds; returns {output name: uint8 copy}."""
    nbytes = int(case.size_query())
    assert nbytes >= 0, f"{case.name}: size query failed ({nbytes})"
    assert ws.nbytes >= nbytes, f"{case.name}: workspace of {ws.nbytes} bytes for a query of {nbytes}"
    outs = case.make_outs()
    before = {k: g.bytes() for k, g in case.inputs.items()}
    if case.prepare is not None:
        case.prepare(ws)
    case.ws = ws                                              # (for stand-in entries in the harness's own self-tests)
    case.call(ws.ptr, nbytes, outs)
    _sync(device)
    assert ws.intact(), f"{case.name}: a write outside the {ws.nbytes} workspace bytes (query: {nbytes})"
    for k, g in outs.items():
        assert g.intact(), f"{case.name}: a write outside output '{k}' ({g.nbytes} bytes)"
    for k, g in case.inputs.items():
        assert g.intact(), f"{case.name}: a write next to input '{k}'"
        assert torch.equal(g.bytes(), before[k]), f"{case.name}: input '{k}' was written"
    return {k: g.bytes() for k, g in outs.items()}


def fresh(case, fill, device):
    """A workspace of exactly the queried size, poisoned with `fill` behind the caller-owned region."""
    ws = Guarded(case.size_query(), 0x00, align=case.align, device=device)
    ws.fill = int(fill)
    ws.refill(start=min(case.poison_from, ws.nbytes))
    return ws


def same_bytes(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), f"{what}: output '{k}' differs ({int((a[k] != b[k]).sum())} of {a[k].numel()} bytes)"


def as_bytes(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def check_content(case, device):
    """Property (1) with (3): the outputs on a 0x00-filled and on a 0xFF-filled workspace of exactly the queried size are the same bytes,
    equal the wrapper's, and no guard is touched.  Returns ({name: bytes}, the last workspace)."""
    results, ws = [], None
    for fill in FILLS:
        ws = fresh(case, fill, device)
        assert ws.nbytes == case.size_query()                 # the interior is the queried size, not rounded up
        results.append(run(case, ws, device))
    same_bytes(results[0], results[1], f"{case.name}: outputs depend on the workspace's content (0x00 against 0xFF)")
    if case.wrapper is not None:
        for k, t in case.wrapper().items():
            _sync(device)
            assert torch.equal(results[0][k], as_bytes(t).to(results[0][k].device)), f"{case.name}: output '{k}' differs from the wrapper's"
    return results[0], ws


def check_stale(large, small, expected, device):
    """Property (2): `large`, then `small` on the same workspace with no refill in between gives `small`'s outputs of check_content."""
    ws = fresh(large, 0x00, device)
    run(large, ws, device)
    got = run(small, ws, device)
    same_bytes(expected, got, f"{small.name} after {large.name} on one workspace")
