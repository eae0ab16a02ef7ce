"""Guarded device buffers and the checks of the extent tests (tests/test_extents_cpu.py, tests/test_gpu_extents.py).

A buffer handed to an entry of include/olsr.h sits in the middle of a larger uint8 tensor that the test owns: GUARD bytes of
FILL on either side, so that a store past either end lands in memory whose contents are known and is seen afterwards.  The
view itself is filled too: with FILL (scratch and state buffers, whose sub-arrays the library's carve log names), or with a
pattern no kernel writes (outputs declared fully written).  Nothing here knows a field, an entry or a layout: only buffers
and the log of (base, offset, bytes) records that olsr_debug_carve_log_read returns.

GUARD is 64 KiB: a block of 1024 threads stores 16 KiB in one round of 16-byte stores, so a ragged-tail overrun of a whole
block, or of a few, stays inside the guard."""
import numpy as np
import torch

GUARD = 64 * 1024
FILL = 0xA5
F32_PREFILL = 0x7FC0A5A5   # a quiet NaN with a recognisable payload
I32_PREFILL = 0x5A5A5A5A
DEV = "cuda:0"

_REG = {}   # data_ptr of a guarded view -> (whole tensor, start, nbytes)


def reset():
    """Forget (and free) every guarded buffer handed out so far."""
    _REG.clear()


def guarded(nbytes, misalign=0, device=DEV):
    """A uint8 view of exactly `nbytes` bytes, GUARD bytes of FILL before and behind it inside one tensor, itself filled with
    FILL; it starts `misalign` bytes past a 256-byte boundary."""
    nbytes = int(nbytes)
    assert 0 <= misalign < 256
    whole = torch.full((GUARD + 512 + nbytes + GUARD,), FILL, dtype=torch.uint8, device=device)
    start = GUARD + (-(whole.data_ptr() + GUARD)) % 256 + misalign
    view = whole[start:start + nbytes]
    assert nbytes == 0 or view.data_ptr() % 256 == misalign
    _REG[whole.data_ptr() + start] = (whole, start, nbytes)
    return view


def guarded_tensor(shape, dtype, misalign=0, device=DEV):
    """A guarded tensor of `shape` and `dtype`, pre-filled for written(): floats with the NaN F32_PREFILL, integers with
    I32_PREFILL (one-byte types with its byte, 0x5A)."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    size = torch.empty(0, dtype=dtype).element_size()
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    raw = guarded(n * size, misalign, device)
    t = raw.view(dtype).view(shape) if n else torch.empty(shape, dtype=dtype, device=device)
    prefill(t)
    return t


def prefill(t):
    """Fill `t` (any tensor on the device) with the pattern that written() looks for."""
    if t.numel() == 0:
        return t
    flat = t.view(-1).view(torch.uint8)
    word = F32_PREFILL if t.is_floating_point() else I32_PREFILL
    if t.element_size() % 4 == 0:
        flat.view(torch.int32).fill_(word)
    else:
        assert t.element_size() == 1
        flat.fill_(0x5A)
    return t


class Allocator:
    """Serves the library's allocation callbacks (olsr_alloc_fn) and remembers what it handed out, in call order:
    `handed` = [(user word, uint8 view)].  guard=True: views from guarded(), `misalign` bytes past a 256-byte boundary;
    guard=False: plain torch.empty."""

    def __init__(self, alloc_fn_type, guard=True, misalign=0, device=DEV):
        self.guard, self.misalign, self.device = guard, misalign, device
        self.handed = []
        self.cb = alloc_fn_type(self._serve)

    def _serve(self, user, nbytes):
        n = int(nbytes)
        t = guarded(n, self.misalign, self.device) if self.guard else torch.empty(n, dtype=torch.uint8, device=self.device)
        self.handed.append((int(user or 0), t))
        return t.data_ptr()

    def of(self, user):
        """The views handed out for this user word."""
        return [t for u, t in self.handed if u == user]

    @property
    def buffers(self):
        return [t for _, t in self.handed]


def log_on():
    from online_lang_splatting_amd._lib import carve_log
    carve_log(True)


def log_off():
    """Switch the log off and return what it held: [(base, offset, bytes)]."""
    from online_lang_splatting_amd._lib import carve_log, carve_log_read
    log = carve_log_read()
    carve_log(False)
    return log


def _first_bad(bad):
    i = int(np.flatnonzero(bad)[0])
    return i, int(bad.sum())


def check(buffers, log=(), written=()):
    """buffers: guarded views or guarded tensors (looked up by address); log: carve records; written: tensors declared fully
    written, pre-filled by guarded_tensor / prefill (a bool or uint8 output passes only if none of its bytes is 0x5A = 90: such
    outputs here are flags and masks of 0 / 1 / 255 and indices below 90; declare any other written=False).  Asserts that
      - every guard byte still holds FILL,
      - a carve record that starts inside a buffer also ends inside it,
      - in a buffer that holds carve records, every byte outside all of them still holds FILL,
      - no 32-bit word (one-byte types: no byte) of a `written` tensor still holds its pre-fill."""
    torch.cuda.synchronize()
    for b in buffers:
        if b.numel() == 0:
            continue
        whole, start, n = _REG[b.data_ptr()]
        host = whole.cpu().numpy()
        for name, part, at in (("before", host[:start], -start), ("behind", host[start + n:], n)):
            bad = part != FILL
            if bad.any():
                i, k = _first_bad(bad)
                raise AssertionError(f"{k} guard bytes {name} a buffer of {n} bytes were overwritten, the first at offset {at + i} "
                                     f"of the buffer (value {int(part[i]):#x})")
        ptr = b.data_ptr()
        covered = np.zeros(n, dtype=bool)
        carved = False
        for base, off, nbytes in log:
            lo = base + off - ptr
            if base == 0 or lo < 0 or lo >= n + 256:   # (another buffer's record; a zero-byte record at the very end is ours)
                continue
            if nbytes == 0 and lo >= n:
                continue
            assert lo + nbytes <= n, (f"a carved range [{lo}, {lo + nbytes}) leaves its buffer of {n} bytes")
            covered[lo:lo + nbytes] = True
            carved = True
        if carved:
            body = host[start:start + n]
            bad = ~covered & (body != FILL)
            if bad.any():
                i, k = _first_bad(bad)
                raise AssertionError(f"{k} bytes between the carved ranges of a buffer of {n} bytes were overwritten, the first at "
                                     f"offset {i} (value {int(body[i]):#x}, {(ptr + i) % 256} past a 256-byte boundary)")
    for t in written:
        if t.numel() == 0:
            continue
        flat = t.detach().contiguous().view(-1).view(torch.uint8)
        if t.element_size() % 4 == 0:
            word = F32_PREFILL if t.is_floating_point() else I32_PREFILL
            left = (flat.view(torch.int32) == word)
        else:
            left = (flat == 0x5A)
        k = int(left.sum())
        if k:
            i = int(left.nonzero()[0])
            raise AssertionError(f"{k} of {left.numel()} words of a {tuple(t.shape)} {t.dtype} output were never written, the first "
                                 f"at word {i}")


def same_bits(a, b):
    """Bit-for-bit equality of two tensors of one dtype and shape (NaNs compare by their bits)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return bool(torch.equal(a.detach().contiguous().view(-1).view(torch.uint8).cpu(),
                            b.detach().contiguous().view(-1).view(torch.uint8).cpu()))
