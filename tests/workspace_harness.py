"""Guarded, pre-filled workspaces for the entries that take caller-supplied scratch memory.

The library's contract (include/d3p_hip.h, "Workspaces"): a workspace's contents on entry are unspecified, an entry writes nothing
outside ``[workspace_dev, workspace_dev + d3p_*_workspace())``, a shorter buffer is refused before any launch, and what one run
leaves behind never changes what the next computes.  ``torch.empty`` inside one pytest process hands back recycled memory that
usually holds the previous, similar test's correct intermediates, which hides both a read before the first write and a write past
the declared size.  This module makes both visible:

  ``guarded(nbytes, fill, device)``  one uint8 allocation ``[4096 guard | nbytes interior | 4096 guard]``; the guards hold 0xA5, the
                                     interior is exactly ``nbytes`` long, starts 256-byte aligned and holds one of the FILLS
  ``patched(monkeypatch, fill)``     replaces ``DPSVI._workspace`` so that every workspace a public call takes is such an interior
                                     of exactly the requested size (or ``short_by`` bytes less: all of them, or the ``short_at``-th
                                     only), and records what it handed out

  ``guarded_empty(monkeypatch, module, rec, tag)``  the same for a module whose wrappers call ``torch.empty`` themselves

A plain module (no conftest): a test opts in by calling ``patched``; nothing changes for tests that do not.
"""
import torch

GUARD = 4096
GUARD_BYTE = 0xA5
ALIGN = 256
BIG_WORD = 0x7F7FFFFF            # the largest finite float32
FILLS = ("zero", "ones", "big", "bits", "replay", "replay_shifted")
SHIFT = 256                      # replay_shifted: the donor image rolled by one carve alignment


def _fill_bytes(nbytes, fill, donor=None, seed=0):
    """The ``nbytes`` interior bytes of ``fill`` as a CPU uint8 tensor."""
    n = int(nbytes)
    if fill == "zero":
        return torch.zeros(n, dtype=torch.uint8)
    if fill == "ones":
        return torch.full((n,), 0xFF, dtype=torch.uint8)
    if fill == "big":          # little-endian 0x7F7FFFFF words (a trailing partial word takes the word's leading bytes)
        word = torch.tensor([0xFF, 0xFF, 0x7F, 0x7F], dtype=torch.uint8)
        return word.repeat(n // 4 + 1)[:n].clone()
    if fill == "bits":
        g = torch.Generator().manual_seed(0x5EED + int(seed))
        return torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8)
    if fill in ("replay", "replay_shifted"):
        if donor is None:
            raise ValueError(f"fill {fill!r} needs the donor run's image of this workspace")
        img = donor.detach().reshape(-1).view(torch.uint8).cpu()
        if img.numel() == 0 and n:
            raise ValueError(f"fill {fill!r}: the donor image is empty")
        if img.numel() < n:      # (a donor of other size: tiled -- the scenarios here use equal shapes, so equal sizes)
            img = img.repeat(-(-n // img.numel()))
        img = img[:n].clone()
        return torch.roll(img, SHIFT) if fill == "replay_shifted" else img
    raise ValueError(f"unknown fill {fill!r} (one of {FILLS})")


class Guarded:
    """``raw`` = [.. guard | interior | guard ..]: every byte of ``raw`` outside ``interior`` holds GUARD_BYTE."""

    def __init__(self, raw, offset, nbytes, fill):
        self.raw, self.offset, self.nbytes, self.fill = raw, int(offset), int(nbytes), fill
        self.interior = raw[self.offset:self.offset + self.nbytes]
        self.requested = self.nbytes     # (patched: the size the caller asked for; nbytes is short_by less)
        self.tag = None

    def damage(self):
        """None if both guards are intact, else (side, offset, value): ``offset`` is relative to the interior's start for the guard
        in front (negative) and to the interior's end for the guard behind (0 = the first byte past the declared size)."""
        end = self.offset + self.nbytes
        for side, lo, hi, origin in (("front", 0, self.offset, self.offset), ("back", end, self.raw.numel(), end)):
            bad = (self.raw[lo:hi] != GUARD_BYTE).nonzero()
            if bad.numel():
                at = lo + int(bad[0])
                return side, at - origin, int(self.raw[at])
        return None

    def check(self, what=""):
        hit = self.damage()
        if hit is not None:
            side, off, val = hit
            where = f"{-off} bytes in front of the workspace" if side == "front" else f"{off} bytes past the workspace's end"
            raise AssertionError(f"{what or self.tag or 'workspace'} ({self.nbytes} bytes, fill {self.fill}): the {side} guard was written, "
                                 f"first at offset {off} ({where}): 0x{val:02X}")

    def image(self):
        """A clone of the interior as it is now (the donor image of a later ``replay``)."""
        return self.interior.clone()


def guarded(nbytes, fill="zero", device="cpu", donor=None, seed=0):
    nbytes = int(nbytes)
    if nbytes < 0:
        raise ValueError("guarded: a negative size")
    raw = torch.full((GUARD + nbytes + GUARD + ALIGN - 1,), GUARD_BYTE, dtype=torch.uint8, device=device)
    offset = GUARD + (-(raw.data_ptr() + GUARD)) % ALIGN
    g = Guarded(raw, offset, nbytes, fill)
    if nbytes:
        g.interior.copy_(_fill_bytes(nbytes, fill, donor, seed))
    return g


def _stream_id(device):
    dev = torch.device(device)
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else 0


class Recorder:
    """What ``patched`` handed out: ``buffers`` in hand-out order (one entry per allocation, not per call)."""

    def __init__(self, fill, short_by, donors, short_at=None):
        self.fill, self.short_by, self.donors, self.short_at = fill, int(short_by), dict(donors or {}), short_at
        self.buffers = []
        self.calls = []          # (tag, requested nbytes) of every call, lookups included
        self.workspaces = []     # the buffers that are workspaces (not guarded outputs), in hand-out order

    def take(self, nbytes, device, tag, output=False):
        """A new guarded buffer of this recorder's fill for purpose ``tag``, recorded: what the patched ``_workspace`` hands out, and
        what a test passes to an entry it calls itself.  A workspace is ``short_by`` bytes shorter than ``nbytes`` -- every one, or
        with ``short_at = k`` only the k-th workspace handed out (0-based) -- and ``replay`` fills it from the donor image of the same
        purpose AND the same ordinal among that purpose's hand-outs (``donors[(tag, i)]``): the image the same call of the donor
        run left.  ``output``: an output array of such a call, guarded like a workspace -- full size, and random bytes where the
        fill would need a donor image."""
        nbytes = int(nbytes)
        if output:
            g = guarded(nbytes, "bits" if self.fill.startswith("replay") else self.fill, device, seed=len(self.buffers))
            g.key = (tag, sum(1 for h in self.buffers if h.tag == tag))
        else:
            short = self.short_by if self.short_at in (None, len(self.workspaces)) else 0
            key = (tag, sum(1 for h in self.workspaces if h.tag == tag))
            g = guarded(max(nbytes - short, 0), self.fill, device, donor=self.donors.get(key), seed=len(self.buffers))
            g.key = key
            self.workspaces.append(g)
        g.requested, g.tag, g.seed = nbytes, tag, len(self.buffers)
        self.buffers.append(g)
        return g

    def check_all(self, what=""):
        for g in self.buffers:
            g.check(f"{what + ': ' if what else ''}workspace '{g.tag}'")

    def images(self):
        """(tag, i) -> clone of the interior of the i-th workspace handed out for purpose ``tag``: the donors of a later
        ``patched(.., 'replay', donors=...)``, whose i-th hand-out for that purpose is the same call of the same scenario."""
        return {g.key: g.image() for g in self.workspaces}

    def of(self, tensor):
        """The Guarded whose interior ``tensor`` is."""
        for g in self.buffers:
            if g.interior.data_ptr() == tensor.data_ptr() and g.nbytes == tensor.numel():
                return g
        raise KeyError("not a buffer of this recorder")


def patched(monkeypatch, fill, short_by=0, donors=None, short_at=None):
    """Replace ``DPSVI._workspace`` (through ``monkeypatch``, so the real method is back after the test) and return the Recorder.

    The real rule: one buffer per (purpose, device, stream), handed back as long as it is at least as large as the request -- so a
    caller may get MORE than it asked for.  The replacement keeps the key and the re-use (``last_run_status()`` and the host key-chain
    record read the buffer of the last run again, also through the ``nbytes = 0`` lookup), but a request for another positive size
    than the cached buffer's gets a new buffer of exactly that size: whatever an entry writes past its declared size lands in a guard.
    A buffer is filled once, at its first hand-out; a later call of the same size sees what the call before left there, as with the
    real method.  ``short_by`` / ``short_at`` and ``donors``: ``Recorder.take``."""
    from d3p_amd.svi import DPSVI
    rec = Recorder(fill, short_by, donors, short_at)
    if fill not in FILLS:
        raise ValueError(f"unknown fill {fill!r} (one of {FILLS})")

    def _workspace(self, nbytes, device, tag="ws"):
        nbytes = int(nbytes)
        rec.calls.append((tag, nbytes))
        key = (tag, str(device), _stream_id(device))
        held = getattr(self, "_guarded_ws", None)
        if held is None:
            held = self._guarded_ws = {}
        g = held.get(key)
        if g is not None and (nbytes == 0 or g.requested == nbytes):
            return g.interior
        g = rec.take(nbytes, device, tag)
        held[key] = g
        self._ws[key] = g.interior       # (what the real method keeps: code that looks there finds the same buffer)
        return g.interior

    monkeypatch.setattr(DPSVI, "_workspace", _workspace)
    return rec


class _TorchWithGuardedEmpty:
    """``torch`` as a module under test sees it, except that ``torch.empty`` hands out the recorder's guarded memory: a 1-D uint8
    request is the call's workspace (purpose ``tag``), everything else an output array."""

    def __init__(self, rec, tag):
        self._rec, self._tag = rec, tag

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None, **kw):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        size = tuple(int(n) for n in size)
        dtype = dtype or torch.get_default_dtype()
        count = 1
        for n in size:
            count *= n
        workspace = dtype == torch.uint8 and len(size) == 1
        tag = self._tag if workspace else f"out.{self._tag}.{len(self._rec.buffers)}"
        g = self._rec.take(count * torch.empty(0, dtype=dtype).element_size(), device or "cpu", tag, output=not workspace)
        return g.interior if workspace else g.interior.view(dtype).reshape(size)      # (a short workspace is short)


def guarded_empty(monkeypatch, module, rec, tag):
    """Make ``module`` (one whose wrappers allocate their workspace and outputs with ``torch.empty`` themselves) allocate from ``rec``
    instead, until ``monkeypatch`` is undone: its PUBLIC functions then run on a guarded, pre-filled workspace of purpose ``tag`` --
    short where the recorder says so -- and write into guarded outputs."""
    monkeypatch.setattr(module, "torch", _TorchWithGuardedEmpty(rec, tag))


def raw_bytes(t):
    """A tensor's bytes as a CPU uint8 tensor: the comparisons are on bits, so NaN equals NaN and -0.0 differs from 0.0."""
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()
