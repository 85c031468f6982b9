"""Poisoned allocations: every buffer dh3d_amd uses comes from torch.empty / torch.empty_like / Tensor.new_empty
(csrc/ holds no hipMalloc), so `with poisoned(kind):` can make all of them start from chosen garbage.  A result that
differs between a plain run and the three kinds depends on memory nobody wrote.

    kind     floating   integer / bool   uint8 (workspaces, masks)
    "nan"    NaN        0                0x00
    "pos"    +1e30      1                0xFF
    "neg"    -1e30      0                0x00

Three kinds, because fmaxf / fminf on the device drop a NaN operand: "pos" and "neg" show what a max- or min-reduction
would hide.  The integer values stay small on purpose: a kernel that wrongly reads one as an index or a count stays
inside or next to its buffer -- the harness is there to show a wrong value, not to provoke a fault.

The fill runs on the current stream right after the allocation (inside a graph capture it is captured with it: every
replay poisons again).  CPU tensors and zero-element tensors are left alone (pm.ZeroArena.take builds its views with
torch.empty((0,)).set_(...)).  The module-level workspace caches of dh3d_amd.registration are emptied while the context
is active, so that cached workspaces are allocated again through the wrappers, and put back afterwards.

Used with an explicit `with` inside a test; nothing here is a fixture, and nothing changes how Python starts.
tests/test_poisoned_alloc_host.py keeps dh3d_amd from obtaining uninitialised memory by a route that is not wrapped.
"""
import contextlib

import torch

KINDS = ("nan", "pos", "neg")
# (floating, integer / bool, uint8)
FILL = {"nan": (float("nan"), 0, 0x00), "pos": (1e30, 1, 0xFF), "neg": (-1e30, 0, 0x00)}
# the three entry points: (owner, attribute)
ENTRY_POINTS = ((torch, "empty"), (torch, "empty_like"), (torch.Tensor, "new_empty"))
# module-level workspace caches: (module name, attribute) -- dicts of tensors whose content carries nothing between calls
WORKSPACE_CACHES = (("dh3d_amd.registration", "_ICP_WS"), ("dh3d_amd.registration", "_ISS_WS"))

_active = [None]


def fill_value(kind, dtype):
    """The table above; None for a dtype that is left alone (complex, quantised)."""
    f, i, u = FILL[kind]
    if dtype.is_floating_point:
        top = torch.finfo(dtype).max      # (float16 cannot hold 1e30: its largest finite value stands in)
        return f if f != f else max(-top, min(top, f))
    if dtype == torch.uint8:
        return u
    if dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.bool):
        return i
    return None


def _poison(t, kind, cpu_too):
    if not isinstance(t, torch.Tensor) or t.numel() == 0 or not (t.is_cuda or cpu_too):
        return t
    v = fill_value(kind, t.dtype)
    if v is not None:
        with torch.no_grad():
            t.fill_(v)
    return t


def _wrap(orig, kind, cpu_too):
    def wrapper(*args, **kwargs):
        return _poison(orig(*args, **kwargs), kind, cpu_too)
    wrapper.__wrapped__ = orig
    wrapper.__name__ = getattr(orig, "__name__", "empty")
    return wrapper


@contextlib.contextmanager
def poisoned(kind, _cpu_too=False):
    """kind: "nan" | "pos" | "neg"; None: nothing is replaced (the plain run, so that a test can loop over all four).
    _cpu_too: also fill CPU tensors -- for tests/test_poisoned_alloc_host.py only."""
    if kind is None:
        yield
        return
    if kind not in FILL:
        raise ValueError("poisoned: kind must be one of %s or None, got %r" % (KINDS, kind))
    if _active[0] is not None:
        raise RuntimeError("poisoned(%r) inside poisoned(%r): the context does not nest" % (kind, _active[0]))
    import importlib
    saved = [(owner, name, getattr(owner, name)) for owner, name in ENTRY_POINTS]
    caches = []
    for mod, name in WORKSPACE_CACHES:
        d = getattr(importlib.import_module(mod), name)
        caches.append((d, dict(d)))
    _active[0] = kind
    try:
        for owner, name, orig in saved:
            setattr(owner, name, _wrap(orig, kind, _cpu_too))
        for d, _ in caches:
            d.clear()
        yield
    finally:
        for owner, name, orig in saved:
            setattr(owner, name, orig)
        for d, old in caches:
            d.clear()
            d.update(old)
        _active[0] = None
