"""What every Python wrapper asks of its arguments, and how small integer tables reach the device: the one `fail`, the tensor,
offset-list, device and scalar checks, and the cached upload.  (_util.py has handles, streams and the weight watcher.)

A wrapper checks on the host first (tensors, scalars, then offset lists), then requires the device, and only then uploads."""
from __future__ import annotations

import collections
import ctypes
import os
import threading

import numpy as np
import torch


def fail(what, msg, exc=RuntimeError):
    raise exc(f"gmf_amd.{what}: {msg}")


# ---- tensors ------------------------------------------------------------------------------------------------------------------

def check_rows(what, name, x, dims, width, non_empty=False):
    """`x` is a float32 torch tensor [B,N,width] (dims 3) or packed [sum N,width] (dims 2); non_empty: no zero-sized dimension."""
    if not isinstance(x, torch.Tensor):
        fail(what, f"`{name}` must be a torch tensor")
    if x.dtype != torch.float32:
        fail(what, f"`{name}` must be float32 (got {x.dtype})")
    if x.dim() != dims or x.shape[-1] != width or (non_empty and 0 in x.shape):
        fail(what, f"`{name}` must be a {'non-empty ' if non_empty else ''}[{'B,N' if dims == 3 else 'sum N'},{width}] tensor "
                   f"(got {tuple(x.shape)})")


def require_device(x, name, what):
    """`x` lives on a HIP device.  x: a tensor, named as the argument `name`; or the device of something that is not one
    tensor, which `name` then describes ("the points")."""
    dev, subject = (x.device, f"`{name}`") if isinstance(x, torch.Tensor) else (x, name)
    if dev.type != "cuda":
        fail(what, f"{subject} must live on a HIP device (got {dev}); the HIP path is mandatory, there is no CPU fallback")


def same_device(what, **tensors):
    """The named tensors (None: absent) live on the device of the first."""
    xs = [x for x in tensors.values() if x is not None]
    if any(x.device != xs[0].device for x in xs):
        names = list(tensors)
        fail(what, f"{', '.join(names[:-1])} and {names[-1]} must live on the same device")


# ---- scalars ------------------------------------------------------------------------------------------------------------------

def positive_finite(what, name, v, allow_inf=False, rule=None, numeric=False):
    """float(v), finite (allow_inf: or +inf) and > 0.  rule: how the message states it (default "finite and > 0", or "> 0" with
    allow_inf).  numeric: something that is no number gets its own message; otherwise it fails the rule like a NaN."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        if numeric:
            fail(what, f"{name} must be a number (got {v!r})")
        f = float("nan")
    if not f > 0 or (not allow_inf and not np.isfinite(f)):
        fail(what, f"{name} must be {rule or ('> 0' if allow_inf else 'finite and > 0')} (got {v})")
    return f


def unit_interval(what, name, v):
    """float(v), finite and in [0, 1]; something that is no number fails the rule like a NaN."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        f = float("nan")
    if not 0.0 <= f <= 1.0:
        fail(what, f"{name} must be finite and in [0, 1] (got {v})")
    return f


def int_in_range(what, name, v, lo, hi, rule=None):
    """int(v) when v is integral and lo <= v <= hi.  rule: how the message states the range (default "lo..hi")."""
    try:
        n = int(v)
    except (TypeError, ValueError):
        n = None
    if n is None or n != v or not lo <= n <= hi:
        fail(what, f"{name} must be an integer {rule or f'in {lo}..{hi}'} (got {v})")
    return n


# ---- offset lists -------------------------------------------------------------------------------------------------------------

def uniform_offsets(B, N):
    """The offsets of B problems of N rows each (N = 0: B empty problems)."""
    return list(range(0, B * N + 1, N)) if N else [0] * (B + 1)


def check_offsets(what, name, offsets, n_rows, allow_empty=False):
    """The row offsets of a ragged batch, checked on the host: B + 1 integers that increase strictly (allow_empty: ascend) from 0
    to n_rows -> a list, ready for `device_offsets(..., checked=True)`.  An int32 tensor already on the device passes through
    untouched: `device_offsets` looks at its form, and the caller vouches for its values."""
    if isinstance(offsets, torch.Tensor) and offsets.is_cuda:
        return offsets
    try:
        off = [int(o) for o in (offsets.tolist() if isinstance(offsets, (torch.Tensor, np.ndarray)) else offsets)]
    except (TypeError, ValueError):
        fail(what, f"{name} must be B + 1 integers")
    if len(off) < 2 or off[0] != 0 or off[-1] != n_rows or any(b < a or (b == a and not allow_empty) for a, b in zip(off, off[1:])):
        fail(what, f"{name} must {'ascend' if allow_empty else 'increase strictly'} from 0 to the row count {n_rows} (B + 1 integers)")
    return off


def c_ints(v):
    """A C int array of a host list, for the entries that read a table on the host (never of length 0)."""
    return (ctypes.c_int * max(1, len(v)))(*v)


# (device, ints) -> [int32 device tensor, largest problem (offset lists), pinned source, event]: an LRU of the 64 most recent offset lists behind a lock (callers on
# several threads share it).  Evaluation loops that repeat a handful of shapes hit it; a loop whose offsets change on every
# call pays the upload each time - through a pinned staging buffer and an asynchronous copy, not a pageable synchronous one.
_OFFSETS_CACHE: "collections.OrderedDict" = collections.OrderedDict()
_OFFSETS_LOCK = threading.Lock()
_OFFSETS_CAP = 64


def cached_upload(values: tuple, device):
    """The cache entry [int32 device tensor, slot for the caller's derived figure, pinned source, event] of a tuple of ints (or
    of equally long tuples of ints: the tensor is then 2-d): uploaded once per (device, tuple) through a pinned buffer,
    asynchronously on the current stream, and kept."""
    key = (device, values)
    with _OFFSETS_LOCK:
        hit = _OFFSETS_CACHE.get(key)
        if hit is not None:
            _OFFSETS_CACHE.move_to_end(key)
            if hit[3] is not None:                   # the upload may still be in flight on ANOTHER stream: order this one behind it
                # (an event may not be queried while a stream captures a graph; waiting on it there is legal)
                if not torch.cuda.is_current_stream_capturing() and hit[3].query():
                    hit[3] = None
                else:
                    torch.cuda.current_stream(device).wait_event(hit[3])
            return hit
    # not cached: a pinned host copy and an asynchronous upload on the current stream (ordered before the solve that follows)
    host = torch.tensor(values, dtype=torch.int32).pin_memory()
    dev = host.to(device, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(device))
    entry = [dev, None, host, ev]                    # (the pinned source lives as long as the entry)
    with _OFFSETS_LOCK:
        _OFFSETS_CACHE[key] = entry
        while len(_OFFSETS_CACHE) > _OFFSETS_CAP:
            _OFFSETS_CACHE.popitem(last=False)
    return entry


def device_offsets(offsets, n_rows: int, device, what: str, allow_empty: bool = False, checked: bool = False):
    """The row offsets of a ragged batch as an int32 device tensor, and the largest problem.  A Python sequence is checked
    here (increasing, from 0 to n_rows; allow_empty: not decreasing) without a device round trip - unless it is `checked`, the
    list `check_offsets` returned, which is not walked again - and its device copy is kept for the next call with the same
    offsets (a list met for the first time travels through a pinned buffer, asynchronously); an int32 tensor already on the
    device is taken as it is (the caller vouches for it: only its end is not read back)."""
    if isinstance(offsets, torch.Tensor) and offsets.is_cuda:
        if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2 or not offsets.is_contiguous() \
                or offsets.device != device:
            fail(what, "device offsets must be a contiguous int32 vector of B + 1 entries on the points' device")
        if os.environ.get("GMF_DEBUG_OFFSETS"):          # (debugging aid: one device read-back of the whole vector)
            off_h = offsets.cpu().tolist()
            if off_h[0] != 0 or off_h[-1] != n_rows or any(b < a or (b == a and not allow_empty) for a, b in zip(off_h, off_h[1:])):
                fail(what, "device offsets must be increasing, start at 0 and end at N")
        return offsets, n_rows
    off = tuple(offsets) if checked else tuple(int(o) for o in offsets)
    if not checked and (len(off) < 2 or off[0] != 0 or off[-1] != n_rows
                        or any(b < a or (b == a and not allow_empty) for a, b in zip(off, off[1:]))):
        fail(what, "offsets must be increasing, start at 0 and end at N")
    entry = cached_upload(off, device)
    if entry[1] is None:
        entry[1] = max(b - a for a, b in zip(off, off[1:]))
    return entry[0], entry[1]
