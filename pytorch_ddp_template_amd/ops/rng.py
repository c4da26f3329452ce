"""Counter-based RNG state for dropout / stochastic depth (Philox4x32-10).

The generator is stateless: every draw is a pure function of

* the **key** ``(key0, key1)`` set by :func:`manual_seed`
  (``key0 = seed & 0xFFFFFFFF``, ``key1 = ((seed >> 32) ^ rank) & 0xFFFFFFFF``),
* a **host call counter** — a Python int that never resets within a run; every
  train-mode mask takes the next value as its ``call_id``, which is a kernel
  argument (under stream capture it is baked into the graph, as wanted),
* a **device step scalar** — one int32 element per device, created lazily,
  read by the kernel as a u32.  :func:`tick` advances it with a torch op that
  is legal under stream capture, so a captured step draws fresh masks on
  every replay from the same baked call ids.  Eager training needs no tick (call ids are already
  unique); ``GraphStep._inner`` ticks once at its start; nothing ticks between
  a forward and its backward, which regenerates the forward's mask.

Element ``e`` of a call uses output word ``e & 3`` of the Philox block whose
counter is ``(e >> 2, call_id & 0xFFFFFFFF, call_id >> 32, step)``; for a row
mask ``e`` is the row index.  An element is kept iff ``word >= floor(p *
2^32)`` and scaled by ``float32(1 / (1 - p))``.

``(call_id, step)`` pairs never repeat: eager calls differ in ``call_id``,
replays of one site differ in ``step``, and eager calls before or after a
capture use smaller or larger ids than the captured ones.

The numpy implementation below is the CPU path of ``ops.functional.dropout*``
and produces the same bits as ``ops/csrc/dropout.hip``.
"""

from __future__ import annotations

import math

import numpy as np
import torch

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = 0xFFFFFFFF

_seed = 0
_rank = 0
_next_call = 0
_step_init = 0  # value a newly created device scalar starts from
_scalars: dict[torch.device, torch.Tensor] = {}
_last: torch.device | None = None  # device whose scalar was used last


def manual_seed(seed: int, rank: int = 0) -> None:
    """Set the key from (seed, rank); reset the call counter and the step."""
    global _seed, _rank, _next_call, _step_init
    _seed, _rank = int(seed), int(rank)
    _next_call = 0
    _step_init = 0
    for t in _scalars.values():
        t.zero_()


def key() -> tuple[int, int]:
    return _seed & _MASK32, ((_seed >> 32) ^ _rank) & _MASK32


def next_call_id() -> int:
    """Take the next value of the host call counter."""
    global _next_call
    cid = _next_call
    _next_call += 1
    return cid


def _as_i32(v: int) -> int:
    v &= _MASK32
    return v - (1 << 32) if v >= (1 << 31) else v


def _current_step() -> int:
    if _last is not None:
        return int(_scalars[_last].item()) & _MASK32
    return _step_init


def step_scalar(device) -> torch.Tensor:
    """The device's step scalar (one int32 element), created on first use
    with the current step value.  A process normally draws on one device; if
    it draws on several, each keeps its own step, :func:`tick` advances the
    one it names and :func:`get_state` reports the one used last
    (:func:`manual_seed` and :func:`set_state` write all of them)."""
    global _last
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    t = _scalars.get(device)
    if t is None:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(
                "rng.step_scalar: the step scalar of a device must exist "
                "before a stream capture begins (run one eager step, or call "
                "rng.step_scalar(device) first)"
            )
        t = torch.full((1,), _as_i32(_current_step()), dtype=torch.int32,
                       device=device)
        _scalars[device] = t
    _last = device
    return t


def tick(device=None) -> None:
    """Advance the step of ``device`` (default: the device used last, else
    the CPU) by one with an in-place add, which is legal under capture."""
    if device is None:
        device = _last if _last is not None else "cpu"
    step_scalar(device).add_(1)


def get_state() -> dict:
    """Seed, rank, next call id and step (reads the device scalar)."""
    return {"seed": _seed, "rank": _rank, "next_call": _next_call,
            "step": _current_step()}


def set_state(state: dict) -> None:
    global _seed, _rank, _next_call, _step_init
    _seed, _rank = int(state["seed"]), int(state["rank"])
    _next_call = int(state["next_call"])
    _step_init = int(state["step"]) & _MASK32
    for t in _scalars.values():
        t.fill_(_as_i32(_step_init))


# ------------------------------------------------------------- host Philox --


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over numpy arrays (or ints) of counter words; returns the
    four output words as uint64 arrays holding 32-bit values."""
    m = np.uint64(_MASK32)
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & m
                      for v in (c0, c1, c2, c3))
    k0, k1 = int(k0) & _MASK32, int(k1) & _MASK32
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(_M0) * c0
        p1 = np.uint64(_M1) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m,
                          (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m)
        k0, k1 = (k0 + _W0) & _MASK32, (k1 + _W1) & _MASK32
    return c0, c1, c2, c3


def draws(n: int, call_id: int, step: int) -> np.ndarray:
    """The words of elements 0..n-1 of a call under the current key."""
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    k0, k1 = key()
    w = philox4x32_10(blocks, call_id & _MASK32, (call_id >> 32) & _MASK32,
                      step & _MASK32, k0, k1)
    return np.stack(w, axis=1).reshape(-1)[:n]


def keep_threshold(p: float) -> int:
    return int(math.floor(float(p) * 4294967296.0))


def keep_scale(p: float) -> float:
    """float32(1 / (1 - p)), formed in double."""
    return float(np.float32(1.0 / (1.0 - float(p))))


def keep_mask(n: int, p: float, call_id: int, step: int) -> torch.Tensor:
    """Bool tensor [n]: element kept iff its word >= floor(p * 2^32)."""
    w = draws(n, call_id, step)
    return torch.from_numpy(w >= np.uint64(keep_threshold(p)))
