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

**Attention-probability mask** (``attention`` / ``attention_qkv`` with
``p > 0``).  A word per element would cost the fused attention kernels four
Philox blocks per lane and 64x64 tile pair, so this mask spends one *byte* per
element.  Element ``(bh, q, k)`` of the ``[B, S, S]`` probabilities, with
``rho = q & 31``, ``ks = (rho >> 2) & 1`` and ``j = (rho & 3) + 4 * (rho >> 3)``,
draws byte ``j & 3`` (little-endian) of output word ``j >> 2`` of the block
whose counter is::

    (((bh * ceil(S / 32) + (q >> 5)) * 2 + ks) * S + k,
     call_id & 0xFFFFFFFF, call_id >> 32, step)

under the same key.  It is kept iff ``byte >= thr8 = floor(p * 256)`` and
scaled by ``float32(256 / (256 - thr8))``, the reciprocal of the *effective*
keep rate, so the expectation is exact; ``0 < p < 1/256`` would drop nothing
and is an error.  ``(ks, j)`` is the (lane half, register) that holds row
``rho`` of a 32x32 ``mfma_f32_32x32x16`` accumulator, so one lane of a score
quadrant owns exactly one block; the map depends on ``(bh, q, k)`` alone, and
the fused forward, the fused backward, the composed GPU route
(``ops/csrc/philox.h``) and :func:`attn_keep_mask` all use it.

**Mixup / cutmix parameters** (``BatchMix``, ``ops/csrc/mix.hip``).  One draw
per micro-batch takes one ``call_id`` and uses 65 blocks with counters
``(c0, call_id & 0xFFFFFFFF, call_id >> 32, step)`` under the same key:

* ``c0 = 64``, the choice block: apply iff ``w0 < floor(prob * 2^32)``; cutmix
  rather than mixup iff ``w1 < floor(switch_prob * 2^32)`` (with only one
  alpha nonzero that mode is always chosen); box centre ``cy = w2 mod H``,
  ``cx = w3 mod W``.
* ``c0 = t`` for ``t = 0..63``, try ``t`` of Jöhnk's sampler for
  ``Beta(alpha, alpha)``, ``0 < alpha <= 1``: ``U = (w0 + 0.5) * 2^-32``,
  ``V = (w1 + 0.5) * 2^-32``, ``X = U^(1/alpha)``, ``Y = V^(1/alpha)``; the try
  accepts iff ``X + Y <= 1``.  The lowest accepting try wins and ``lambda =
  X / (X + Y)`` (on the GPU the 64 tries are the 64 lanes of one wave); if
  none accepts, ``lambda = 0.5`` (probability at most 2^-64).

Cutmix cuts timm's box: ``r = sqrt(1 - lambda)``, ``ch = int(H r)``, ``cw =
int(W r)``, ``y0, y1 = clamp(cy -+ ch // 2, 0, H)`` and likewise in x, and the
label weight becomes ``(H W - box area) / (H W)`` rounded once to float32.
The forward and the backward of the loss read that weight from the record the
draw wrote; the only thing that writes the record is the next step's draw,
which runs before that step's forward, so both always see the same values.
:func:`mix_draw` is the float64 mirror of the kernel: the CPU path and the
oracle of the GPU draw.
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


# ------------------------------------------- attention-probability mask ----


def attn_keep_threshold(p: float) -> int:
    """thr8 = floor(p * 256); a rate in (0, 1/256) would drop nothing."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"attention dropout rate must be in [0, 1), got {p}")
    thr8 = int(math.floor(p * 256.0))
    if p > 0 and thr8 == 0:
        raise ValueError(
            f"attention dropout rate {p} is below 1/256: the byte mask would "
            "drop nothing")
    return thr8


def attn_keep_scale(p: float) -> float:
    """float32(256 / (256 - thr8)): one over the effective keep rate."""
    return float(np.float32(256.0 / (256.0 - attn_keep_threshold(p))))


def attn_draw_index(B: int, S: int) -> tuple[np.ndarray, np.ndarray]:
    """(counter word 0, byte index 0..15) of every element, each [B, S, S]."""
    nq32 = (S + 31) // 32
    if B * nq32 * 2 * S > _MASK32:
        raise ValueError(
            f"attention dropout: the block counter of {B} x {S} x {S} "
            "probabilities does not fit 32 bits")
    bh = np.arange(B, dtype=np.uint64)[:, None, None]
    q = np.arange(S, dtype=np.uint64)[None, :, None]
    k = np.arange(S, dtype=np.uint64)[None, None, :]
    rho = q & np.uint64(31)
    ks = (rho >> np.uint64(2)) & np.uint64(1)
    j = (rho & np.uint64(3)) + np.uint64(4) * (rho >> np.uint64(3))
    c0 = ((bh * np.uint64(nq32) + (q >> np.uint64(5))) * np.uint64(2)
          + ks) * np.uint64(S) + k
    return c0, np.broadcast_to(j, c0.shape)


def attn_keep_mask(B: int, S: int, p: float, call_id: int,
                   step: int) -> torch.Tensor:
    """Bool tensor [B, S, S]: the attention-probability keep mask of a call
    under the current key (module docstring)."""
    thr8 = attn_keep_threshold(p)
    c0, j = attn_draw_index(B, S)
    k0, k1 = key()
    # the counters are 0 .. B * ceil(S/32) * 2 * S - 1: draw each block once
    blocks = np.arange(B * ((S + 31) // 32) * 2 * S, dtype=np.uint64)
    w = np.stack(philox4x32_10(blocks, call_id & _MASK32,
                               (call_id >> 32) & _MASK32, step & _MASK32,
                               k0, k1), axis=1)
    word = w[c0.astype(np.intp), (j >> np.uint64(2)).astype(np.intp)]
    byte = (word >> (np.uint64(8) * (j & np.uint64(3)))) & np.uint64(0xFF)
    return torch.from_numpy(byte >= np.uint64(thr8))


# ------------------------------------------------ mixup / cutmix draw -------

MIX_NONE, MIX_MIXUP, MIX_CUTMIX = 0, 1, 2


def check_mix_args(alpha_mix, alpha_cut, prob=1.0, switch_prob=0.5) -> None:
    """The argument rules of the draw (module docstring); raises ValueError."""
    for name, alpha in (("mixup", alpha_mix), ("cutmix", alpha_cut)):
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(
                f"{name} alpha must be in [0, 1] (0 = off), got {alpha}: "
                "lambda ~ Beta(alpha, alpha) is drawn by Joehnk's method with "
                "one try per lane of a wave, and its acceptance rate drops "
                "below 1/2 for alpha > 1")
    if alpha_mix == 0 and alpha_cut == 0:
        raise ValueError("mixup and cutmix alpha are both 0: nothing to draw")
    for name, p in (("prob", prob), ("switch_prob", switch_prob)):
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"mix {name} must be in [0, 1], got {p}")


def mix_draw(H, W, alpha_mix, alpha_cut, prob, switch_prob, call_id, step):
    """The mix params record of one draw under the current key, in float64:
    the mirror of ``mix::draw_kernel`` (same counters, same word use).

    Returns a dict: ``lam`` (label weight), ``a`` (blend weight), ``y0 y1 x0
    x1`` (box), ``mode`` (0 not applied, 1 mixup, 2 cutmix), ``raw`` (lambda as
    drawn, before the box correction), plus ``cy cx`` (box centre) and
    ``knife``: True where a float32 evaluation may legitimately decide
    otherwise, i.e. a try up to the winner has ``|X + Y - 1| < 1e-4`` or,
    under cutmix, ``H sqrt(1 - lambda)`` or ``W sqrt(1 - lambda)`` lies within
    1e-3 of an integer >= 1.  ``step`` may be an array; every value is then an
    array over the steps."""
    check_mix_args(alpha_mix, alpha_cut, prob, switch_prob)
    scalar = np.ndim(step) == 0
    steps = np.atleast_1d(np.asarray(step)).astype(np.uint64) & np.uint64(_MASK32)
    n = steps.shape[0]
    k0, k1 = key()
    c0 = np.broadcast_to(np.arange(65, dtype=np.uint64)[None, :], (n, 65))
    w = philox4x32_10(c0, call_id & _MASK32, (call_id >> 32) & _MASK32,
                      steps[:, None], k0, k1)
    w = [np.broadcast_to(a, (n, 65)) for a in w]
    choice = [a[:, 64] for a in w]
    applied = choice[0] < np.uint64(keep_threshold(prob))
    if alpha_mix == 0:
        cut = np.ones(n, dtype=bool)
    elif alpha_cut == 0:
        cut = np.zeros(n, dtype=bool)
    else:
        cut = choice[1] < np.uint64(keep_threshold(switch_prob))
    inv_alpha = 1.0 / np.where(cut, alpha_cut or 1.0, alpha_mix or 1.0)
    X = ((w[0][:, :64].astype(np.float64) + 0.5) * 2.0 ** -32) ** inv_alpha[:, None]
    Y = ((w[1][:, :64].astype(np.float64) + 0.5) * 2.0 ** -32) ** inv_alpha[:, None]
    s = X + Y
    acc = s <= 1.0
    hit = acc.any(axis=1)
    win = np.where(hit, acc.argmax(axis=1), 63)
    rows = np.arange(n)
    xs, ys = X[rows, win], Y[rows, win]
    raw = np.where(hit, xs / (xs + ys), 0.5)
    oml = np.where(hit, ys / (xs + ys), 0.5)  # 1 - lambda, no cancellation
    tried = np.arange(64)[None, :] <= win[:, None]
    knife = ((np.abs(s - 1.0) < 1e-4) & tried).any(axis=1)

    cy = (choice[2] % np.uint64(H)).astype(np.int64)
    cx = (choice[3] % np.uint64(W)).astype(np.int64)
    hr, wr = H * np.sqrt(oml), W * np.sqrt(oml)
    bh, bw = np.floor(hr).astype(np.int64), np.floor(wr).astype(np.int64)
    y0, y1 = np.clip(cy - bh // 2, 0, H), np.clip(cy + bh // 2, 0, H)
    x0, x1 = np.clip(cx - bw // 2, 0, W), np.clip(cx + bw // 2, 0, W)

    def near_int(v):
        return (np.abs(v - np.rint(v)) < 1e-3) & (np.rint(v) >= 1)

    is_cut, is_mix = applied & cut, applied & ~cut
    knife = applied & (knife | (cut & (near_int(hr) | near_int(wr))))
    area = (y1 - y0) * (x1 - x0)
    lam_cut = ((H * W - area).astype(np.float32)
               / np.float32(H * W)).astype(np.float64)
    zero = np.zeros(n, dtype=np.int64)
    out = {
        "lam": np.where(is_cut, lam_cut, np.where(is_mix, raw, 1.0)),
        "a": np.where(is_mix, raw, 1.0),
        "y0": np.where(is_cut, y0, zero), "y1": np.where(is_cut, y1, zero),
        "x0": np.where(is_cut, x0, zero), "x1": np.where(is_cut, x1, zero),
        "mode": is_mix * MIX_MIXUP + is_cut * MIX_CUTMIX,
        "raw": np.where(applied, raw, 1.0),
        "cy": cy, "cx": cx, "knife": knife,
    }
    if scalar:
        out = {k: v[0].item() for k, v in out.items()}
    return out


def mix_record(lam=1.0, a=1.0, box=(0, 0, 0, 0), mode=MIX_NONE, raw=None):
    """The 8-slot float32 record (CPU) the mix and loss kernels read: lam, a,
    then y0 y1 x0 x1 and mode as int32 bit patterns, then raw."""
    rec = torch.zeros(8, dtype=torch.float32)
    rec[0], rec[1] = float(lam), float(a)
    rec[7] = float(lam if raw is None else raw)
    rec.view(torch.int32)[2:7] = torch.tensor([*box, mode], dtype=torch.int32)
    return rec
