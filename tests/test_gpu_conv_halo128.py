"""Halo-resident A operand of the 128-wide glds conv tile (``PDT_CONV_HALO128``).

For 3x3 stride-1 pad-1 convs with 128 input channels on 16-wide images whose
256-row M-tile is one 16 x 16 slab of an image, ``cg::conv_fwd_glds_kernel``
stages the 18 x 18 input patch once per block (two 64-channel planes) instead
of the whole A tile once per tap and channel slice.  The K order (tap-major,
then the two 64-channel slices) and the MFMA sequence per output element are
those of the per-tap route, so:

1. ``conv_halo128_eligible`` says which shapes take the route (asserted on
   taken and declined shapes alike, so a shape cannot be silently declined and
   the rest pass vacuously).
2. ``y`` (``conv2d_fwd_stats``) and ``dx`` (``conv2d_dgrad`` with no epilogue,
   ``addend``, ``out_mask``, both, and ``conv2d_dgrad_bnstats``) are
   BIT-IDENTICAL with the gate on and off, on the same seeded inputs, outputs
   allocated after ``poison``.
3. Independently ``y`` and the plain ``dx`` are inside
   ``_errbound.assert_gemm_close`` of the float64 reference at depth 9 x 128
   (the epilogue cases inherit it through 2).
4. The forward stats and the BN-backward sums (fp32 atomics, not bit-stable)
   of each route against float64 sums of that route's own ``y`` / ``dx``, with
   the bounds of checks 4 and 5 of test_gpu_conv_halo64.py: depth M with
   eps_out = 0 (+3 for the three fp32 roundings inside one
   ``g * (t - mean) * rstd`` term), plus, for the forward stats, the
   reference's own bf16 rounding (the kernel sums its fp32 accumulators, the
   reference sees only the rounded ``y``).
5. One fused BasicBlock(128, 128) forward+backward at (2, 16, 16, 128), gate
   on vs off: output bit-identical; every conv call of the block replayed with
   the gate off on the tensors it received, bit-identical; input, weight and
   BN grads under the block bounds of test_gpu_dgrad_epilogue.py (3e-2 / 5e-2
   allclose, 16 bf16 ulps of max|ref|).  The input grad is not asserted
   bit-identical end to end: the block's backward is not reproducible run to
   run on either route (BN-backward sums are combined with float atomics).
"""

import functools
import os

import pytest
import torch

from _errbound import (EPS_OUT, U32, assert_gemm_close, conv_dgrad_ref,
                       conv_fwd_ref, poison)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from pytorch_ddp_template_amd.ops.native import native

    EXT = native()
DEV = "cuda:0"
GATE = "PDT_CONV_HALO128"
ULP = 2.0 ** -8

# n, h, w, c, kout — all 3x3, stride 1, pad 1
TAKEN = [
    (1, 16, 16, 128, 128),  # one block; both halo edge rows are image borders
    (3, 16, 16, 128, 128),  # odd block count (XCD remap); image boundaries
    (2, 32, 16, 128, 128),  # two tiles per image: interior halo rows
    (2, 16, 16, 128, 384),  # three column tiles, n0 != 0
]
DECLINED = [
    (2, 16, 16, 128, 256),  # 256-wide tile
    (2, 16, 16, 128, 64),   # 64-wide tile
    (2, 16, 32, 128, 128),  # W = 32
    (2, 8, 16, 128, 128),   # H < 16
    (2, 16, 16, 256, 128),  # C = 256
    (2, 16, 16, 64, 128),   # C = 64
]
_ids = lambda s: "-".join(map(str, s))  # noqa: E731


class _gate:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get(GATE)
        os.environ[GATE] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(GATE, None)
        else:
            os.environ[GATE] = self.old


def _t(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _assert_identical(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape
    gi, wi = got.view(torch.int16), want.view(torch.int16)
    if not torch.equal(gi, wi):
        diff = (got.float() - want.float()).abs()
        raise AssertionError(
            f"{what}: {int((gi != wi).sum())}/{got.numel()} elements differ "
            f"bitwise, max abs diff {diff.max().item()}")


@pytest.mark.parametrize("shape", TAKEN + DECLINED, ids=_ids)
def test_route_query(shape):
    n, h, w, c, kout = shape
    assert EXT.conv_halo128_eligible(h, w, c, kout, 3, 3, 1, 1) == (
        shape in TAKEN)
    # not a 3x3 stride-1 pad-1 conv: always the per-tap route
    assert not EXT.conv_halo128_eligible(h, w, c, kout, 1, 1, 1, 0)
    assert not EXT.conv_halo128_eligible(h, w, c, kout, 3, 3, 2, 1)
    assert not EXT.conv_halo128_eligible(h, w, c, kout, 3, 3, 1, 0)


# ------------------------------------------------------------ forward -----


@functools.lru_cache(maxsize=None)
def _fwd(shape):
    """Inputs, both routes' (y, ws) and the float64 reference of one shape."""
    n, h, w, c, kout = shape
    x = _t(n, h, w, c, seed=51).to(torch.bfloat16).to(DEV)
    wt = (_t(kout, 3, 3, c, seed=52) * 0.1).to(torch.bfloat16).to(DEV)
    res = {}
    for gate in ("0", "1"):
        with _gate(gate):
            poison(DEV, 2 * n * h * w * kout)
            y, ws = EXT.conv2d_fwd_stats(x, wt, None, 1, 1, False)
        res[gate] = (y, ws)
    torch.cuda.synchronize()
    return x, wt, res, conv_fwd_ref(x, wt, None, 1, 1)


@pytest.mark.parametrize("shape", TAKEN, ids=_ids)
def test_fwd_bit_identical_and_close(shape):
    _, _, res, (ref, mag, depth) = _fwd(shape)
    assert depth == 9 * 128
    _assert_identical(res["1"][0], res["0"][0], f"y{shape}")
    assert_gemm_close(res["1"][0], ref, mag, depth, f"halo128 y{shape}")


@pytest.mark.parametrize("gate", ["0", "1"])
@pytest.mark.parametrize("shape", TAKEN, ids=_ids)
def test_fwd_stats_match_own_output(shape, gate):
    kout = shape[4]
    y, ws = _fwd(shape)[2][gate]
    assert ws.dtype == torch.float32 and ws.shape[1] == kout
    nb = ws.shape[0] // 2
    got_s = ws[:nb].double().sum(0).cpu()
    got_q = ws[nb:].double().sum(0).cpu()
    y2 = y.reshape(-1, kout).double().cpu()
    M = y2.shape[0]
    eps = EPS_OUT[torch.bfloat16]
    for what, got, ref, mag, e in (
            ("sum", got_s, y2.sum(0), y2.abs().sum(0), eps),
            ("sumsq", got_q, (y2 * y2).sum(0), (y2 * y2).sum(0),
             2 * eps + eps * eps)):
        # docstring, check 4: the reference's own rounding + the depth-M bound
        bound = e * mag + 1.01 * (M + 2) * U32 * mag + 1e-30
        err = (got - ref).abs()
        used = (err / bound).max().item()
        print(f"HALO128 fwd {what}{shape} gate={gate} used={used:.4f}")
        assert (err <= bound).all(), (
            f"{what}{shape} gate={gate}: worst uses {used:.3g}x of the bound")


# -------------------------------------------------------------- dgrad -----


@functools.lru_cache(maxsize=None)
def _dgrad_inputs(shape):
    # the shape's C is dy's channel count, its Kout is dx's
    n, h, w, c, kout = shape
    dy = _t(n, h, w, c, seed=53).to(torch.bfloat16).to(DEV)
    wt = (_t(c, 3, 3, kout, seed=54) * 0.1).to(torch.bfloat16).to(DEV)
    a = _t(n, h, w, kout, seed=55).to(torch.bfloat16).to(DEV)
    # a ReLU output: about half exact zeros, plus a few planted -0.0
    m = torch.relu(_t(n, h, w, kout, seed=56)).to(torch.bfloat16)
    m.view(-1)[::97] = -0.0
    assert (m.view(torch.int16) == -32768).sum() > 0
    m = m.to(DEV)
    # BN input with per-channel offset and scale, and its saved statistics
    t = (_t(n, h, w, kout, seed=57) * (0.5 + torch.rand(kout))
         + torch.linspace(-1, 1, kout)).to(torch.bfloat16).to(DEV)
    t2 = t.reshape(-1, kout).float()
    mean = t2.mean(0).contiguous()
    rstd = (t2.var(0, unbiased=False) + 1e-5).rsqrt().contiguous()
    return dy, wt, a, m, t, mean, rstd


MODES = ["none", "add", "mask", "add_mask", "bnstats"]


@functools.lru_cache(maxsize=None)
def _dgrad(shape, mode, gate):
    n, h, w, c, kout = shape
    dy, wt, a, m, t, mean, rstd = _dgrad_inputs(shape)
    with _gate(gate):
        poison(DEV, 2 * n * h * w * kout)
        if mode == "bnstats":
            dx, ws = EXT.conv2d_dgrad_bnstats(dy, wt, 1, 1, h, w, m, t, mean,
                                              rstd)
            assert ws is not None
            return dx, ws
        dx = EXT.conv2d_dgrad(
            dy, wt, 1, 1, h, w,
            addend=a if mode in ("add", "add_mask") else None,
            out_mask=m if mode in ("mask", "add_mask") else None)
    return dx, None


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", TAKEN, ids=_ids)
def test_dgrad_bit_identical(shape, mode):
    n, h, w, c, kout = shape
    # dgrad is the conv of dy (C channels) to dx (Kout channels)
    assert EXT.conv_halo128_eligible(h, w, c, kout, 3, 3, 1, 1)
    on, _ = _dgrad(shape, mode, "1")
    off, _ = _dgrad(shape, mode, "0")
    _assert_identical(on, off, f"dx{shape} {mode}")
    if mode in ("mask", "add_mask", "bnstats"):
        m = _dgrad_inputs(shape)[3]
        assert (on[~(m.float() > 0)] == 0).all()


@pytest.mark.parametrize("shape", TAKEN, ids=_ids)
def test_dgrad_close_to_float64(shape):
    n, h, w, c, kout = shape
    dy, wt = _dgrad_inputs(shape)[:2]
    ref, mag, depth = conv_dgrad_ref(dy, wt, 1, 1, h, w)
    assert depth == 9 * 128
    assert_gemm_close(_dgrad(shape, "none", "1")[0], ref, mag, depth,
                      f"halo128 dx{shape}")


@pytest.mark.parametrize("gate", ["0", "1"])
@pytest.mark.parametrize("shape", TAKEN, ids=_ids)
def test_bn_bwd_sums_match_own_output(shape, gate):
    kout = shape[4]
    _, _, _, _, t, mean, rstd = _dgrad_inputs(shape)
    dx, ws = _dgrad(shape, "bnstats", gate)
    assert ws.dtype == torch.float32 and ws.shape[1] == kout
    R = ws.shape[0] // 2
    got_dg = ws[:R].double().sum(0).cpu()
    got_db = ws[R:].double().sum(0).cpu()
    g = dx.reshape(-1, kout).double()
    xh = (t.reshape(-1, kout).double() - mean.double()) * rstd.double()
    M = g.shape[0]
    assert_gemm_close(got_dg, (g * xh).sum(0).cpu(),
                      (g.abs() * xh.abs()).sum(0).cpu(), M + 3,
                      f"halo128 dgamma-sum{shape} gate={gate}", torch.float32)
    assert_gemm_close(got_db, g.sum(0).cpu(), g.abs().sum(0).cpu(), M,
                      f"halo128 dbeta-sum{shape} gate={gate}", torch.float32)


# -------------------------------------------------------------- block -----

BLOCK_ULPS = 16  # 2^-4 * max|ref|: test_gpu_dgrad_epilogue.py, block pair
CONV_OPS = ("conv2d_fwd_stats", "conv2d_dgrad", "conv2d_dgrad_bnstats")


class _record_convs:
    """Records every conv call of the extension (arguments and first output),
    so that each can be replayed on the tensors it actually received."""

    def __enter__(self):
        self.calls, self.orig = [], {}
        for name in CONV_OPS:
            self.orig[name] = orig = getattr(EXT, name)

            def rec(*a, _name=name, _orig=orig, **k):
                out = _orig(*a, **k)
                first = out[0] if isinstance(out, (tuple, list)) else out
                self.calls.append((_name, a, k, first.clone()))
                return out

            setattr(EXT, name, rec)
        return self

    def __exit__(self, *exc):
        for name, orig in self.orig.items():
            setattr(EXT, name, orig)


def _block_fwd_bwd(blk, x0):
    for p in blk.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    out = blk(x)
    assert "FusedBasicBlockFn" in type(out.grad_fn).__name__
    out.float().square().mean().backward()
    res = {"out": out.detach().clone(), "x.grad": x.grad.clone()}
    for name, p in blk.named_parameters():
        res[name] = p.grad.clone()
    return res


def test_fused_basic_block_matches_gate_off():
    from pytorch_ddp_template_amd.models.resnet import BasicBlock

    assert EXT.conv_halo128_eligible(16, 16, 128, 128, 3, 3, 1, 1)
    torch.manual_seed(0)
    blk = BasicBlock(128, 128, 1).to(torch.bfloat16).to(DEV)
    blk.train()
    x0 = torch.relu(torch.randn(2, 16, 16, 128)).to(torch.bfloat16).to(DEV)
    with _gate("0"):
        ref = _block_fwd_bwd(blk, x0)
    with _gate("1"), _record_convs() as rec:
        poison(DEV, x0.numel() * 64)
        got = _block_fwd_bwd(blk, x0)
    assert got.keys() == ref.keys()
    # the forward has one writer per stats-workspace cell at this size
    _assert_identical(got["out"], ref["out"], "out")
    # Every conv of the block (two forwards with stats, the masked dgrad with
    # BN sums, the dgrad with the skip-grad addend), replayed with the gate off
    # on the very tensors it received: bit-identical.  The input grad itself
    # is not reproducible run to run on EITHER route — bn_bwd's stats kernel
    # combines its waves through LDS float atomics — so it is held to the
    # replay plus the same-composition bound below.
    assert [c[0] for c in rec.calls] == [
        "conv2d_fwd_stats", "conv2d_fwd_stats", "conv2d_dgrad_bnstats",
        "conv2d_dgrad"]
    with _gate("0"):
        for name, a, k, first in rec.calls:
            out = getattr(EXT, name)(*a, **k)
            again = out[0] if isinstance(out, (tuple, list)) else out
            _assert_identical(first, again, f"replayed {name}")
    for k in ref:
        tol = 3e-2 if k in ("out", "x.grad") else 5e-2
        g, r = got[k].float(), ref[k].float()
        assert torch.isfinite(g).all(), f"{k}: non-finite"
        err = (g - r).abs().max().item()
        mx = r.abs().max().item()
        print(f"HALO128 block {k}: max|diff|={err:.3e} max|ref|={mx:.3e}")
        assert torch.allclose(g, r, atol=tol, rtol=tol), (
            f"{k}: max abs diff {err} (tol {tol})")
        assert err <= BLOCK_ULPS * ULP * mx, (
            f"{k}: max abs diff {err} is {err / (ULP * mx):.1f} bf16 ulps of "
            f"max|ref|={mx} (bound {BLOCK_ULPS})")
