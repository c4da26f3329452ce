"""BN-backward sums emitted from the glds conv dgrad store phase.

``conv2d_dgrad_bnstats`` is ``conv2d_dgrad(out_mask=)`` that, on the glds
kernel, also leaves the per-channel sums  sum(dz)  and  sum(dz * xhat)  of the
masked result in a workspace; ``bn_bwd_ws`` finishes the BN backward from that
workspace (finalize + two-tensor dx pass).  Checked here:

1. ``dx`` is bit-identical to ``conv2d_dgrad(out_mask=)`` on every shape, the
   one the glds kernel declines included (which returns no workspace).
2. ``dgamma`` / ``dbeta`` (fp32) against a float64 reference computed from
   that same ``dx``: the dot-product bound of ``_errbound`` with eps_out = 0,
   depth M (+3 for dgamma: the three fp32 roundings inside one term
   ``g * (t - mean) * rstd``), mag = sum|dx| resp. sum|dx|*|xhat|.
3. ``dt`` per element against the float64 BN backward: one bf16 rounding
   (2^-8 |ref|) + the bound of check 2 propagated through
   ``gamma*rstd*(g - (dbeta + xhat*dgamma)/M)`` + 8 fp32 ulps of the element's
   magnitude term for the fp32 arithmetic of the dx pass.  Cross-check: where
   it differs from today's ``bn_bwd(dz_unmasked, y_relu=z)`` — which sums in
   another order — it differs by one bf16 ulp on top of twice the fp32 parts
   of that tolerance (both results carry them); the count is printed.
4. Blocks, ``PDT_DGRAD_BNSTATS`` on vs off on the same seeded inputs, under
   the bounds of test_gpu_dgrad_epilogue.py's block checks.

Workspace rows: the kernel wraps at 1024 rows (``kBnStatsRows``); the wrap
shape below runs 2048 workgroups.  References are float64 on the device (the
sums of the wrap shape would take seconds on the host).
"""

import functools
import os

import pytest
import torch

from _errbound import U32, assert_gemm_close, poison

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from pytorch_ddp_template_amd.ops.native import native

    EXT = native()
DEV = "cuda:0"
GATE = "PDT_DGRAD_BNSTATS"
WS_ROWS = 1024  # kBnStatsRows in conv_glds.hip
ULP = 2.0 ** -8

# n, h, dx-channels, dy-channels, r, stride, pad
GLDS_SHAPES = [
    (8, 8, 64, 64, 3, 1, 1),      # 64-wide tile, two M-tiles
    (8, 8, 192, 64, 3, 1, 1),     # three column tiles
    (8, 8, 128, 64, 3, 1, 1),     # 128-wide tile
    (8, 8, 512, 64, 3, 1, 1),     # 256-wide tile, two column tiles
    (8, 8, 64, 128, 3, 2, 1),     # stride-2 stuffed gather
    (8, 8, 256, 64, 1, 1, 0),     # 1x1, a single K-tile
    (64, 14, 64, 64, 3, 1, 1),    # non-pow2 spatial
    (512, 32, 64, 64, 3, 1, 1),   # 2048 workgroups on 1024 rows: row wrap
]
FALLBACK_SHAPE = (2, 8, 32, 32, 3, 1, 1)  # the glds kernel declines
_ids = lambda s: "-".join(map(str, s))  # noqa: E731


def _t(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


@functools.lru_cache(maxsize=None)
def _inputs(n, h, cin, kout, r, stride, pad):
    ho = (h + 2 * pad - r) // stride + 1
    dy = _t(n, ho, ho, kout, seed=28).to(torch.bfloat16).to(DEV)
    w = (_t(kout, r, r, cin, seed=29) * 0.1).to(torch.bfloat16).to(DEV)
    # BN input with per-channel offset and scale
    t = (_t(n, h, h, cin, seed=30) * (0.5 + torch.rand(cin))
         + torch.linspace(-1, 1, cin)).to(torch.bfloat16).to(DEV)
    # a ReLU output: about half exact zeros, plus a few planted -0.0
    m = torch.relu(_t(n, h, h, cin, seed=31)).to(torch.bfloat16)
    m.view(-1)[::97] = -0.0
    assert (m.view(torch.int16) == -32768).sum() > 0
    m = m.to(DEV)
    t2 = t.reshape(-1, cin).float()
    mean = t2.mean(0)
    rstd = (t2.var(0, unbiased=False) + 1e-5).rsqrt()
    # fp32 (grads then come back in fp32) with bf16-exact values, so that
    # bn_bwd, which takes gamma in the activation dtype, sees the same numbers
    gamma = (1.0 + 0.25 * _t(cin, seed=32)).to(torch.bfloat16).float().to(DEV)
    return dy, w, t, m, mean.contiguous(), rstd.contiguous(), gamma


@functools.lru_cache(maxsize=None)
def _run(shape):
    """One fused call per shape, shared by the checks (nothing is modified)."""
    n, h, cin, kout, r, stride, pad = shape
    dy, w, t, m, mean, rstd, gamma = _inputs(*shape)
    want = EXT.conv2d_dgrad(dy, w, stride, pad, h, h, out_mask=m)
    poison(DEV, 2 * n * h * h * cin + 8 * WS_ROWS * cin)
    dx, ws = EXT.conv2d_dgrad_bnstats(dy, w, stride, pad, h, h, m, t, mean,
                                      rstd)
    return want, dx, ws


def _assert_identical(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape
    gi, wi = got.view(torch.int16), want.view(torch.int16)
    if not torch.equal(gi, wi):
        diff = (got.float() - want.float()).abs()
        raise AssertionError(
            f"{what}: {int((gi != wi).sum())}/{got.numel()} elements differ "
            f"bitwise, max abs diff {diff.max().item()}")


@pytest.mark.parametrize("shape", GLDS_SHAPES + [FALLBACK_SHAPE], ids=_ids)
def test_dx_bit_identical_to_masked_dgrad(shape):
    want, dx, ws = _run(shape)
    _assert_identical(dx, want, "dx")
    m = _inputs(*shape)[3]
    assert (dx[~(m.float() > 0)] == 0).all()
    cin = shape[2]
    if shape == FALLBACK_SHAPE:
        assert ws is None
    else:
        assert ws is not None and ws.dtype == torch.float32
        assert ws.shape[1] == cin and ws.shape[0] % 2 == 0
        assert ws.shape[0] // 2 <= WS_ROWS
        assert torch.isfinite(ws).all()
    if shape == GLDS_SHAPES[-1]:
        nwg = shape[0] * shape[1] * shape[1] // 256 * (cin // 64)
        assert nwg >= 2 * (ws.shape[0] // 2) == 2 * WS_ROWS


def _refs(shape):
    """float64 sums and BN-backward dx from the op's own (bit-exact) dx."""
    cin = shape[2]
    _, _, t, _, mean, rstd, gamma = _inputs(*shape)
    _, dx, _ = _run(shape)
    g = dx.reshape(-1, cin).double()
    xh = (t.reshape(-1, cin).double() - mean.double()) * rstd.double()
    M = g.shape[0]
    dgam, dgam_mag = (g * xh).sum(0), (g.abs() * xh.abs()).sum(0)
    dbet, dbet_mag = g.sum(0), g.abs().sum(0)
    # bound of check 2 (gemm_bound with eps_out = 0)
    b_dgam = 1.01 * (M + 3 + 2) * U32 * dgam_mag + 1e-30
    b_dbet = 1.01 * (M + 2) * U32 * dbet_mag + 1e-30
    k = (gamma.double() * rstd.double()).abs()
    dt = gamma.double() * rstd.double() * (g - (dbet + xh * dgam) / M)
    dt_mag = k * (g.abs() + (dbet.abs() + xh.abs() * dgam.abs()) / M)
    prop = k / M * (b_dbet + xh.abs() * b_dgam)
    return dict(M=M, dgam=dgam, dgam_mag=dgam_mag, dbet=dbet,
                dbet_mag=dbet_mag, dt=dt, fp32=prop + 8 * U32 * dt_mag)


@pytest.mark.parametrize("shape", GLDS_SHAPES, ids=_ids)
def test_bn_bwd_ws_sums_and_dx(shape):
    cin = shape[2]
    _, _, t, m, mean, rstd, gamma = _inputs(*shape)
    _, dx, ws = _run(shape)
    assert ws is not None
    poison(DEV, 2 * dx.numel())
    dt, dgamma, dbeta = EXT.bn_bwd_ws(dx.reshape(-1, cin), t.reshape(-1, cin),
                                      gamma, mean, rstd, ws)
    assert dgamma.dtype == torch.float32 and dbeta.dtype == torch.float32
    assert dt.dtype == torch.bfloat16
    r = _refs(shape)
    M = r["M"]
    # check 2
    assert_gemm_close(dgamma, r["dgam"].cpu(), r["dgam_mag"].cpu(), M + 3,
                      f"dgamma{shape}", torch.float32)
    assert_gemm_close(dbeta, r["dbet"].cpu(), r["dbet_mag"].cpu(), M,
                      f"dbeta{shape}", torch.float32)
    # check 3
    assert torch.isfinite(dt).all()
    err = (dt.double() - r["dt"]).abs()
    tol = ULP * r["dt"].abs() + r["fp32"]
    used = (err / tol.clamp(min=1e-300)).max().item()
    print(f"BNSTATS dt{shape} used={used:.4f}")
    bad = ~(err <= tol)
    assert not bad.any(), (
        f"dt: {int(bad.sum())}/{bad.numel()} elements outside the tolerance "
        f"(worst uses {used:.3g}x)")
    # cross-check against today's sequence on the unmasked dgrad
    n, h, _, _, _, stride, pad = shape
    dy, w = _inputs(*shape)[:2]
    dz = EXT.conv2d_dgrad(dy, w, stride, pad, h, h)
    old, _, _ = EXT.bn_bwd(dz.reshape(-1, cin), t.reshape(-1, cin),
                           gamma.to(torch.bfloat16), mean, rstd,
                           m.reshape(-1, cin))
    a, b = dt.double(), old.double()
    ndiff = int((dt.view(torch.int16) != old.view(torch.int16)).sum())
    print(f"BNSTATS dt{shape} differs from bn_bwd(y_relu=) in "
          f"{ndiff}/{dt.numel()} elements")
    one_ulp = 2 * ULP * torch.maximum(a.abs(), b.abs())  # bf16 spacing
    assert ((a - b).abs() <= one_ulp + 2 * r["fp32"]).all()


# ------------------------------------------------------- block level -----


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


class _count_ws_calls:
    """Counts bn_bwd_ws calls, so that a block check cannot pass by never
    reaching the new path."""

    def __enter__(self):
        self.n = 0
        self.orig = EXT.bn_bwd_ws

        def counted(*a, **k):
            self.n += 1
            return self.orig(*a, **k)

        EXT.bn_bwd_ws = counted
        return self

    def __exit__(self, *exc):
        EXT.bn_bwd_ws = self.orig


def _fwd_bwd(blk, x0):
    for p in blk.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    out = blk(x)
    out.float().square().mean().backward()
    res = {"out": out.detach().clone(), "x.grad": x.grad.clone()}
    for name, p in blk.named_parameters():
        res[name] = p.grad.clone()
    return res


BLOCK_ULPS = 16  # 2^-4 * max|ref|: test_gpu_dgrad_epilogue.py, block pair


def _assert_close(got, ref):
    assert got.keys() == ref.keys()
    for k in ref:
        tol = 3e-2 if k in ("out", "x.grad") else 5e-2
        g, r = got[k].float(), ref[k].float()
        assert torch.isfinite(g).all(), f"{k}: non-finite"
        err = (g - r).abs().max().item()
        mx = r.abs().max().item()
        print(f"BNSTATS {k}: max|diff|={err:.3e} max|ref|={mx:.3e}")
        assert torch.allclose(g, r, atol=tol, rtol=tol), (
            f"{k}: max abs diff {err} (tol {tol})")
        assert err <= BLOCK_ULPS * ULP * mx, (
            f"{k}: max abs diff {err} is {err / (ULP * mx):.1f} bf16 ulps of "
            f"max|ref|={mx} (bound {BLOCK_ULPS})")


# kind, constructor args, input shape, bn_bwd_ws calls expected with the gate
BLOCKS = [
    ("basic", (64, 64, 1), (4, 8, 8, 64), 1),
    ("basic", (64, 128, 2), (16, 8, 8, 64), 1),
    ("bottleneck", (256, 64, 1), (4, 8, 8, 256), 2),
    ("basic", (32, 32, 1), (4, 8, 8, 32), 0),  # the glds kernel declines
]


@pytest.mark.parametrize("kind,args,xshape,ncalls", BLOCKS,
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else
                         str(v))
def test_block_matches_gate_off(kind, args, xshape, ncalls):
    from pytorch_ddp_template_amd.models.resnet import BasicBlock, Bottleneck

    torch.manual_seed(0)
    cls = BasicBlock if kind == "basic" else Bottleneck
    blk = cls(*args).to(torch.bfloat16).to(DEV)
    blk.train()
    x0 = torch.relu(torch.randn(*xshape)).to(torch.bfloat16).to(DEV)
    with _gate("0"), _count_ws_calls() as c0:
        ref = _fwd_bwd(blk, x0)
    assert c0.n == 0
    with _gate("1"), _count_ws_calls() as c1:
        poison(DEV, x0.numel() * 64)
        got = _fwd_bwd(blk, x0)
    assert c1.n == ncalls
    _assert_close(got, ref)
