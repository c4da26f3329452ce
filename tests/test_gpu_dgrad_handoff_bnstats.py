"""BN-backward sums of the upstream block's last BN, emitted by a block's
last dgrad together with the skip-grad addend and the ReLU mask
(``conv2d_dgrad_bnstats(..., addend=)``, glds epilogue mode add+mask+bnstats),
and the hand-off of those sums between autograd nodes
(``PDT_DGRAD_HANDOFF_BNSTATS``).

1. ``dx`` is bit-identical to ``conv2d_dgrad(addend=, out_mask=)`` on the
   smallest shape that reaches each route of the glds kernel (the route queries
   confirm which one a shape takes), and on one whose workgroups wrap the
   1024 workspace rows.
2. The workspace, reduced over its rows in float64, against float64 sums of
   that same ``dx``: the bounds of test_gpu_dgrad_bnstats.py's
   ``test_bn_bwd_ws_sums_and_dx`` (dot-product bound, depth M, +3 for dgamma).
   ``bn_bwd_ws`` on it against the float64 BN backward and against ``bn_bwd``
   on the same inputs, with that test's bounds.
3. A shape the glds kernel declines returns no workspace and the masked sum
   of the separate route.
4. Wired blocks and ResNet-18, gate on against gate off: forward bit-identical;
   every hand-off dgrad, replayed on the tensors it received through
   ``conv2d_dgrad(addend=, out_mask=)``, bit-identical; all gradients inside
   the block / model bounds of test_gpu_dgrad_bnstats.py and
   test_gpu_dgrad_epilogue.py (atomics order differs, so not bit-identical).
   The stem BN's dgamma / dbeta are ``stem.0.1.weight`` / ``.bias`` of the
   ResNet-18 case and its dx reaches ``stem.0.0.weight`` through the stem
   conv's wgrad.  ResNet-18 at batch 4 also has one hand-off the glds kernel
   declines (4x4 maps: 64 rows).
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
GATE = "PDT_DGRAD_HANDOFF_BNSTATS"
WS_ROWS = 1024  # kBnStatsRows in conv_glds.hip
ULP = 2.0 ** -8

# n, h (dx), dx channels, dy channels, r, stride, pad, route
SHAPES = [
    (2, 32, 64, 64, 3, 1, 1, "halo64"),
    (2, 16, 128, 128, 3, 1, 1, "halo128"),
    (4, 8, 256, 256, 3, 1, 1, "pertap256"),
    (4, 16, 64, 128, 1, 2, 0, "stuffed64"),   # the layer-boundary hand-off
    (4, 16, 64, 128, 3, 2, 1, "parity"),
    (272, 32, 64, 64, 3, 1, 1, "halo64"),     # 1088 blocks: rows wrap
]
DECLINED = (2, 8, 48, 64, 3, 1, 1, "declined")  # 48 dx channels
_ids = lambda s: "-".join(map(str, s))  # noqa: E731


def _t(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


@functools.lru_cache(maxsize=None)
def _inputs(n, h, cin, kout, r, stride, pad, route):
    ho = (h + 2 * pad - r) // stride + 1
    dy = _t(n, ho, ho, kout, seed=48).to(torch.bfloat16).to(DEV)
    w = (_t(kout, r, r, cin, seed=49) * 0.1).to(torch.bfloat16).to(DEV)
    a = _t(n, h, h, cin, seed=50).to(torch.bfloat16).to(DEV)
    # BN input with per-channel offset and scale
    t = (_t(n, h, h, cin, seed=51) * (0.5 + torch.rand(cin))
         + torch.linspace(-1, 1, cin)).to(torch.bfloat16).to(DEV)
    # a ReLU output: about half exact zeros, plus a few planted -0.0
    m = torch.relu(_t(n, h, h, cin, seed=52)).to(torch.bfloat16)
    m.view(-1)[::97] = -0.0
    assert (m.view(torch.int16) == -32768).sum() > 0
    m = m.to(DEV)
    t2 = t.reshape(-1, cin).float()
    mean = t2.mean(0)
    rstd = (t2.var(0, unbiased=False) + 1e-5).rsqrt()
    # fp32 with bf16-exact values: bn_bwd takes gamma in the activation dtype
    gamma = (1.0 + 0.25 * _t(cin, seed=53)).to(torch.bfloat16).float().to(DEV)
    return dy, w, a, t, m, mean.contiguous(), rstd.contiguous(), gamma


@functools.lru_cache(maxsize=None)
def _run(shape):
    """One fused call per shape, shared by the checks (nothing is modified)."""
    n, h, cin, kout, r, stride, pad, _ = shape
    dy, w, a, t, m, mean, rstd, _ = _inputs(*shape)
    want = EXT.conv2d_dgrad(dy, w, stride, pad, h, h, addend=a, out_mask=m)
    poison(DEV, 2 * n * h * h * cin + 8 * WS_ROWS * cin)
    dx, ws = EXT.conv2d_dgrad_bnstats(dy, w, stride, pad, h, h, m, t, mean,
                                      rstd, addend=a)
    return want, dx, ws


def _assert_identical(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape
    gi, wi = got.view(torch.int16), want.view(torch.int16)
    if not torch.equal(gi, wi):
        diff = (got.float() - want.float()).abs()
        raise AssertionError(
            f"{what}: {int((gi != wi).sum())}/{got.numel()} elements differ "
            f"bitwise, max abs diff {diff.max().item()}")


def _routes(shape):
    """The route queries, asked as the launcher asks them: the dgrad is a
    stride-1 conv of dy (kout channels) producing dx (cin channels)."""
    n, h, cin, kout, r, stride, pad, _ = shape
    ho = (h + 2 * pad - r) // stride + 1
    dpad = r - 1 - pad
    s1 = stride == 1
    return dict(
        halo64=s1 and EXT.conv_halo64_eligible(ho, ho, kout, cin, r, r, 1,
                                               dpad),
        halo128=s1 and EXT.conv_halo128_eligible(ho, ho, kout, cin, r, r, 1,
                                                 dpad),
        parity=EXT.conv_dgrad_s2_parity_eligible(h, h, cin, kout, r, r,
                                                 stride, pad, n),
    )


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_shape_takes_the_route_named(shape):
    n, h, cin, kout, r, stride, pad, route = shape
    got = _routes(shape)
    want = dict(halo64=route == "halo64", halo128=route == "halo128",
                parity=route == "parity")
    assert got == want
    width = 256 if cin % 256 == 0 else 128 if cin % 128 == 0 else 64
    if route == "pertap256":
        assert width == 256
    if route == "stuffed64":
        assert width == 64 and stride == 2
    assert (n * h * h) % 256 == 0  # whole M-tiles: the glds kernel takes it


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_dx_bit_identical_to_add_mask_dgrad(shape):
    n, h, cin = shape[:3]
    want, dx, ws = _run(shape)
    _assert_identical(dx, want, "dx")
    m = _inputs(*shape)[4]
    assert (dx[~(m.float() > 0)] == 0).all()
    assert ws is not None and ws.dtype == torch.float32
    nwg = n * h * h // 256 * (cin // (256 if cin % 256 == 0 else
                                      128 if cin % 128 == 0 else 64))
    assert tuple(ws.shape) == (2 * min(WS_ROWS, nwg), cin)
    assert torch.isfinite(ws).all()
    if shape == SHAPES[-1]:
        assert nwg == 1088 > WS_ROWS


def _refs(shape):
    """float64 sums and BN-backward dx from the op's own (bit-exact) dx;
    the bounds are those of test_gpu_dgrad_bnstats.py::_refs."""
    cin = shape[2]
    _, _, _, t, _, mean, rstd, gamma = _inputs(*shape)
    _, dx, _ = _run(shape)
    g = dx.reshape(-1, cin).double()
    xh = (t.reshape(-1, cin).double() - mean.double()) * rstd.double()
    M = g.shape[0]
    dgam, dgam_mag = (g * xh).sum(0), (g.abs() * xh.abs()).sum(0)
    dbet, dbet_mag = g.sum(0), g.abs().sum(0)
    b_dgam = 1.01 * (M + 3 + 2) * U32 * dgam_mag + 1e-30
    b_dbet = 1.01 * (M + 2) * U32 * dbet_mag + 1e-30
    k = (gamma.double() * rstd.double()).abs()
    dt = gamma.double() * rstd.double() * (g - (dbet + xh * dgam) / M)
    dt_mag = k * (g.abs() + (dbet.abs() + xh.abs() * dgam.abs()) / M)
    prop = k / M * (b_dbet + xh.abs() * b_dgam)
    return dict(M=M, dgam=dgam, dgam_mag=dgam_mag, dbet=dbet,
                dbet_mag=dbet_mag, dt=dt, fp32=prop + 8 * U32 * dt_mag)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_sums_and_bn_bwd_ws(shape):
    cin = shape[2]
    _, _, _, t, m, mean, rstd, gamma = _inputs(*shape)
    _, dx, ws = _run(shape)
    assert ws is not None
    r = _refs(shape)
    M, R = r["M"], ws.shape[0] // 2
    # the workspace itself, rows reduced exactly
    ws64 = ws.double()
    assert_gemm_close(ws64[:R].sum(0), r["dgam"].cpu(), r["dgam_mag"].cpu(),
                      M + 3, f"ws dgamma{shape}", torch.float32)
    assert_gemm_close(ws64[R:].sum(0), r["dbet"].cpu(), r["dbet_mag"].cpu(),
                      M, f"ws dbeta{shape}", torch.float32)
    poison(DEV, 2 * dx.numel())
    dt, dgamma, dbeta = EXT.bn_bwd_ws(dx.reshape(-1, cin), t.reshape(-1, cin),
                                      gamma, mean, rstd, ws)
    assert dgamma.dtype == torch.float32 and dbeta.dtype == torch.float32
    assert dt.dtype == torch.bfloat16
    assert_gemm_close(dgamma, r["dgam"].cpu(), r["dgam_mag"].cpu(), M + 3,
                      f"dgamma{shape}", torch.float32)
    assert_gemm_close(dbeta, r["dbet"].cpu(), r["dbet_mag"].cpu(), M,
                      f"dbeta{shape}", torch.float32)
    assert torch.isfinite(dt).all()
    err = (dt.double() - r["dt"]).abs()
    tol = ULP * r["dt"].abs() + r["fp32"]
    used = (err / tol.clamp(min=1e-300)).max().item()
    print(f"HANDOFF dt{shape} used={used:.4f}")
    bad = ~(err <= tol)
    assert not bad.any(), (
        f"dt: {int(bad.sum())}/{bad.numel()} elements outside the tolerance "
        f"(worst uses {used:.3g}x)")
    # bn_bwd on the same inputs: the pass the hand-off replaces
    old, ogam, obet = EXT.bn_bwd(dx.reshape(-1, cin), t.reshape(-1, cin),
                                 gamma.to(torch.bfloat16), mean, rstd, None)
    # (bn_bwd returns them in gamma's dtype: the bound adds that rounding)
    assert ogam.dtype == torch.bfloat16 and obet.dtype == torch.bfloat16
    assert_gemm_close(ogam, r["dgam"].cpu(), r["dgam_mag"].cpu(), M + 3,
                      f"bn_bwd dgamma{shape}")
    assert_gemm_close(obet, r["dbet"].cpu(), r["dbet_mag"].cpu(), M,
                      f"bn_bwd dbeta{shape}")
    a, b = dt.double(), old.double()
    ndiff = int((dt.view(torch.int16) != old.view(torch.int16)).sum())
    print(f"HANDOFF dt{shape} differs from bn_bwd in {ndiff}/{dt.numel()} "
          f"elements")
    one_ulp = 2 * ULP * torch.maximum(a.abs(), b.abs())  # bf16 spacing
    assert ((a - b).abs() <= one_ulp + 2 * r["fp32"]).all()


def test_declined_shape_returns_masked_sum_and_no_workspace():
    n, h, cin, kout, r, stride, pad, _ = DECLINED
    dy, w, a, t, m, mean, rstd, _ = _inputs(*DECLINED)
    want, dx, ws = _run(DECLINED)
    assert ws is None
    _assert_identical(dx, want, "declined dx")
    # the separate passes of that route: addend in the dgrad, then relu_bwd
    sep = EXT.relu_bwd(EXT.conv2d_dgrad(dy, w, stride, pad, h, h, addend=a),
                       m)
    _assert_identical(dx, sep, "declined dx vs separate passes")
    assert (dx[~(m.float() > 0)] == 0).all()


# ------------------------------------------------------- model level -----


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


class _watch:
    """Counts bn_bwd_ws calls and replays every hand-off dgrad (a
    conv2d_dgrad_bnstats call with an addend) through the add+mask dgrad."""

    def __enter__(self):
        self.ws_calls = self.handoffs = self.with_ws = 0
        self.orig_ws, self.orig_dg = EXT.bn_bwd_ws, EXT.conv2d_dgrad_bnstats

        def counted(*a, **k):
            self.ws_calls += 1
            return self.orig_ws(*a, **k)

        def replayed(dy, w, stride, pad, H, W, mask, t, mean, rstd,
                     addend=None):
            dx, ws = self.orig_dg(dy, w, stride, pad, H, W, mask, t, mean,
                                  rstd, addend=addend)
            if addend is not None:
                self.handoffs += 1
                self.with_ws += ws is not None
                want = EXT.conv2d_dgrad(dy, w, stride, pad, H, W,
                                        addend=addend, out_mask=mask)
                _assert_identical(dx, want, f"hand-off dgrad {self.handoffs}")
            return dx, ws

        EXT.bn_bwd_ws, EXT.conv2d_dgrad_bnstats = counted, replayed
        return self

    def __exit__(self, *exc):
        EXT.bn_bwd_ws, EXT.conv2d_dgrad_bnstats = self.orig_ws, self.orig_dg


def _fwd_bwd(seq, x0):
    for p in seq.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    out = seq(x)
    out.float().square().mean().backward()
    res = {"out": out.detach().clone(), "x.grad": x.grad.clone()}
    for name, p in seq.named_parameters():
        res[name] = p.grad.clone()
    return res


# second block's constructor args, input shape
PAIRS = [((64, 64, 1), (2, 32, 32, 64)), ((64, 128, 2), (4, 32, 32, 64))]


@pytest.mark.parametrize("args,xshape", PAIRS, ids=_ids)
def test_wired_pair_matches_gate_off(args, xshape):
    from pytorch_ddp_template_amd.models.resnet import BasicBlock, wire_blocks
    from test_gpu_dgrad_bnstats import _assert_close

    torch.manual_seed(0)
    blocks = [BasicBlock(64, 64, 1), BasicBlock(*args)]
    wire_blocks(blocks)
    seq = torch.nn.Sequential(*blocks).to(torch.bfloat16).to(DEV)
    seq.train()
    x0 = torch.relu(torch.randn(*xshape)).to(torch.bfloat16).to(DEV)
    with _gate("0"), _watch() as w0:
        ref = _fwd_bwd(seq, x0)
    assert w0.handoffs == 0
    with _gate("1"), _watch() as w1:
        poison(DEV, x0.numel() * 64)
        got = _fwd_bwd(seq, x0)
    assert w1.handoffs == 1 and w1.with_ws == 1
    assert w1.ws_calls == w0.ws_calls + 1
    _assert_identical(got["out"], ref["out"], "forward output")
    _assert_close(got, ref)  # BLOCK_ULPS of max|ref|


def test_resnet18_matches_gate_off():
    from pytorch_ddp_template_amd.models import resnet18
    from pytorch_ddp_template_amd.ops import CrossEntropyLoss
    from test_gpu_dgrad_epilogue import MODEL_ULPS, _assert_close

    torch.manual_seed(3)
    model = resnet18(num_classes=10, stem="cifar").to(torch.bfloat16).to(DEV)
    model.train()
    crit = CrossEntropyLoss()
    x = torch.randn(4, 32, 32, 3).to(torch.bfloat16).to(DEV)
    y = torch.randint(0, 10, (4,)).to(DEV)

    def run():
        model.zero_grad(set_to_none=True)
        poison(DEV, x.numel() * 64 * 2)
        logits = model(x)
        crit(logits, y).backward()
        res = {"logits": logits.detach().clone()}
        for name, p in model.named_parameters():
            assert p.grad is not None, name
            res[name] = p.grad.clone()
        return res

    with _gate("0"), _watch() as w0:
        ref = run()
    assert w0.handoffs == 0
    with _gate("1"), _watch() as w1:
        got = run()
    # the stem and seven blocks offer; the 4x4 maps of layer4 are 64 rows,
    # which the glds kernel declines
    assert w1.handoffs == 8 and w1.with_ws == 7
    assert w1.ws_calls == w0.ws_calls + 7
    _assert_identical(got["logits"], ref["logits"], "logits")
    for k in ("stem.0.0.weight", "stem.0.1.weight", "stem.0.1.bias"):
        assert k in got
    _assert_close(got, ref, MODEL_ULPS)
