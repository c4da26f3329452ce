"""The MLP epilogue kinds of the 256x256 NT kernel (gemm_nt_epi), mlp_gelu on
top of them and one ViT block, against float64.

u = 2^-8 is bf16's unit roundoff, acc(mag, K) = 1.01 (K + 2) 2^-23 mag the
accumulation term of _errbound.gemm_bound, by = u |y| + acc that bound itself.
  bias_gelu y  one rounding of acc + bias: by.
  bias_gelu g  bf16(gelu(y_kernel)): sup|gelu'| < 1.13 carries y's error, plus
               g's own rounding: 1.13 by + u |g|.
  mul_dgelu    bf16(bf16(acc) gelu'(y)), y exact: |gelu'(y)| times the bound of
               bf16(acc), plus the product's rounding u |ref|.
  bias_res     one rounding of acc + bias + res: the GEMM bound with |res| in
               mag and depth K + 1 for the extra f32 add.
"""

import copy
import math

import pytest
import torch

import _errbound as eb
from pytorch_ddp_template_amd.models.vit import Block
from pytorch_ddp_template_amd.ops.functional import mlp_gelu
from pytorch_ddp_template_amd.ops.native import native as _ext

pytestmark = pytest.mark.gpu
DEV, BF = "cuda:0", torch.bfloat16
U = eb.EPS_OUT[BF]


def _gelu(t):
    return 0.5 * t * (1 + torch.erf(t / math.sqrt(2)))


def _dgelu(t):
    return (0.5 * (1 + torch.erf(t / math.sqrt(2)))
            + t * torch.exp(-0.5 * t * t) / math.sqrt(2 * math.pi))


def _acc(mag, depth):
    return eb.gemm_bound(torch.zeros_like(mag), mag, depth, torch.float32)


def _check(out, ref, bound, what):
    err = (out.detach().cpu().double() - ref).abs()
    print(f"MLPGELU {what} used={(err / bound).max().item():.4f}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} outside"


# one tile, prologue only; 8-row tail, two N tiles, one loop trip; the tail
# alone; two full tiles plus a tail (block remap)
@pytest.mark.parametrize("kind", ["bias_gelu", "mul_dgelu", "bias_res"])
@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (264, 512, 128),
                                   (1, 256, 192), (520, 256, 64)])
def test_gemm_nt_epi(M, N, K, kind):
    a = eb.randn(M, K, seed=1, dtype=BF)
    b = eb.randn(N, K, seed=2, scale=K ** -0.5, dtype=BF)
    bias = None if kind == "mul_dgelu" else eb.randn(N, seed=3, dtype=BF)
    aux = None if kind == "bias_gelu" else eb.randn(M, N, seed=4, dtype=BF)
    ref, mag, _ = eb.linear_ref(a, b, bias)
    args = [None if t is None else t.to(DEV) for t in (a, b, bias, aux)]
    eb.poison(DEV, 4 * M * N)
    c, c2 = _ext().gemm_nt_epi(*args[:3], kind, args[3])
    assert c.shape == (M, N) and c.dtype == BF
    assert c2.shape == ((M, N) if kind == "bias_gelu" else (0,))
    by = eb.gemm_bound(ref, mag, K, BF)
    if kind == "bias_gelu":
        _check(c, ref, by, "y")
        _check(c2, _gelu(ref), 1.13 * by + U * _gelu(ref).abs(), "g")
        # the formula shared with the backward: g is gelu_fwd of the stored y
        assert torch.equal(c2, _ext().gelu_fwd(c))
    elif kind == "mul_dgelu":
        gp = _dgelu(aux.double())
        _check(c, ref * gp, gp.abs() * by + U * (ref * gp).abs(), "dz")
    else:
        r = aux.double()
        _check(c, ref + r, eb.gemm_bound(ref + r, mag + r.abs(), K + 1, BF),
               "out")


@pytest.mark.parametrize("dtype,with_res", [(BF, False), (BF, True),
                                            (torch.float16, True)])
def test_mlp_gelu(dtype, with_res, monkeypatch):
    """Forward and every gradient against float64 autograd of the plain
    formula, fused route on (PDT_MLP_FUSED=1); fp16 still takes the composed
    route, which rounds at the same points and h once more.  First-order
    elementwise propagation (second order is below the 1.01; |gelu''| <= 0.8):
      ey = u|y| + acc;  eg = 1.13 ey + u|g|;  out: eg |w2|^T + acc + u|out|
      ez = |gelu'(y)| (u|a| + acc) + 0.8 |a| ey + u|z|,  a = dout w2
      dx: ez |w1|;  dw1: ez^T |x|;  db1: sum ez;  dw2: |dout|^T eg;  db2: 0;
      each + acc + u|ref|.  dresidual is dout itself, bit for bit."""
    monkeypatch.setenv("PDT_MLP_FUSED", "1")
    T, C, H = 264, 256, 1024
    u = eb.EPS_OUT[dtype]
    x, res, do = (eb.randn(T, C, seed=s, dtype=dtype) for s in (1, 2, 3))
    w1 = eb.randn(H, C, seed=4, scale=C ** -0.5, dtype=dtype)
    w2 = eb.randn(C, H, seed=5, scale=H ** -0.5, dtype=dtype)
    b1, b2 = eb.randn(H, seed=6, dtype=dtype), eb.randn(C, seed=7, dtype=dtype)
    cpu = [x, w1, b1, w2, b2, res]
    dev = [t.to(DEV).requires_grad_() for t in cpu]
    out = mlp_gelu(*dev[:5], dev[5] if with_res else None)
    assert (type(out.grad_fn).__name__ == "_MlpGeluFnBackward") == (dtype == BF)
    out.backward(do.to(DEV))

    X, W1, B1, W2, B2, R = (t.double().requires_grad_() for t in cpu)
    y = X @ W1.t() + B1
    g = _gelu(y)
    h = g @ W2.t() + B2
    ref = h + R if with_res else h
    ref.backward(do.double())
    with torch.no_grad():
        D, aX, aW1, aW2 = do.double().abs(), X.abs(), W1.abs(), W2.abs()
        ey = u * y.abs() + _acc(aX @ aW1.t() + B1.abs(), C)
        eg = 1.13 * ey + u * g.abs()
        mo = g.abs() @ aW2.t() + B2.abs() + (R.abs() if with_res else 0)
        twice = u * h.abs() if with_res and dtype != BF else 0
        _check(out, ref, 1.01 * (eg @ aW2.t() + _acc(mo, H + 1) + twice
                                 + u * ref.abs()), "out")
        a = do.double() @ W2
        z = a * _dgelu(y)
        ez = (_dgelu(y).abs() * (u * a.abs() + _acc(D @ aW2, C))
              + 0.8 * a.abs() * ey + u * z.abs())
        for name, got, want, prop, mag, depth in [
            ("dx", dev[0], X, ez @ aW1, z.abs() @ aW1, H),
            ("dw1", dev[1], W1, ez.t() @ aX, z.abs().t() @ aX, T),
            ("db1", dev[2], B1, ez.sum(0), z.abs().sum(0), T),
            ("dw2", dev[3], W2, D.t() @ eg, D.t() @ g.abs(), T),
            ("db2", dev[4], B2, 0.0, D.sum(0), T),
        ]:
            _check(got.grad, want.grad,
                   1.01 * (prop + _acc(mag, depth) + u * want.grad.abs()), name)
    if with_res:
        assert torch.equal(dev[5].grad.cpu(), do)


def test_vit_block_fused_agrees_with_composed(monkeypatch):
    """dim 256, 4 heads, 2 x 264 tokens.  The composed run's distance from
    the float64 reference is what the block's own bf16 rounding gives; the
    fused run must stay within FACTOR = 2 of it from the composed run."""
    FACTOR = 2.0
    torch.manual_seed(0)
    gpu = Block(256, 4).train().to(BF).to(DEV)
    x, do = (eb.randn(2, 264, 256, seed=s, dtype=BF) for s in (1, 2))

    def run(m, xin, dout, fused="0"):
        monkeypatch.setenv("PDT_MLP_FUSED", fused)
        xin = xin.clone().requires_grad_()
        out = m(xin)
        out.backward(dout)
        named = {"out": out.detach(), "dx": xin.grad}
        named.update({k: p.grad for k, p in m.named_parameters()})
        return {k: v.cpu().double() for k, v in named.items()}

    # the reference runs on the bf16-rounded parameters
    ref = run(copy.deepcopy(gpu).cpu().double(), x.double(), do.double())
    composed = run(copy.deepcopy(gpu), x.to(DEV), do.to(DEV))
    fused = run(copy.deepcopy(gpu), x.to(DEV), do.to(DEV), "1")
    for k in ref:
        yard = (composed[k] - ref[k]).abs().max().item()
        diff = (fused[k] - composed[k]).abs().max().item()
        print(f"MLPGELU block {k} fused-composed={diff:.3e} yard={yard:.3e}")
        assert diff <= FACTOR * yard, k
