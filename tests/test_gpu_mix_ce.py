"""Label smoothing / mixup / cutmix on the MI355X: loss and mix kernels against
float64, the draw against rng.mix_draw, hipGraph liveness, GraphStep wiring."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _errbound as eb
from pytorch_ddp_template_amd.ops import (BatchMix, CrossEntropyLoss,
                                          cross_entropy, rng)
from pytorch_ddp_template_amd.ops.native import native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SEED, RANK = (0x5EED << 32) | 0xC0FFEE, 3
U = 1.01 * eb.U32


def _state(next_call=0, step=0):
    rng.set_state({"seed": SEED, "rank": RANK, "next_call": next_call,
                   "step": step})



@pytest.mark.parametrize("eps,lam", [(0.1, 1.0), (0.0, 0.3), (0.1, 0.3),
                                     (0.1, None)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,D", [(1, 10), (5, 10), (5, 1000), (4, 1003),
                                 (3, 4104)])
def test_soft_ce_forward_backward_vs_float64(M, D, dtype, eps, lam):
    """Bounds per row, U = 1.01 * 2^-23 one ulp, rg = max z - min z, R =
    ceil(D/256) + 6 rescales a term can pass (lane trips + shuffle merges):
    * lse: an fp32 sum of D exps (D+2 ulp); an exp of argument x costs |x|+2
      ulp (log2e product, hardware exp2), |x| <= rg; R rescales whose arguments
      add up to <= rg (rg + 3R ulp); log |log s| + 1, the add |lse|:
      d_lse = U (D + 2 rg + 3 R + |log s| + |lse| + 8);
    * loss row: d_lse + the fp32 sum z of D terms times eps/D + 8 roundings of
      the target terms + 3 of the row magnitude; the mean adds M+2 roundings;
    * grad: sm (d_lse + (|z - lse| + 3) U) + 6 U (sm + q), times dloss/M, +
      the output rounding (fp16: + half a subnormal step, 2^-25)."""
    g = torch.Generator().manual_seed(M * D)
    z = torch.randn(M, D, generator=g) * 4 + 60
    z[0, 0] = z[0].max() + 8
    z[-1, D - 1] = z[-1].max() + 8
    z = z.to(dtype)
    t = torch.randint(0, D, (M,), generator=g)
    rec = None if lam is None else rng.mix_record(lam, lam, mode=1).to(DEV)
    lam = 1.0 if lam is None else float(np.float32(lam))
    zg, tg = z.to(DEV), t.to(DEV)
    eb.poison(DEV, 4 * M * D)
    loss, lse = native().ce_soft_fwd(zg, tg, eps, rec)
    dl = native().ce_soft_bwd(zg, tg, lse, torch.full((), 3.0, device=DEV),
                              eps, rec)

    zd = z.double()
    oh = F.one_hot(t, D).double()
    q = eps / D + (1 - eps) * (lam * oh + (1 - lam) * oh.flip(0))
    lse_ref = torch.logsumexp(zd, 1)
    rows = -(q * (zd - lse_ref[:, None])).sum(1)
    rg = zd.max(1).values - zd.min(1).values
    R = math.ceil(D / 256) + 6
    d_lse = U * (D + 2 * rg + 3 * R + (lse_ref - zd.max(1).values).abs()
                 + lse_ref.abs() + 8)
    hard = ((1 - eps) * (lam * oh + (1 - lam) * oh.flip(0)) * zd.abs()).sum(1)
    soft = eps / D * zd.abs().sum(1)
    d_row = d_lse + U * ((D + 2) * soft + 8 * hard
                         + 3 * (lse_ref.abs() + hard + soft))
    bound = d_row.mean() + U * (M + 2) * rows.abs().mean()
    err = abs(loss.item() - rows.mean().item())
    print(f"SOFTCE {M}x{D} {dtype} loss err={err:.3e} bound={bound:.3e}")
    assert err <= bound

    sm = torch.softmax(zd, 1)
    ref = (sm - q) * 3.0 / M
    d_el = (3.0 / M) * (sm * (d_lse[:, None] + U * ((zd - lse_ref[:, None]).abs() + 3))
                        + 6 * U * (sm + q))
    d_el = d_el + eb.EPS_OUT[dtype] * ref.abs() + (2.0 ** -25 if dtype == torch.float16 else 0)
    assert ((dl.cpu().double() - ref).abs() <= d_el).all()


def test_default_cross_entropy_is_the_hard_label_kernels_bit_for_bit():
    """M = 2: the mean is two atomic adds onto 0, the same bits either way."""
    z = eb.randn(2, 1000, seed=5, scale=4).to(DEV).requires_grad_(True)
    t = torch.tensor([7, 993], device=DEV)
    loss = cross_entropy(z, t)
    loss.backward(torch.full((), 3.0, device=DEV))
    want, lse = native().ce_fwd(z.detach(), t)
    assert torch.equal(loss.detach(), want)
    assert torch.equal(z.grad, native().ce_bwd(
        z.detach(), t, lse, torch.full((), 3.0, device=DEV)))



def _mixed(x, rec):
    """(float64 expectation, per-element magnitude) of the record on a CPU
    batch x; the layout rule is the models'."""
    ints = rec.view(torch.int32)
    a = float(rec[1]) if int(ints[6]) else 1.0
    y0, y1, x0, x1 = (int(v) for v in ints[2:6]) if int(ints[6]) else (0,) * 4
    nchw = x.shape[1] == 3 and x.shape[-1] != 3
    xd, xp = x.double(), x.double().flip(0)
    ref, mag = a * xd + (1 - a) * xp, a * xd.abs() + (1 - a) * xp.abs()
    box = (slice(None), slice(None), slice(y0, y1), slice(x0, x1)) if nchw \
        else (slice(None), slice(y0, y1), slice(x0, x1))
    ref[box], mag[box] = xp[box], xp[box].abs()
    return ref, mag


MIX_CASES = [(s, B, dt) for s in [(5, 7, 3), (3, 5, 7), (8, 8, 4), (8, 8, 3)]
             for B in (1, 2, 5) for dt in DTYPES]
MIX_CASES.append(((520, 256, 16), 2, torch.float32))


@pytest.mark.parametrize("shape,B,dtype", MIX_CASES, ids=str)
def test_batch_mix_kernel(shape, B, dtype):
    """(5,7,3) NHWC, (3,5,7) NCHW: 105 elements, the scalar route; (8,8,4),
    (8,8,3): whole vectors, box edges inside a vector; (520,256,16): a second
    grid-stride trip.  Copies are exact, the blend is three fp32 roundings."""
    if shape[0] == 520:
        assert 520 * 256 * 16 // 4 > native().mix_grid_cap() * native().mix_block()
    nchw = shape[0] == 3
    H, W = shape[1:] if nchw else shape[:2]
    x = eb.randn(B, *shape, seed=B, dtype=dtype)
    records = {
        "mixup": rng.mix_record(0.3, 0.3, mode=rng.MIX_MIXUP),
        "cutmix": rng.mix_record(0.6, 1.0, (1, 4, 2, 6), rng.MIX_CUTMIX),
        "empty": rng.mix_record(1.0, 1.0, (0, 0, 0, 0), rng.MIX_CUTMIX),
        "whole": rng.mix_record(0.0, 1.0, (0, H, 0, W), rng.MIX_CUTMIX),
        "off": rng.mix_record(),
    }
    for name, rec in records.items():
        xg = x.to(DEV)
        out = native().mix_batch_(xg, rec.to(DEV), H, W, 1 if nchw else shape[2])
        assert out.data_ptr() == xg.data_ptr()
        ref, mag = _mixed(x, rec)
        what = f"mix {name} {shape} B={B} {dtype}"
        if name == "mixup":
            eb.assert_gemm_close(xg, ref, mag, 1, what, out_dtype=dtype)
        else:
            assert torch.equal(xg.cpu(), ref.to(dtype)), what
        if B % 2:
            assert torch.equal(xg[B // 2].cpu(), x[B // 2]), what



@pytest.mark.parametrize("H,W", [(32, 32), (224, 224)])
@pytest.mark.parametrize("am,ac,prob,sw", [(0.8, 0, 1, 0.5), (0, 1.0, 1, 0.5),
                                           (0.8, 1.0, 0.5, 0.5),
                                           (0.2, 0, 1, 0.5)])
def test_draw_kernel_matches_the_float64_mirror(am, ac, prob, sw, H, W):
    """Steps 0..255.  Mode (the apply and the mixup/cutmix decision) always
    matches.  Off the mirror's knife-edge steps (at most 2%) the box and the
    corrected lambda match exactly, which pins the centre too, and lambda as
    drawn lies within lam (1-lam) (rx + ry) + 3 * 2^-24, rx = ry = ln2 * de +
    3 * 2^-23, de = (33/alpha) * 5 * 2^-23 + 2^-23 / alpha: X = exp2(log2(U) /
    alpha), |log2 U| <= 33; log2f and exp2f are good to 3 ulp, 1/alpha and the
    product round once each (5 ulp on the exponent), U rounds once (2^-24 / ln2
    on log2 U); X / (X + Y) turns the relative errors of X and Y into
    lam (1-lam) times their sum, plus three roundings."""
    cid, steps = 11, np.arange(256)
    buf = torch.zeros(256, 8, device=DEV)
    k0, k1 = SEED & 0xFFFFFFFF, ((SEED >> 32) ^ RANK) & 0xFFFFFFFF
    for s in range(256):
        _state(step=s)
        native().mix_draw(buf[s], rng.step_scalar(DEV), k0, k1, cid, H, W, am,
                          ac, prob, sw)
    gi = buf.cpu().view(torch.int32).numpy()
    gf = buf.cpu().numpy().astype(np.float64)
    d = rng.mix_draw(H, W, am, ac, prob, sw, cid, steps)
    assert (gi[:, 6] == d["mode"]).all()
    ok = ~d["knife"]
    assert (~ok).mean() <= 0.02
    box = np.stack([d[k] for k in ("y0", "y1", "x0", "x1")], axis=1)
    assert (gi[ok, 2:6] == box[ok]).all()
    cut = ok & (d["mode"] == rng.MIX_CUTMIX)
    assert (gf[cut, 0] == d["lam"][cut]).all() and (gf[cut, 1] == 1).all()
    off = d["mode"] == rng.MIX_NONE
    assert (gf[off][:, [0, 1, 7]] == 1).all()
    alpha = np.where(d["mode"] == rng.MIX_CUTMIX, ac or 1, am or 1)
    de = (33 / alpha) * 5 * 2.0 ** -23 + 2.0 ** -23 / alpha
    raw, live = d["raw"], ok & ~off
    bound = raw * (1 - raw) * 2 * (math.log(2) * de + 3 * 2.0 ** -23) + 3 * 2.0 ** -24
    assert (np.abs(gf[live, 7] - raw[live]) <= bound[live]).all()
    mixup = live & (d["mode"] == rng.MIX_MIXUP)
    assert (gf[mixup, 0] == gf[mixup, 7]).all() and (gf[mixup, 1] == gf[mixup, 7]).all()



def test_captured_mix_and_loss_draw_fresh_parameters_on_every_replay():
    """Captured as GraphStep does.  The call id (102) is baked in, the step is
    live: replay k holds the mirror's record of step k and uses it."""
    mix = BatchMix(0.8, 1.0)
    x0 = eb.randn(4, 8, 8, 3, seed=1, dtype=torch.bfloat16)
    xg, x_src = x0.to(DEV), x0.to(DEV)
    z = eb.randn(4, 10, seed=2, scale=4).to(DEV).requires_grad_(True)
    t = torch.tensor([1, 5, 5, 9], device=DEV)
    _state(next_call=100)
    mix.params(DEV)

    def inner():
        rng.tick(DEV)
        xg.copy_(x_src)
        mix.apply_(xg)
        loss = cross_entropy(z, t, 0.1, mix)
        return loss, torch.autograd.grad(loss, z)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            inner()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _state(next_call=102, step=0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        loss, gz = inner()
    seen = []
    for k in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        rec = mix.params(DEV).cpu()
        d = rng.mix_draw(8, 8, 0.8, 1.0, 1.0, 0.5, 102, k)
        assert not d["knife"]
        ints = rec.view(torch.int32).tolist()
        assert ints[2:7] == [d["y0"], d["y1"], d["x0"], d["x1"], d["mode"]]
        assert abs(float(rec[0]) - d["lam"]) <= 2e-5  # the draw test's bound
        ref, mag = _mixed(x0, rec)
        eb.assert_gemm_close(xg, ref, mag, 1, f"replay {k}", out_dtype=x0.dtype)
        oh, lam = F.one_hot(t.cpu(), 10).double(), float(rec[0])
        zd = z.detach().cpu().double().requires_grad_(True)
        want = F.cross_entropy(
            zd, 0.01 + 0.9 * (lam * oh + (1 - lam) * oh.flip(0)))
        assert abs(loss.item() - want.item()) <= 1e-4
        assert (gz.cpu().double() - torch.autograd.grad(want, zd)[0]
                ).abs().max() <= 1e-5
        seen.append(rec)
    assert not any(torch.equal(seen[i], seen[j]) for i, j in ((0, 1), (0, 2), (1, 2)))



@pytest.mark.parametrize("name", ["resnet18", "vit"])
def test_graph_step_with_smoothing_and_mix(name):
    from pytorch_ddp_template_amd.ddp import GraphStep
    from pytorch_ddp_template_amd.models import ViT, resnet18
    from pytorch_ddp_template_amd.optim import SGD

    torch.manual_seed(8)
    model = resnet18(num_classes=10, stem="cifar") if name == "resnet18" else ViT(
        image_size=32, patch_size=8, dim=128, depth=2, heads=2, num_classes=10)
    model = model.to(torch.bfloat16).to(DEV).train()
    before = [p.detach().clone() for p in model.parameters()]
    mix = BatchMix(0.8, 1.0)
    gs = GraphStep(model, CrossEntropyLoss(0.1, mix),
                   SGD(model.parameters(), lr=0.05, master_weights=True),
                   1000.0, mix)
    x = eb.randn(8, 32, 32, 3, seed=3, dtype=torch.bfloat16).to(DEV)
    y = torch.arange(8, device=DEV)
    _state()
    losses = [float(gs.step(x, y)) for _ in range(GraphStep.WARMUP + 2)]
    assert gs.active and all(math.isfinite(v) for v in losses), losses
    assert rng.get_state()["step"] == GraphStep.WARMUP + 2
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    with torch.no_grad():
        out = model.eval()(x)
        mix.apply_(x.clone())
        assert torch.equal(model(x), out)
