"""The fused Philox dropout / stochastic-depth / residual-add kernel on the
MI355X: masks against an independent numpy oracle (every dtype, the vector
body, the tail, a second grid-stride trip, the unaligned all-scalar route, the
per-vector and per-element row mask), values against a float64 reference with
a derived bound, backward, agreement with the CPU path, liveness under
hipGraph replay, and the ViT / GraphStep wiring."""

import functools
import math

import numpy as np
import pytest
import torch

import _errbound as eb
from pytorch_ddp_template_amd.ops import dropout_add, rng
from pytorch_ddp_template_amd.ops.native import native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SEED, RANK = (0x5EED << 32) | 0xC0FFEE, 3
PER_LANE = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}

# ------------------------------------------------ independent numpy oracle --


def philox(ctr, key):
    """Philox4x32-10.  ctr: four words (ints or uint64 arrays), key: two."""
    m = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, dtype=np.uint64) & m for v in ctr]
    k = [int(key[0]), int(key[1])]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & m,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & m]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


@functools.lru_cache(maxsize=None)
def oracle_words(n, seed, rank, call_id, step):
    """Word of element e = word (e & 3) of block (e >> 2, call lo, call hi,
    step) under key (seed lo, seed hi ^ rank).  Computed once per argument
    set and shared; callers must not write to it."""
    blk = np.arange((n + 3) // 4, dtype=np.uint64)
    key = (seed & 0xFFFFFFFF, ((seed >> 32) ^ rank) & 0xFFFFFFFF)
    w = philox((blk, call_id & 0xFFFFFFFF, call_id >> 32, step), key)
    out = np.stack(w, axis=1).reshape(-1)[:n]
    out.setflags(write=False)
    return out


def oracle_keep(n, p, call_id, step, seed=SEED, rank=RANK):
    if p == 0:
        return torch.ones(n, dtype=torch.bool)
    w = oracle_words(n, seed, rank, call_id, step)
    return torch.from_numpy(w >= np.uint64(math.floor(p * 2 ** 32)))


def test_oracle_matches_published_vectors():
    def hx(words):
        return " ".join("%08x" % int(w) for w in words)

    assert hx(philox((0, 0, 0, 0), (0, 0))) == (
        "6627e8d5 e169c58d bc57ac4c 9b00dbd8")
    assert hx(philox((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)) == (
        "408f276d 41c83b0e a20bc7c6 6d5451fd")
    assert hx(philox((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
                     (0xA4093822, 0x299F31D0))) == (
        "d16cfe09 94fdcceb 5001e420 24126ea1")


# ------------------------------------------------------------- helpers -----


def _state(next_call=0, step=0, seed=SEED, rank=RANK):
    rng.set_state({"seed": seed, "rank": rank, "next_call": next_call,
                   "step": step})


def _inputs(shape, dtype, seed):
    """x with |x| >= 0.5 (so no exact zeros, and res + x * s != res in every
    dtype), res ~ N(0, 1); both already rounded to dtype."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(shape, generator=g)
    x = torch.where(r < 0, r - 0.5, r + 0.5).to(dtype)
    res = torch.randn(shape, generator=g).to(dtype)
    return x, res


def _raw(x, res, cid_e, cid_r, p, p_row, inner, out=None):
    k0, k1 = rng.key()
    eb.poison(x.device, x.numel() * x.element_size())
    return native().dropout_fwd(x, res, out, rng.step_scalar(x.device), k0, k1,
                                cid_e, cid_r, p, p_row, inner)


def _check(out, x, res, keep, p, p_row, what):
    """keep: bool [numel] (CPU).  Dropped elements equal res (or 0) exactly,
    kept ones lie within the bound of the float64 reference."""
    dtype = out.dtype
    o = out.detach().cpu().reshape(-1)
    xd = x.detach().cpu().double().reshape(-1)
    rd = (torch.zeros_like(xd) if res is None
          else res.detach().cpu().double().reshape(-1))
    base = rd.to(dtype)
    assert torch.isfinite(o.float()).all(), f"{what}: non-finite output"
    # zero pattern / dropped == res exactly; kept != res (|x| >= 0.5)
    got_keep = o != base
    assert torch.equal(got_keep, keep), (
        f"{what}: mask differs from the oracle in "
        f"{int((got_keep != keep).sum())} of {keep.numel()} elements")
    s = (1.0 / (1.0 - p)) * (1.0 / (1.0 - p_row))
    ref = rd + torch.where(keep, xd * s, torch.zeros_like(xd))
    mag = rd.abs() + xd.abs() * s
    # five fp32 roundings: the two scales, the two products, the add
    eb.assert_gemm_close(o, ref, mag, 3, what, out_dtype=dtype)


def _grid_n(dtype):
    ext = native()
    return ext.dropout_grid_cap() * ext.dropout_block() * PER_LANE[dtype] + 13


# ---------------------------------------------------- element mask ---------

SIZES = [1, 3, 7, 8, 9, 4099, "second_trip"]


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_element_mask_and_values(dtype, n, with_res):
    """n = 'second_trip' is grid cap x block x elements per lane + 13: the
    grid-stride loop of the vector body takes a second trip, then the tail."""
    if n == "second_trip":
        n = _grid_n(dtype)
    p, cid, step = 0.3, (5 << 32) | 17, 9
    _state(step=step)
    x, res = _inputs((n,), dtype, seed=n % 1000)
    xg = x.to(DEV)
    rg = res.to(DEV) if with_res else None
    out = _raw(xg, rg, cid, 0, p, 0.0, 1)
    keep = oracle_keep(n, p, cid, step)
    _check(out, x, res if with_res else None, keep, p, 0.0,
           f"elem {dtype} n={n} res={with_res}")


# -------------------------------------------------------- row mask ---------

ROW_SHAPES = [(5, 91), (8, 64), (4, 197 * 64)]


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.4], ids=["rowonly", "elem+row"])
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_mask(dtype, shape, p, with_res):
    """(5, 91): rows end inside vectors (one draw per element's row);
    (8, 64): one row per vector; (4, 197*64): rows longer than a wave's span."""
    rows, inner = shape
    p_row, cid_e, cid_r, step = 0.5, 21, (1 << 32) | 22, 4
    _state(step=step)
    x, res = _inputs(shape, dtype, seed=rows * inner % 1000)
    out = _raw(x.to(DEV), res.to(DEV) if with_res else None, cid_e, cid_r, p,
               p_row, inner)
    keep_r = oracle_keep(rows, p_row, cid_r, step)
    assert 0 < int(keep_r.sum()) < rows, "shape must mix kept and dropped rows"
    keep = oracle_keep(rows * inner, p, cid_e, step) & (
        keep_r.repeat_interleave(inner))
    _check(out, x, res if with_res else None, keep, p, p_row,
           f"row {dtype} {shape} p={p} res={with_res}")


# -------------------------------------------------------- alignment --------


@pytest.mark.parametrize("which", ["x", "res", "out"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_unaligned_pointer_matches_aligned_bit_for_bit(dtype, which):
    """A contiguous view at a one-element storage offset is 2 B off the 16-B
    grid: the launcher must take the all-scalar route and draw the same bits."""
    rows, inner = 7, 587
    n = rows * inner
    _state(step=2)
    x, res = _inputs((rows, inner), dtype, seed=77)
    xg, rg = x.to(DEV), res.to(DEV)
    want = _raw(xg, rg, 8, 9, 0.3, 0.4, inner)

    def off(t):
        base = torch.empty(n + 1, dtype=dtype, device=DEV)
        v = base[1:].view(rows, inner)
        if t is not None:
            v.copy_(t)
        assert v.data_ptr() % 16 == 2 and v.is_contiguous()
        return v

    args = {"x": xg, "res": rg, "out": None}
    args[which] = off(None if which == "out" else args[which])
    if which == "out":
        args["out"].fill_(float("nan"))
    got = _raw(args["x"], args["res"], 8, 9, 0.3, 0.4, inner, out=args["out"])
    if which == "out":
        assert got.data_ptr() == args["out"].data_ptr()
    assert torch.equal(got, want)
    keep = oracle_keep(n, 0.3, 8, 2) & oracle_keep(
        rows, 0.4, 9, 2).repeat_interleave(inner)
    _check(got, x, res, keep, 0.3, 0.4, f"unaligned {which} {dtype}")


# ------------------------------------------- backward / CPU agreement ------


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_is_the_forward_kernel_on_dy(dtype):
    rows, inner = 6, 200
    _state(next_call=30, step=7)
    x, res = _inputs((rows, inner), dtype, seed=31)
    dy, _ = _inputs((rows, inner), dtype, seed=32)
    xg = x.to(DEV).requires_grad_(True)
    rg = res.to(DEV).requires_grad_(True)
    dyg = dy.to(DEV)
    y = dropout_add(xg, rg, 0.5, 0.25, True)
    assert rng.get_state()["next_call"] == 32  # one id per mask
    y.backward(dyg)
    assert torch.equal(rg.grad, dyg)
    want = _raw(dyg, None, 30, 31, 0.5, 0.25, inner)
    assert torch.equal(xg.grad, want)
    keep = oracle_keep(rows * inner, 0.5, 30, 7) & oracle_keep(
        rows, 0.25, 31, 7).repeat_interleave(inner)
    _check(xg.grad, dy, None, keep, 0.5, 0.25, f"dx {dtype}")
    _check(y, x, res, keep, 0.5, 0.25, f"y {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gpu_and_cpu_paths_agree(dtype):
    rows, inner = 9, 130
    x, res = _inputs((rows, inner), dtype, seed=41)
    _state(next_call=50, step=3)
    yc = dropout_add(x, res, 0.2, 0.3, True)
    _state(next_call=50, step=3)
    yg = dropout_add(x.to(DEV), res.to(DEV), 0.2, 0.3, True).cpu()
    keep_c = (yc != res).reshape(-1)
    assert torch.equal((yg != res).reshape(-1), keep_c)
    _check(yg, x, res, keep_c, 0.2, 0.3, f"gpu-vs-cpu {dtype}")
    _check(yc, x, res, keep_c, 0.2, 0.3, f"cpu {dtype}")


# ------------------------------------------------------- graph capture -----


def test_captured_call_draws_a_fresh_oracle_mask_on_every_replay():
    """tick(); dropout_add; backward captured on a side stream as GraphStep
    does.  The call ids are baked in; the step scalar is read live, so replay
    k draws the oracle mask at step k, and backward regenerates it."""
    rows, inner = 16, 264
    n = rows * inner
    dtype = torch.bfloat16
    x, res = _inputs((rows, inner), dtype, seed=61)
    dy, _ = _inputs((rows, inner), dtype, seed=62)
    xg = x.to(DEV).requires_grad_(True)
    rg = res.to(DEV).requires_grad_(True)
    dyg = dy.to(DEV)
    _state(next_call=100)

    def inner_step():
        rng.tick(DEV)
        y = dropout_add(xg, rg, 0.5, 0.25, True)
        gx, gr = torch.autograd.grad(y, (xg, rg), dyg)
        return y, gx, gr

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            inner_step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    st = rng.get_state()
    assert st["next_call"] == 104 and st["step"] == 2
    rng.set_state(dict(st, step=0))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        y, gx, gr = inner_step()
    assert rng.get_state() == dict(st, step=0, next_call=106)
    masks = []
    for k in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        assert rng.get_state()["step"] == k
        keep = oracle_keep(n, 0.5, 104, k) & oracle_keep(
            rows, 0.25, 105, k).repeat_interleave(inner)
        _check(y, x, res, keep, 0.5, 0.25, f"replay {k} y")
        assert torch.equal((gx.cpu() != 0).reshape(-1), keep), (
            f"replay {k}: backward's mask differs from forward's")
        assert torch.equal(gr, dyg)
        masks.append(keep)
    assert not torch.equal(masks[0], masks[1])
    assert not torch.equal(masks[1], masks[2])
    assert not torch.equal(masks[0], masks[2])


# ------------------------------------------------------------- models ------


def _tiny_vit(dropout=0.1, drop_path=0.1, heads=4):
    from pytorch_ddp_template_amd.models.vit import ViT

    return ViT(image_size=32, patch_size=8, dim=64, depth=2, heads=heads,
               num_classes=10, dropout=dropout, drop_path=drop_path)


def _fwd_bwd_f32(model, x, y):
    from pytorch_ddp_template_amd.ops import CrossEntropyLoss

    _state(next_call=0, step=0)  # the same masks in every run
    model.zero_grad(set_to_none=True)
    logits = model(x)
    CrossEntropyLoss()(logits, y).backward()
    out = {"logits": logits.detach().cpu()}
    for n, p in model.named_parameters():
        assert p.grad is not None, f"{n}: no gradient"
        out[n] = p.grad.detach().cpu()
    return out


def test_vit_tiny_f32_with_dropout_matches_cpu():
    """Yardstick of test_gpu_models.py::test_vit_tiny_f32_fwd_bwd_matches_cpu
    with dropout 0.1 and drop_path 0.1 in train mode: logits and every
    parameter gradient within 8x the CPU path's own sensitivity to a +-1 ulp
    perturbation of the input (4 seeded draws, largest change per tensor,
    normalised by max|tensor|).  The rng state is set identically before
    every run, the perturbed CPU runs included."""
    g = torch.Generator().manual_seed(13)
    x = torch.randn(4, 32, 32, 3, generator=g)
    y = torch.randint(0, 10, (4,), generator=g)
    torch.manual_seed(11)
    m = _tiny_vit()
    m.train()
    mg = _tiny_vit()
    mg.load_state_dict(m.state_dict())
    mg.train()
    mg = mg.to(DEV)
    base = _fwd_bwd_f32(m, x, y)
    assert rng.get_state()["next_call"] > 0
    noise = {k: 0.0 for k in base}
    for seed in range(4):
        g = torch.Generator().manual_seed(100 + seed)
        up = torch.randint(0, 2, x.shape, generator=g).bool()
        inf = torch.full_like(x, float("inf"))
        xp = torch.nextafter(x, torch.where(up, inf, -inf))
        pert = _fwd_bwd_f32(m, xp, y)
        for k, t in base.items():
            d = ((pert[k] - t).abs().max() / t.abs().max()).item()
            noise[k] = max(noise[k], d)
    got = _fwd_bwd_f32(mg, x.to(DEV), y.to(DEV))
    bad = []
    for k, t in base.items():
        err = ((got[k] - t).abs().max() / t.abs().max()).item()
        print(f"MODELF32 vit_tiny_dropout {k} err={err:.3e} "
              f"noise={noise[k]:.3e} "
              f"ratio={err / noise[k] if noise[k] else float('inf'):.2f}")
        if not err <= 8 * noise[k]:
            bad.append(f"{k}: err {err:.3e} > 8 * noise {noise[k]:.3e}")
    assert not bad, "; ".join(bad)


def test_vit_tiny_bf16_fused_attention_with_dropout():
    """heads 1, dim 64 -> head size 64: the fused-attention route.  Train mode
    gives a finite loss and finite grads; eval mode equals the rate-0 model
    with the same weights bit for bit."""
    from pytorch_ddp_template_amd.ops import CrossEntropyLoss

    torch.manual_seed(4)
    plain = _tiny_vit(0.0, 0.0, heads=1).to(torch.bfloat16).to(DEV)
    reg = _tiny_vit(0.1, 0.1, heads=1).to(torch.bfloat16).to(DEV)
    reg.load_state_dict(plain.state_dict())
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 32, 32, 3, generator=g).to(torch.bfloat16).to(DEV)
    y = torch.randint(0, 10, (4,), generator=g).to(DEV)
    _state()
    reg.train()
    loss = CrossEntropyLoss()(reg(x), y)
    loss.backward()
    assert rng.get_state()["next_call"] > 0
    assert math.isfinite(float(loss))
    for n, p in reg.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad.float()).all(), n
    with torch.no_grad():
        assert torch.equal(reg.eval()(x), plain.eval()(x))
        assert not torch.equal(reg.train()(x), plain.train()(x))


def test_graph_step_with_dropout_ticks_and_keeps_the_mask_live():
    """GraphStep driven directly with the tiny ViT (the CLI builds only the
    named models): 3 eager warm-up steps, then 4 replayed ones.  Ticks by
    construction: 3 (warm-ups run _inner eagerly) + 0 (the capture pass
    records the add without running it) + 4 (one per replay) = 7.  With lr 0
    the weights never move, so two replays on the same batch can differ in
    loss only through the masks."""
    from pytorch_ddp_template_amd.ddp import GraphStep
    from pytorch_ddp_template_amd.ops import CrossEntropyLoss
    from pytorch_ddp_template_amd.optim import SGD

    torch.manual_seed(6)
    model = _tiny_vit(0.1, 0.1, heads=1).to(torch.bfloat16).to(DEV)
    model.train()
    opt = SGD(model.parameters(), lr=0.0)
    gs = GraphStep(model, CrossEntropyLoss(), opt, 1000.0)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(8, 32, 32, 3, generator=g).to(torch.bfloat16).to(DEV)
    y = torch.randint(0, 10, (8,), generator=g).to(DEV)
    _state()
    losses = []
    for i in range(GraphStep.WARMUP + 4):
        losses.append(float(gs.step(x, y)))
        assert gs.active == (i >= GraphStep.WARMUP)
    assert all(math.isfinite(v) for v in losses), losses
    assert rng.get_state()["step"] == GraphStep.WARMUP + 4
    replayed = losses[GraphStep.WARMUP:]
    assert len(set(replayed)) > 1, f"frozen mask: {replayed}"
