"""Fused multi-tensor AdamW on the GPU (mt::adamw_kernel through
optim.AdamW): numerics against torch.optim.AdamW, master weights, the
optimizer-wide device step scalar across plans / groups / skipped steps /
graph replays, the device lr, and the --optimizer adamw engine path.

fp32 state is checked with _errbound.assert_calibrated: ``gpu`` is ours,
``cpu`` is torch.optim.AdamW in fp32 on the CPU (the yardstick), ``ref`` is
torch.optim.AdamW in float64.  Compared are exp_avg, exp_avg_sq and the
UPDATE p_T - p_0 (p_T itself would hide an error in the update behind the
parameter's magnitude); lr=1e-2 and weight_decay=0.1 keep the update well
above rounding.
"""

import pytest
import torch

from _errbound import CAL_FLOOR, EPS_OUT, assert_calibrated

pytestmark = pytest.mark.gpu

DEV = "cuda"
KW = dict(lr=1e-2, weight_decay=0.1)

# every path of an 8192-element chunk with a four-wide body: tail only (1, 3),
# body + tail below one chunk (130), exactly one chunk (8192), a chunk plus a
# body-less tail chunk (8197), several chunks with a partial last one (24580)
SIZES = [1, 3, 130, 8192, 8197, 24580]
# more than the 512 tensors of one launch plan: two plans
MANY = [7] * 520 + [8197]


def _randn_list(sizes, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).to(dtype) for n in sizes]


def _leaf(ts, device="cpu", dtype=None):
    return [t.detach().to(device=device, dtype=dtype or t.dtype).clone()
            .requires_grad_(True) for t in ts]


def _set_grads(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = g.to(device=p.device, dtype=p.dtype).clone()


def _cat(ts):
    return torch.cat([t.detach().reshape(-1).cpu() for t in ts])


def _torch_adamw(init, grads_per_step, dtype, split=None, **kw):
    """torch.optim.AdamW on the CPU in ``dtype`` from ``init`` (a list of
    CPU tensors, upcast exactly) -> (flat moments and update, params)."""
    ps = _leaf(init, dtype=dtype)
    groups = ps if split is None else [
        {"params": ps[:split]}, {"params": ps[split:]}]
    opt = torch.optim.AdamW(groups, **kw)
    for gs in grads_per_step:
        _set_grads(ps, gs)
        opt.step()
    p0 = [t.to(dtype) for t in init]
    return {
        "exp_avg": _cat([opt.state[p]["exp_avg"] for p in ps]),
        "exp_avg_sq": _cat([opt.state[p]["exp_avg_sq"] for p in ps]),
        "update": _cat([p.detach() - q for p, q in zip(ps, p0)]),
    }, ps


def _ours(init, grads_per_step, split=None, master=False, **kw):
    from pytorch_ddp_template_amd.optim import AdamW

    ps = _leaf(init, device=DEV)
    groups = ps if split is None else [
        {"params": ps[:split]}, {"params": ps[split:]}]
    opt = AdamW(groups, master_weights=master, **kw)
    for gs in grads_per_step:
        _set_grads(ps, gs)
        opt.step()
    torch.cuda.synchronize()
    return opt, ps


def _flat_state(opt, ps, init, master):
    work = [opt.state[p]["master"] for p in ps] if master else ps
    return {
        "exp_avg": _cat([opt.state[p]["exp_avg"] for p in ps]),
        "exp_avg_sq": _cat([opt.state[p]["exp_avg_sq"] for p in ps]),
        "update": _cat([w.detach().cpu() - q.float()
                        for w, q in zip(work, init)]),
    }


def test_adamw_fp32_matches_torch():
    init = _randn_list(SIZES, 0)
    grads = [_randn_list(SIZES, 10 + s) for s in range(4)]
    opt, ps = _ours(init, grads, **KW)
    cpu, _ = _torch_adamw(init, grads, torch.float32, **KW)
    ref, _ = _torch_adamw(init, grads, torch.float64, **KW)
    for p in ps:
        assert opt.state[p]["exp_avg"].dtype == torch.float32
    assert float(opt._step_t) == 4.0
    assert_calibrated("adamw_f32", _flat_state(opt, ps, init, False), cpu, ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "fp16"])
def test_adamw_master_weights_match_torch(dtype):
    init = _randn_list(SIZES, 1, dtype)
    grads = [_randn_list(SIZES, 20 + s, dtype) for s in range(4)]
    opt, ps = _ours(init, grads, master=True, **KW)
    # torch fp32 / float64 from the rounded start, on the rounded grads
    cpu, _ = _torch_adamw(init, grads, torch.float32, **KW)
    ref, _ = _torch_adamw(init, grads, torch.float64, **KW)
    for p in ps:
        st = opt.state[p]
        assert st["master"].dtype == torch.float32
        assert st["exp_avg"].dtype == torch.float32
        assert st["exp_avg_sq"].dtype == torch.float32
        assert p.dtype == dtype
        assert torch.equal(p.detach(), st["master"].to(dtype))
    assert_calibrated(f"adamw_master_{dtype}".replace("torch.", ""),
                      _flat_state(opt, ps, init, True), cpu, ref)


def test_adamw_bf16_without_master_one_step():
    """The kernel computes in fp32 and rounds once: |p - ref64| stays within
    one bf16 unit roundoff of |ref64| plus the calibrated fp32 floor (2^-20
    of max|ref64|) for the fp32 arithmetic before that rounding."""
    dtype = torch.bfloat16
    init = _randn_list(SIZES, 2, dtype)
    grads = [_randn_list(SIZES, 30, dtype)]
    opt, ps = _ours(init, grads, **KW)
    _, ref_ps = _torch_adamw(init, grads, torch.float64, **KW)
    got = _cat(ps).double()
    ref = _cat(ref_ps)
    bound = EPS_OUT[dtype] * ref.abs() + CAL_FLOOR * ref.abs().max()
    err = (got - ref).abs()
    print(f"ADAMW bf16 no-master used={(err / bound).max().item():.4f}")
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (err / bound).max().item()
    assert not torch.equal(got, _cat(init).double())
    for p in ps:
        assert "master" not in opt.state[p]


def test_adamw_more_than_512_tensors_one_tick_per_step():
    """Two launch plans per step.  A step count that ticked per plan would
    put bc1 off by ~40% at t = 2, far outside the calibrated tolerance."""
    init = _randn_list(MANY, 3)
    grads = [_randn_list(MANY, 40 + s) for s in range(3)]
    opt, ps = _ours(init, grads, **KW)
    cpu, _ = _torch_adamw(init, grads, torch.float32, **KW)
    ref, _ = _torch_adamw(init, grads, torch.float64, **KW)
    assert float(opt._step_t) == 3.0
    assert_calibrated("adamw_many", _flat_state(opt, ps, init, False), cpu, ref)


def test_adamw_guard_skips_on_device_once_per_step():
    init = _randn_list(MANY, 4)
    # two groups, the first of them two plans: three launches per step
    opt, ps = _ours(init, [_randn_list(MANY, 50)], split=515, **KW)
    snap = lambda: (  # noqa: E731
        [p.detach().clone() for p in ps],
        [opt.state[p]["exp_avg"].clone() for p in ps],
        [opt.state[p]["exp_avg_sq"].clone() for p in ps],
        opt._step_t.clone(),
    )
    p0, m0, v0, t0 = snap()
    assert float(t0) == 1.0
    skip = torch.zeros((), device=DEV)
    _set_grads(ps, _randn_list(MANY, 51))
    opt.step(guard=torch.tensor(float("inf"), device=DEV), skip_count=skip)
    torch.cuda.synchronize()
    p1, m1, v1, t1 = snap()
    for a, b in zip(p0 + m0 + v0 + [t0], p1 + m1 + v1 + [t1]):
        assert torch.equal(a, b)
    assert float(skip) == 1.0
    opt.step(guard=torch.tensor(3.0, device=DEV), skip_count=skip)
    torch.cuda.synchronize()
    p2, m2, v2, t2 = snap()
    assert all(not torch.equal(a, b) for a, b in zip(p1, p2))
    assert all(not torch.equal(a, b) for a, b in zip(m1, m2))
    assert float(t2) == 2.0
    assert float(skip) == 1.0


def test_adamw_device_lr_wins():
    init = _randn_list(SIZES, 5)
    grads = _randn_list(SIZES, 60)
    from pytorch_ddp_template_amd.optim import AdamW

    pa, pb = _leaf(init, device=DEV), _leaf(init, device=DEV)
    a = AdamW(pa, lr=99.0, weight_decay=0.1)
    b = AdamW(pb, lr=0.25, weight_decay=0.1)
    _set_grads(pa, grads)
    _set_grads(pb, grads)
    a.step(lr_tensor=torch.tensor(0.25, device=DEV))
    b.step()
    torch.cuda.synchronize()
    for x, y, i in zip(pa, pb, init):
        assert torch.equal(x.detach(), y.detach())
        assert torch.isfinite(x).all()
        # one AdamW step moves every element by about lr
        assert ((x.detach().cpu() - i).abs() < 1.0).all()


def test_adamw_graph_capture_follows_live_step_and_lr():
    """GraphStep's recipe: three eager warm-ups on a side stream, one capture
    of step(lr_tensor=lr_dev) on static grads, replays with refilled grads
    and a changed lr_dev.  The kernel is elementwise and deterministic, so an
    eager optimizer doing the same 3 + 1 + 3 steps must end bit-equal — which
    it can only if t and lr are read live on every replay."""
    from pytorch_ddp_template_amd.optim import AdamW

    init = _randn_list(SIZES, 6)
    n_steps = 7
    grads = [_randn_list(SIZES, 70 + s) for s in range(n_steps)]
    lrs = [1e-2, 2e-2, 5e-3, 1e-2, 3e-2, 1e-3, 7e-3]

    pg, pe = _leaf(init, device=DEV), _leaf(init, device=DEV)
    og = AdamW(pg, lr=99.0, weight_decay=0.1)
    oe = AdamW(pe, lr=99.0, weight_decay=0.1)
    for p in pg + pe:
        p.grad = torch.zeros_like(p)  # static grad tensors
    lr_g = torch.zeros((), device=DEV)
    lr_e = torch.zeros((), device=DEV)

    def feed(ps, lr_dev, s):
        for p, g in zip(ps, grads[s]):
            p.grad.copy_(g)
        lr_dev.fill_(lrs[s])

    for s in range(n_steps):  # the eager twin
        feed(pe, lr_e, s)
        oe.step(lr_tensor=lr_e)

    side = torch.cuda.Stream()
    for s in range(3):
        feed(pg, lr_g, s)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            og.step(lr_tensor=lr_g)
        torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    feed(pg, lr_g, 3)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        og.step(lr_tensor=lr_g)
    graph.replay()  # capture records without executing: this is step 4
    for s in range(4, n_steps):
        feed(pg, lr_g, s)
        graph.replay()
    torch.cuda.synchronize()

    assert float(og._step_t) == float(n_steps)
    assert torch.equal(og._step_t, oe._step_t)
    for a, b in zip(pg, pe):
        assert torch.equal(a.detach(), b.detach())
        assert torch.equal(og.state[a]["exp_avg"], oe.state[b]["exp_avg"])
        assert torch.equal(og.state[a]["exp_avg_sq"],
                           oe.state[b]["exp_avg_sq"])


def test_vit_tiny_bf16_trains_with_adamw():
    from pytorch_ddp_template_amd.models.vit import ViT
    from pytorch_ddp_template_amd.ops import CrossEntropyLoss
    from pytorch_ddp_template_amd.optim import (
        AdamW, clip_grad_norm_, param_groups_no_decay,
    )

    torch.manual_seed(4)
    m = (
        ViT(image_size=32, patch_size=8, dim=64, depth=2, heads=4,
            num_classes=10)
        .to(torch.bfloat16)
        .to(DEV)
    )
    groups = param_groups_no_decay(m, 0.05)
    assert len(groups) == 2
    opt = AdamW(groups, lr=1e-3, master_weights=True)
    crit = CrossEntropyLoss()
    x = torch.randn(8, 32, 32, 3).to(torch.bfloat16).to(DEV)
    y = torch.randint(0, 10, (8,)).to(DEV)
    losses = []
    for _ in range(12):
        loss = crit(m(x), y)
        loss.backward()
        clip_grad_norm_(list(m.parameters()), 1000.0)
        opt.step()
        m.zero_grad()
        losses.append(float(loss.detach()))
    print("ADAMW vit_tiny losses", [round(v, 4) for v in losses])
    assert losses[-1] < losses[0] * 0.5, (losses[0], losses[-1])


# ---------------------------------------------------------------- engine ----


def _run(tmp_path, extra):
    from pytorch_ddp_template_amd.ddp import main

    argv = [
        "--model", "resnet18", "--dataset", "cifar", "--dataset_size", "512",
        "--per_gpu_train_batch_size", "64", "--max_steps", "3",
        "--logging_steps", "1", "--save_steps", "2",
        "--output_dir", str(tmp_path / "out"), "--num_workers", "0",
        "--no_tensorboard", "--no_progress_bar", "--seed", "3",
        "--optimizer", "adamw", "--weight_decay", "0.05",
        "--learning_rate", "1e-3",
    ] + extra
    main(argv)
    return tmp_path / "out"


def test_engine_adamw_bf16_checkpoint_and_resume(tmp_path):
    out = _run(tmp_path, ["--bf16", "--max_steps", "4", "--save_steps", "2"])
    ck = out / "checkpoint-2"
    assert (ck / "model.bin").exists()
    sd = torch.load(ck / "optimizer.pt", map_location="cpu",
                    weights_only=True)
    assert len(sd["param_groups"]) == 2
    assert float(sd["step"]) == 2.0
    st = next(iter(sd["state"].values()))
    assert st["exp_avg"].dtype == torch.float32
    assert st["exp_avg_sq"].dtype == torch.float32
    assert st["master"].dtype == torch.float32
    # second run resumes from step 2 and must complete steps 3..4
    _run(tmp_path, ["--bf16", "--max_steps", "4", "--save_steps", "4",
                    "--global-step", "2"])
    sd = torch.load(out / "checkpoint-4" / "optimizer.pt",
                    map_location="cpu", weights_only=True)
    assert float(sd["step"]) == 4.0


def test_engine_adamw_hip_graph(tmp_path):
    from pytorch_ddp_template_amd.models import build_model

    out = _run(tmp_path, ["--bf16", "--hip_graph", "--max_steps", "8",
                          "--save_steps", "8"])
    ck = out / "checkpoint-8"
    sd = torch.load(ck / "model.bin", map_location="cpu", weights_only=True)
    init = build_model("resnet18", 10).to(torch.bfloat16).state_dict()
    moved = sum(
        1 for k in sd
        if k in init and sd[k].shape == init[k].shape
        and not torch.equal(sd[k], init[k])
    )
    assert moved > 10, f"only {moved} tensors changed — frozen capture?"
    for v in sd.values():
        assert torch.isfinite(v.float()).all()
    osd = torch.load(ck / "optimizer.pt", map_location="cpu",
                     weights_only=True)
    assert float(osd["step"]) == 8.0  # t ticked on every replay


def test_engine_adamw_fp16_scaler(tmp_path):
    out = _run(tmp_path, ["--fp16", "--loss_scale", "0"])  # dynamic scale
    assert (out / "checkpoint-2" / "model.bin").exists()
    assert (out / "checkpoint-2" / "optimizer.pt").exists()
