"""AdamW on the CPU reference path: parity with torch.optim.AdamW, master
weights, the guard / step-scalar semantics, checkpoint round trip, the
no-decay param groups and the --optimizer adamw engine path."""

import io
import os

import pytest
import torch

from pytorch_ddp_template_amd.optim import AdamW, param_groups_no_decay

RTOL, ATOL = 1e-5, 1e-6  # tests/test_optim.py's fp32 tolerances

SHAPES = [(20, 10), (10,), (7, 3), (5,)]


def _params(seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(dtype) for s in SHAPES]


def _grads(seed, step, dtype=torch.float32):
    g = torch.Generator().manual_seed(1000 * seed + step)
    return [torch.randn(s, generator=g).to(dtype) for s in SHAPES]


def _groups(ps, wd_a, wd_b):
    return [{"params": ps[:2], "weight_decay": wd_a},
            {"params": ps[2:], "weight_decay": wd_b}]


def _leaf(ts):
    return [t.detach().clone().requires_grad_(True) for t in ts]


def _set_grads(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = g.clone().to(p.dtype)


@pytest.mark.parametrize(
    "kw",
    [
        dict(lr=1e-3),
        dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-6),
    ],
    ids=["defaults", "custom"],
)
def test_adamw_fp32_matches_torch(kw):
    wd_a, wd_b = (1e-2, 0.0) if "betas" not in kw else (0.1, 0.03)
    init = _params(0)
    p1, p2 = _leaf(init), _leaf(init)
    ours = AdamW(_groups(p1, wd_a, wd_b), **kw)
    ref = torch.optim.AdamW(_groups(p2, wd_a, wd_b), **kw)
    for s in range(5):
        gs = _grads(0, s)
        _set_grads(p1, gs)
        _set_grads(p2, gs)
        ours.step()
        ref.step()
    for a, b in zip(p1, p2):
        torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(ours.state[a]["exp_avg"],
                                   ref.state[b]["exp_avg"],
                                   rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(ours.state[a]["exp_avg_sq"],
                                   ref.state[b]["exp_avg_sq"],
                                   rtol=RTOL, atol=ATOL)
    assert float(ours._step_t) == 5.0


def test_adamw_defaults_signature():
    p = _leaf(_params(1))
    opt = AdamW(p, lr=1e-3)
    g = opt.param_groups[0]
    assert g["betas"] == (0.9, 0.999)
    assert g["eps"] == 1e-8
    assert g["weight_decay"] == 1e-2
    assert g["master_weights"] is False
    with pytest.raises(ValueError):
        AdamW(p, lr=1e-3, betas=(1.0, 0.999))


def test_adamw_bf16_master_weights():
    init = _params(2, torch.bfloat16)
    p1 = _leaf(init)
    p2 = _leaf([t.float() for t in init])  # fp32 from the bf16-rounded start
    kw = dict(lr=1e-2, weight_decay=0.1)
    ours = AdamW(p1, master_weights=True, **kw)
    ref = torch.optim.AdamW(p2, **kw)
    for s in range(4):
        gs = _grads(2, s, torch.bfloat16)
        _set_grads(p1, gs)
        _set_grads(p2, [g.float() for g in gs])  # the bf16 grads, upcast
        ours.step()
        ref.step()
    for a, b in zip(p1, p2):
        st = ours.state[a]
        assert st["master"].dtype == torch.float32
        assert st["exp_avg"].dtype == torch.float32
        assert st["exp_avg_sq"].dtype == torch.float32
        torch.testing.assert_close(st["master"], b.detach(),
                                   rtol=RTOL, atol=ATOL)
        assert torch.equal(a.detach(), st["master"].to(torch.bfloat16))


def test_adamw_guard_skips_whole_step_once():
    init = _params(3)
    p1, p2 = _leaf(init), _leaf(init)
    kw = dict(lr=1e-2)
    ours = AdamW(_groups(p1, 0.1, 0.0), **kw)
    ref = torch.optim.AdamW(_groups(p2, 0.1, 0.0), **kw)
    gs = _grads(3, 0)
    # one good step so that the moments exist and are non-zero
    _set_grads(p1, gs)
    _set_grads(p2, gs)
    ours.step(guard=torch.tensor(1.0))
    ref.step()
    before_p = [p.detach().clone() for p in p1]
    before_m = [ours.state[p]["exp_avg"].clone() for p in p1]
    before_v = [ours.state[p]["exp_avg_sq"].clone() for p in p1]
    before_t = ours._step_t.clone()
    skip = torch.zeros(())
    gs = _grads(3, 1)
    _set_grads(p1, gs)
    ours.step(guard=torch.tensor(float("inf")), skip_count=skip)
    for p, bp, bm, bv in zip(p1, before_p, before_m, before_v):
        assert torch.equal(p.detach(), bp)
        assert torch.equal(ours.state[p]["exp_avg"], bm)
        assert torch.equal(ours.state[p]["exp_avg_sq"], bv)
    assert torch.equal(ours._step_t, before_t)
    assert float(skip) == 1.0  # once per step, not once per group
    ours.step(guard=torch.tensor(float("nan")), skip_count=skip)
    assert float(skip) == 2.0
    assert torch.equal(ours._step_t, before_t)
    # the next finite step is torch's next step: t was not advanced
    _set_grads(p2, gs)
    ours.step(guard=torch.tensor(2.0), skip_count=skip)
    ref.step()
    assert float(skip) == 2.0
    assert float(ours._step_t) == 2.0
    for a, b in zip(p1, p2):
        torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL)


def test_adamw_guard_first_step_is_t1():
    """Skipped very first step, then a finite one: equals torch's t = 1."""
    init = _params(4)
    p1, p2 = _leaf(init), _leaf(init)
    ours = AdamW(_groups(p1, 0.1, 0.0), lr=1e-2)
    ref = torch.optim.AdamW(_groups(p2, 0.1, 0.0), lr=1e-2)
    gs = _grads(4, 0)
    _set_grads(p1, gs)
    _set_grads(p2, gs)
    skip = torch.zeros(())
    ours.step(guard=torch.tensor(float("inf")), skip_count=skip)
    for p, i in zip(p1, init):
        assert torch.equal(p.detach(), i)
        assert not ours.state[p]["exp_avg"].any()
        assert not ours.state[p]["exp_avg_sq"].any()
    assert float(ours._step_t) == 0.0
    assert float(skip) == 1.0
    ours.step(guard=torch.tensor(1.0), skip_count=skip)
    ref.step()
    assert float(skip) == 1.0
    assert float(ours._step_t) == 1.0
    for a, b in zip(p1, p2):
        torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL)


def test_adamw_lr_tensor_overrides_group_lr():
    init = _params(5)
    p1, p2 = _leaf(init), _leaf(init)
    ours = AdamW(_groups(p1, 0.1, 0.0), lr=99.0)
    ref = torch.optim.AdamW(_groups(p2, 0.1, 0.0), lr=0.25)
    gs = _grads(5, 0)
    _set_grads(p1, gs)
    _set_grads(p2, gs)
    ours.step(lr_tensor=torch.tensor(0.25))
    ref.step()
    for a, b in zip(p1, p2):
        torch.testing.assert_close(a, b, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16_master"])
def test_adamw_checkpoint_roundtrip(dtype):
    master = dtype != torch.float32
    kw = dict(lr=1e-2, master_weights=master)
    init = _params(6, dtype)

    def run(ps, opt, steps):
        for s in steps:
            _set_grads(ps, _grads(6, s, dtype))
            opt.step()

    pa = _leaf(init)
    unbroken = AdamW(_groups(pa, 0.1, 0.0), **kw)
    run(pa, unbroken, range(5))

    pb = _leaf(init)
    first = AdamW(_groups(pb, 0.1, 0.0), **kw)
    run(pb, first, range(3))
    buf = io.BytesIO()
    torch.save(first.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu", weights_only=True)

    pc = _leaf([p.detach() for p in pb])  # the model weights, as model.bin
    second = AdamW(_groups(pc, 0.1, 0.0), **kw)
    second.load_state_dict(sd)
    assert second._step_t.dtype == torch.float32
    assert float(second._step_t) == 3.0
    for p in pc:
        st = second.state[p]
        for k in ("exp_avg", "exp_avg_sq") + (("master",) if master else ()):
            assert st[k].dtype == torch.float32, k
            assert st[k].device == p.device
    run(pc, second, range(3, 5))
    assert float(second._step_t) == 5.0
    for a, c in zip(pa, pc):
        assert torch.equal(a.detach(), c.detach())
        for k in ("exp_avg", "exp_avg_sq") + (("master",) if master else ()):
            assert torch.equal(unbroken.state[a][k], second.state[c][k]), k


def test_sgd_checkpoint_still_loads_into_sgd():
    from pytorch_ddp_template_amd.optim import SGD

    p = _leaf(_params(7))
    opt = SGD(p, lr=0.1, momentum=0.9)
    _set_grads(p, _grads(7, 0))
    opt.step()
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"}
    opt2 = SGD(p, lr=0.1, momentum=0.9)
    opt2.load_state_dict(sd)
    for q in p:
        assert torch.equal(opt.state[q]["momentum_buffer"],
                           opt2.state[q]["momentum_buffer"])


def _check_no_decay_groups(model, extra_names):
    groups = param_groups_no_decay(model, 0.05)
    assert len(groups) == 2
    by_wd = {g["weight_decay"]: g["params"] for g in groups}
    assert set(by_wd) == {0.05, 0.0}
    decay = {id(p) for p in by_wd[0.05]}
    no_decay = {id(p) for p in by_wd[0.0]}
    n_seen = len(by_wd[0.05]) + len(by_wd[0.0])
    assert len(decay) + len(no_decay) == n_seen  # no duplicates in a group
    assert not decay & no_decay
    named = dict(model.named_parameters())
    assert n_seen == len(named)  # each parameter exactly once
    for name, p in named.items():
        if p.ndim <= 1 or name in extra_names:
            assert id(p) in no_decay, name
        else:
            assert id(p) in decay, name
    assert decay and no_decay


def test_param_groups_no_decay_vit():
    from pytorch_ddp_template_amd.models.vit import ViT

    m = ViT(image_size=32, patch_size=8, dim=64, depth=2, heads=4,
            num_classes=10)
    assert m.no_weight_decay() == {"cls_token", "pos_embed"}
    assert m.cls_token.ndim > 1 and m.pos_embed.ndim > 1
    _check_no_decay_groups(m, {"cls_token", "pos_embed"})


def test_param_groups_no_decay_resnet18():
    from pytorch_ddp_template_amd.models import resnet18

    _check_no_decay_groups(resnet18(), set())


# ---------------------------------------------------------------- engine ----


def _make_args(tmp_path, extra=()):
    from pytorch_ddp_template_amd.ddp import build_parser

    args = build_parser().parse_args(
        ["--no_cuda", "--output_dir", str(tmp_path / "outputs"),
         "--dataset_size", "256", "--max_steps", "4", "--logging_steps", "2",
         "--save_steps", "2", "--no_tensorboard", *extra]
    )
    args.dataset = args.dataset or args.model
    return args


def test_parser_optimizer_flags():
    from pytorch_ddp_template_amd.ddp import build_parser

    args = build_parser().parse_args([])
    assert args.optimizer == "sgd"
    assert args.adam_beta1 == 0.9
    assert args.adam_beta2 == 0.999
    assert args.adam_epsilon == 1e-8
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--optimizer", "lamb"])


def test_engine_adamw_checkpoints_and_resumes(tmp_path):
    from pytorch_ddp_template_amd.ddp import cleanup, setup, train
    from pytorch_ddp_template_amd.models import build_model

    extra = ["--optimizer", "adamw", "--weight_decay", "0.05"]
    args = _make_args(tmp_path, extra)
    setup(args)
    gs, avg = train(args, build_model("foo"))
    assert gs == 4 and avg == avg
    sd = torch.load(
        os.path.join(args.output_dir, "checkpoint-2", "optimizer.pt"),
        map_location="cpu", weights_only=True,
    )
    assert sd["state"], "no optimizer state saved"
    for st in sd["state"].values():
        assert "exp_avg" in st and "exp_avg_sq" in st
    assert float(sd["step"]) == 2.0
    assert sorted(g["weight_decay"] for g in sd["param_groups"]) == [0.0, 0.05]
    cleanup(args)

    args2 = _make_args(tmp_path, extra)
    args2.global_step = 2
    args2.max_steps = 6
    setup(args2)
    gs, avg = train(args2, build_model("foo"))
    assert gs == 6 and avg == avg
    sd = torch.load(
        os.path.join(args2.output_dir, "checkpoint-6", "optimizer.pt"),
        map_location="cpu", weights_only=True,
    )
    assert float(sd["step"]) == 6.0  # 2 restored + 4 resumed steps
    cleanup(args2)
