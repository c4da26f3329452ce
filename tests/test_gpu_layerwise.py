"""LARS (optim.SGD, trust_coef) and LAMB (optim.AdamW, trust_ratio) on the
GPU: mt::{lars,lamb}_{norm,apply}_kernel and mt::layer_ratio_kernel.

Numbers are checked with _errbound.assert_calibrated: ``gpu`` is the kernels,
``cpu`` the project's CPU fp32 path, ``ref`` the float64 rules of
_layerwise.reference.  Compared are the moments and the change of the fp32
working weight.  The sums of all three stages have one fixed order, so two
runs, and a captured and an eager run, must agree bit for bit.
"""

import pytest
import torch

from _errbound import assert_calibrated
from _layerwise import MANY, RULES, SIZES, case, flat, make, reference, run, set_grads

pytestmark = pytest.mark.gpu

DEV = "cuda"
STATE = ("momentum_buffer", "exp_avg", "exp_avg_sq")


def _bits(opt, ps):
    out = [p.detach().clone() for p in ps]
    for p in ps:
        out += [opt.state[p][k].clone() for k in STATE + ("master",)
                if k in opt.state[p]]
    return out


def _calibrated(name, rule, init, grads, opt, ps):
    cpu_opt, cpu_ps = run(rule, [t.float() for t in init], grads)
    assert_calibrated(name, flat(opt, ps, init),
                      flat(cpu_opt, cpu_ps, init), reference(rule, init, grads))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16],
                         ids=["fp32", "bf16_master", "fp16_master"])
@pytest.mark.parametrize("rule", list(RULES))
def test_rule_matches_float64_reference(rule, dtype):
    master = dtype != torch.float32
    init, grads = case(SIZES, 0, 3, dtype)
    opt, ps = run(rule, init, grads, device=DEV, dtype=dtype, master=master)
    for p in ps:
        st = opt.state[p]
        assert all(st[k].dtype == torch.float32 for k in STATE if k in st)
        if master:
            assert p.dtype == dtype
            assert torch.equal(p.detach(), st["master"].to(dtype))
    _calibrated(f"{rule}_{dtype}".replace("torch.", ""), rule, init, grads,
                opt, ps)


@pytest.mark.parametrize("sizes", [SIZES, MANY], ids=["sizes", "two_plans"])
@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_two_runs_are_bit_equal(rule, sizes):
    init, grads = case(sizes, 1, 3)
    a = run(rule, init, grads, device=DEV)
    b = run(rule, init, grads, device=DEV)
    for x, y in zip(_bits(*a), _bits(*b)):
        assert torch.equal(x, y)
    if sizes is MANY:
        _calibrated(f"{rule}_two_plans", rule, init, grads, *a)


@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_guard_skips_whole_step_and_ticks_once(rule):
    # two groups, the first of them two plans
    init, grads = case(MANY, 2, 2)
    opt, ps = run(rule, init, grads[:1], device=DEV)
    before = _bits(opt, ps)
    t0 = opt._step_t.clone() if rule == "lamb" else None
    skip = torch.zeros((), device=DEV)
    set_grads(ps, grads[1])
    opt.step(guard=torch.tensor(float("inf"), device=DEV), skip_count=skip)
    for x, y in zip(before, _bits(opt, ps)):
        assert torch.equal(x, y)
    assert float(skip) == 1.0
    opt.step(guard=torch.tensor(3.0, device=DEV), skip_count=skip)
    assert float(skip) == 1.0
    assert not torch.equal(before[0], ps[0].detach())
    if rule == "lamb":
        assert float(t0) == 1.0 and float(opt._step_t) == 2.0


@pytest.mark.parametrize("rule", ["lars", "lamb"])
def test_captured_step_equals_eager(rule):
    """test_gpu_adamw's recipe: warm-ups on a side stream, one capture of
    step(lr_tensor=...) on static grads, three replays with new grads and a
    new lr each, against an eager twin doing the same steps."""
    lrs = [1e-2, 2e-2, 5e-3, 3e-2]
    init, grads = case(SIZES, 3, len(lrs))
    (og, pg), (oe, pe) = make(rule, init, DEV), make(rule, init, DEV)
    for p in pg + pe:
        p.grad = torch.zeros_like(p)  # static grad tensors
    lr_g, lr_e = torch.zeros((), device=DEV), torch.zeros((), device=DEV)

    def feed(ps, lr_dev, s):
        for p, g in zip(ps, grads[s]):
            p.grad.copy_(g)
        lr_dev.fill_(lrs[s])

    for s in range(len(lrs)):
        feed(pe, lr_e, s)
        oe.step(lr_tensor=lr_e)

    side = torch.cuda.Stream()
    feed(pg, lr_g, 0)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        og.step(lr_tensor=lr_g)  # eager: builds the plans and the state
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        og.step(lr_tensor=lr_g)
    for s in range(1, len(lrs)):
        feed(pg, lr_g, s)
        graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(_bits(og, pg), _bits(oe, pe)):
        assert torch.equal(x, y)
