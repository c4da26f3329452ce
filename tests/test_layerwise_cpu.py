"""LARS / LAMB on the CPU path: the rules against the float64 reference, the
unchanged defaults, old checkpoints, the two flags and the engine path."""

import copy
import os

import pytest
import torch

from _layerwise import RULES, SIZES, case, flat, reference, run, set_grads
from pytorch_ddp_template_amd.optim import SGD, AdamW


@pytest.mark.parametrize("rule", list(RULES))
def test_cpu_path_matches_float64_reference(rule):
    init, grads = case(SIZES[:4], 0, 3)
    got = flat(*run(rule, init, grads), init)
    ref = reference(rule, init, grads)
    assert set(got) == set(ref)
    wmax = max(float(t.abs().max()) for t in init) + float(ref["update"].abs().max())
    for k, r in ref.items():
        # the weight is rounded to fp32 once per step (2^-24 |w|, doubled for
        # the step's own arithmetic); a moment is a few fp32 operations
        tol = (len(grads) * 2.0 ** -23 * wmax if k == "update"
               else 16 * 2.0 ** -24 * float(r.abs().max()))
        assert (got[k].double() - r).abs().max() <= tol, k


@pytest.mark.parametrize("name", ["sgd", "adamw"])
def test_defaults_are_the_plain_optimizers_and_old_state_loads(name):
    ours, theirs, kw = {
        "sgd": (SGD, torch.optim.SGD, dict(momentum=0.9, nesterov=True)),
        "adamw": (AdamW, torch.optim.AdamW, {}),
    }[name]
    init, grads = case([130, 7], 1, 3)
    pa = [t.clone().requires_grad_(True) for t in init]
    pb = [t.clone().requires_grad_(True) for t in init]
    a = ours(pa, lr=1e-2, weight_decay=0.1, **kw)
    b = theirs(pb, lr=1e-2, weight_decay=0.1, **kw)
    g = a.param_groups[0]
    assert g["layer_adapt"] is True
    assert g["trust_coef"] == 0.0 if name == "sgd" else g["trust_ratio"] is False
    for gs in grads[:2]:
        set_grads(pa, gs)
        set_grads(pb, gs)
        a.step()
        b.step()
    for x, y in zip(pa, pb):
        if name == "sgd":  # the same torch ops in the same order
            assert torch.equal(x, y)
        else:  # test_adamw_cpu's tolerances
            torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-6)
    # a state dict from before the new keys loads and steps as before
    sd = copy.deepcopy(a.state_dict())
    for grp in sd["param_groups"]:
        for k in ("trust_coef", "trust_ratio", "layer_adapt"):
            grp.pop(k, None)
    pc = [p.detach().clone().requires_grad_(True) for p in pa]
    c = ours(pc, lr=1e-2, weight_decay=0.1, **kw)
    c.load_state_dict(sd)
    assert "layer_adapt" not in c.param_groups[0]
    set_grads(pa, grads[2])
    set_grads(pc, grads[2])
    a.step()
    c.step()
    for x, y in zip(pa, pc):
        assert torch.equal(x, y)


def test_parser_trust_flags():
    from pytorch_ddp_template_amd.ddp import build_parser

    args = build_parser().parse_args([])
    assert args.trust_ratio is False and args.trust_coef == 0.001
    args = build_parser().parse_args(["--trust_ratio", "--trust_coef", "0.02"])
    assert args.trust_ratio is True and args.trust_coef == 0.02
    for action in build_parser()._actions:
        if action.dest == "optimizer":
            assert tuple(action.choices) == ("sgd", "adamw")


@pytest.mark.parametrize("name", ["sgd", "adamw"])
def test_engine_trust_ratio_checkpoints_and_resumes(tmp_path, name):
    from pytorch_ddp_template_amd.ddp import build_parser, cleanup, setup, train
    from pytorch_ddp_template_amd.models import build_model

    def go(max_steps, global_step):
        args = build_parser().parse_args(
            ["--no_cuda", "--output_dir", str(tmp_path / "outputs"),
             "--dataset_size", "256", "--max_steps", str(max_steps),
             "--logging_steps", "2", "--save_steps", "2", "--no_tensorboard",
             "--model", "foo", "--optimizer", name, "--trust_ratio",
             "--weight_decay", "0.05", "--momentum", "0.9"])
        args.dataset = args.dataset or args.model
        args.global_step = global_step
        setup(args)
        gs, avg = train(args, build_model("foo"))
        cleanup(args)
        assert gs == max_steps and avg == avg
        return torch.load(
            os.path.join(args.output_dir, f"checkpoint-{max_steps}",
                         "optimizer.pt"),
            map_location="cpu", weights_only=True)

    sd = go(4, 0)
    decay, no_decay = sd["param_groups"]
    assert decay["weight_decay"] == 0.05 and decay["layer_adapt"] is True
    assert no_decay["weight_decay"] == 0.0 and no_decay["layer_adapt"] is False
    if name == "adamw":
        assert decay["trust_ratio"] is True and float(sd["step"]) == 4.0
    else:
        assert decay["trust_coef"] == 0.001
    sd = go(6, 4)
    assert len(sd["state"]) == len(decay["params"]) + len(no_decay["params"])
    if name == "adamw":
        assert float(sd["step"]) == 6.0  # 4 restored + 2 resumed steps
