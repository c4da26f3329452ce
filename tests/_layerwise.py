"""Shared by the LARS / LAMB tests: the cases, the optimizers under test and
the float64 reference of the two rules.

A case is a list of tensors: the given sizes, then an all-zero tensor of 130
(weight norm 0, r = 1), a tensor of 130 whose gradient is always zero
(gradient norm 0), and one tensor of 515 that forms a second param group with
``layer_adapt=False, weight_decay=0`` (r = 1 by the group).  eta = 0.5 keeps
LARS's ratios near 1, so that the adapting tensors' updates are of the size of
the non-adapting one's and an error in a ratio shows in the compared maximum.
"""

import torch

# every path of an 8192-element chunk with a four-wide body (test_gpu_adamw)
SIZES = [1, 3, 130, 8192, 8197, 24580]
MANY = [7] * 520 + [8197]  # more than the 512 tensors of one plan
KW = dict(lr=1e-2, weight_decay=0.1)
RULES = {
    "lars": dict(momentum=0.9, trust_coef=0.5),
    "lars_nesterov": dict(momentum=0.9, nesterov=True, trust_coef=0.5),
    "lamb": dict(trust_ratio=True),
}
B1, B2, EPS = 0.9, 0.999, 1e-8  # AdamW's defaults


def case(sizes, seed, steps, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    sizes = list(sizes) + [130, 130, 515]
    init = [torch.randn(n, generator=gen).to(dtype) for n in sizes]
    init[-3].zero_()
    grads = []
    for _ in range(steps):
        gs = [torch.randn(n, generator=gen).to(dtype) for n in sizes]
        gs[-2].zero_()
        grads.append(gs)
    return init, grads


def make(rule, init, device="cpu", dtype=torch.float32, master=False):
    from pytorch_ddp_template_amd.optim import SGD, AdamW

    ps = [t.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
          for t in init]
    groups = [{"params": ps[:-1]},
              {"params": ps[-1:], "layer_adapt": False, "weight_decay": 0.0}]
    cls = AdamW if rule == "lamb" else SGD
    return cls(groups, master_weights=master, **KW, **RULES[rule]), ps


def set_grads(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = g.to(device=p.device, dtype=p.dtype).clone()


def run(rule, init, grads, **kw):
    opt, ps = make(rule, init, **kw)
    for gs in grads:
        set_grads(ps, gs)
        opt.step()
    return opt, ps


def _cat(ts):
    return torch.cat([t.detach().reshape(-1).cpu() for t in ts])


def flat(opt, ps, init):
    """Moments and the fp32 working weight's change, flattened."""
    st = [opt.state[p] for p in ps]
    work = [s.get("master", p) for s, p in zip(st, ps)]
    out = {"update": _cat([w.detach().cpu().float() - i.float()
                           for w, i in zip(work, init)])}
    for k in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
        if k in st[0]:
            out[k] = _cat([s[k] for s in st])
    return out


def reference(rule, init, grads):
    """The two rules in float64, damp = 0."""
    lamb = rule == "lamb"
    lr, mu = KW["lr"], RULES[rule].get("momentum")
    eta, nesterov = RULES[rule].get("trust_coef"), RULES[rule].get("nesterov")
    w = [t.double() for t in init]
    m = [torch.zeros_like(t) for t in w]
    v = [torch.zeros_like(t) for t in w]
    for t, gs in enumerate(grads, 1):
        for i, g in enumerate(gs):
            g = g.double()
            adapt = i < len(w) - 1
            wd = KW["weight_decay"] if adapt else 0.0
            wn = w[i].norm()
            if lamb:
                m[i] = B1 * m[i] + (1 - B1) * g
                v[i] = B2 * v[i] + (1 - B2) * g * g
                u = (m[i] / (1 - B1 ** t)) / (
                    (v[i] / (1 - B2 ** t)).sqrt() + EPS) + wd * w[i]
                ok = adapt and wn > 0 and u.norm() > 0
                w[i] = w[i] - lr * (wn / u.norm() if ok else 1.0) * u
            else:
                gn = g.norm()
                ok = adapt and wn > 0 and gn > 0
                d = (eta * wn / (gn + wd * wn) if ok else 1.0) * (g + wd * w[i])
                m[i] = mu * m[i] + d
                w[i] = w[i] - lr * (d + mu * m[i] if nesterov else m[i])
    out = {"update": _cat([a - b.double() for a, b in zip(w, init)])}
    if lamb:
        out.update(exp_avg=_cat(m), exp_avg_sq=_cat(v))
    else:
        out["momentum_buffer"] = _cat(m)
    return out
