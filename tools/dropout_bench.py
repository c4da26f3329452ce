"""Kernel time of the fused dropout kernels against the elementwise kernels
with the same traffic (profiles/r11_dropout.md).

bf16 [32*197, 768] and [32*197, 3072].  Cases: plain dropout (one read, one
write; yardstick gelu_fwd), dropout_add with the element mask and with both
masks (two reads, one write; yardstick add_relu_fwd).  Each figure is device
events around REPLAYS replays of a captured graph of LAUNCHES back-to-back
launches, so the host's launch rate is not in it; 5 repeats, the cases of a
shape alternating within every repeat.

    python tools/dropout_bench.py [--out result.json]
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pytorch_ddp_template_amd.ops import rng  # noqa: E402
from pytorch_ddp_template_amd.ops.native import native  # noqa: E402

LAUNCHES, REPLAYS, REPEATS = 50, 20, 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    ext = native()
    rng.manual_seed(1, 0)
    step = rng.step_scalar(dev)
    k0, k1 = rng.key()
    result = {"launches_per_window": LAUNCHES * REPLAYS, "shapes": {}}
    for shape in ((32 * 197, 768), (32 * 197, 3072)):
        x = torch.randn(shape, device=dev).to(torch.bfloat16)
        res = torch.randn(shape, device=dev).to(torch.bfloat16)
        inner = shape[1] * 197  # one row of the row mask = one sample
        n = x.numel()

        def drop(r, p, p_row):
            return lambda: ext.dropout_fwd(x, r, None, step, k0, k1, 5, 6, p,
                                           p_row, inner)

        cases = {
            "gelu_fwd": (lambda: ext.gelu_fwd(x), 2),
            "dropout": (drop(None, 0.1, 0.0), 2),
            "add_relu_fwd": (lambda: ext.add_relu_fwd(x, res), 3),
            "dropout_add_elem": (drop(res, 0.1, 0.0), 3),
            "dropout_add_elem_row": (drop(res, 0.1, 0.1), 3),
        }
        graphs = {}
        side = torch.cuda.Stream()
        for name, (fn, _) in cases.items():
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                for _ in range(LAUNCHES):
                    fn()
            g.replay()
            graphs[name] = g
        torch.cuda.synchronize()
        times = {name: [] for name in cases}
        names = list(cases)
        for rep in range(REPEATS):
            order = names if rep % 2 == 0 else names[::-1]
            for name in order:
                g = graphs[name]
                for _ in range(3):
                    g.replay()
                t0 = torch.cuda.Event(enable_timing=True)
                t1 = torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(REPLAYS):
                    g.replay()
                t1.record()
                torch.cuda.synchronize()
                times[name].append(
                    t0.elapsed_time(t1) * 1e3 / (LAUNCHES * REPLAYS))  # us
        rows = {}
        for name, (_, passes) in cases.items():
            us = times[name]
            nbytes = passes * n * 2
            rows[name] = {
                "us": us, "us_min": min(us), "us_max": max(us),
                "bytes": nbytes,
                "gbps_min": nbytes / max(us) / 1e3,
                "gbps_max": nbytes / min(us) / 1e3,
            }
        for name, base in (("dropout", "gelu_fwd"),
                           ("dropout_add_elem", "add_relu_fwd"),
                           ("dropout_add_elem_row", "add_relu_fwd")):
            r = [a / b for a, b in zip(times[name], times[base])]
            rows[name]["ratio_to"] = base
            rows[name]["ratio"] = r
        result["shapes"]["x".join(map(str, shape))] = rows
        for name, r in rows.items():
            extra = ""
            if "ratio" in r:
                extra = (f"  ratio to {r['ratio_to']} "
                         f"{min(r['ratio']):.3f}..{max(r['ratio']):.3f}")
            print(f"{shape} {name:22s} us "
                  + ", ".join(f"{v:.2f}" for v in r["us"])
                  + f"  GB/s {r['gbps_min']:.0f}..{r['gbps_max']:.0f}" + extra)
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
