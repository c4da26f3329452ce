"""Fused ResNet BasicBlock — one autograd node for conv1→bn1(relu)→conv2→bn2
(+ optional 1x1 downsample) → add+relu.

Why (measured on MI355X, ResNet-18/CIFAR bf16 step profile):
* the conv epilogue already holds its output tile in registers, so it emits
  the BN per-block partial sums for free (``conv2d_fwd_stats``) — the BN
  stats pass that re-read every conv output disappears;
* BN backward applies the downstream ReLU mask inline (``bn_bwd(y_relu=·)``)
  — no relu_bwd pass;
* the residual add + final ReLU ride in the last BN's normalize epilogue
  (``bn_fwd_ws(addend=·)``) — the separate add_relu pass disappears;
* the backward-side equivalent: the skip-grad accumulation and the
  block-input ReLU mask ride in the store phase of the block's last dgrad
  (``conv2d_dgrad(addend=·, out_mask=·)``) — the separate ``add_`` pass and
  the next-upstream block's ``relu_bwd`` pass disappear.  An earlier attempt
  at the add lost (+200 us/launch) because the kernel of that time, the NT
  GEMM, had to gather the addend per lane in 2-B pieces in the MFMA C/D
  layout.  The dgrads now run on the glds conv kernel, whose epilogue
  already stages the tile through LDS and stores coalesced 16-B row chunks;
  addend and mask are read with that same pattern, after the accumulator is
  rounded to bf16, so the result is bit-identical to the separate passes;
* the backward mirror of the forward stats epilogue (``PDT_DGRAD_BNSTATS``,
  below): the dgrad that produces ``dz`` for an in-block BN with a ReLU
  (``bn1`` of a BasicBlock, ``bn1``/``bn2`` of a Bottleneck) applies that
  ReLU's mask in its store phase and accumulates the BN's backward sums
  (sum dz, sum dz*xhat per channel) there (``conv2d_dgrad_bnstats``).  The
  BN backward then runs only its finalize and a two-tensor dx pass
  (``bn_bwd_ws``): the three-tensor stats pass disappears and the dx pass no
  longer reads the ReLU output.  Where the glds kernel declines the shape no
  workspace comes back and ``bn_bwd`` runs on the already-masked ``dz``.

ReLU-mask handshake between adjacent blocks (``PDT_DGRAD_EPILOGUE``, below):
a block's output is ``relu(·)``, and its backward starts by masking ``dy``
with ``out > 0``.  When the block downstream consumed exactly that output
through this fused path, it applies the mask itself (its ``x`` IS this
``out``) in its dgrad epilogue, and this block skips its ``relu_bwd``.  The
agreement is made per forward call on the producer's autograd node
(``dy_premasked``): the producer offers it only when ``ResNet`` wired it to a
following block, the consumer accepts only when its input's ``grad_fn`` is
such an offering node.  A consumer on the unfused module path never accepts,
so its producer masks as before; a standalone block neither offers nor
accepts.  The wiring assumes the producer's output has no other consumer
(true for the ``nn.Sequential`` layers of ``models/resnet.py``).

The unfused module path (ops/modules.py) remains the CPU/eval/odd-shape
reference; tests compare the two.  Reference scope note: the reference
template has no conv/BN at all (these ops come from the
BASELINE.json ResNet configs).
"""

from __future__ import annotations

import os

import torch

from .native import native

# Weight-gradient GEMMs can run on a second HIP stream, co-resident with the
# dgrad/BN-dx chain.  Measured on ResNet-18/CIFAR bf16: the serial stream is
# already 99% kernel-busy and co-scheduling LOST ~4%, so this defaults OFF
# (PDT_FUSED_STREAMS=1 opts in; kept for sparser models / future shapes).
_side = None


def _side_stream():
    global _side
    if _side is None:
        _side = torch.cuda.Stream()
    return _side


def _use_streams():
    return os.environ.get("PDT_FUSED_STREAMS", "0") == "1"


def _use_dgrad_epilogue():
    # skip-grad add + input ReLU mask inside the dgrad store phase;
    # PDT_DGRAD_EPILOGUE=0 restores the separate add_ / relu_bwd passes
    # (A/B runs).  Read once per block forward; the backward follows it.
    return os.environ.get("PDT_DGRAD_EPILOGUE", "1") != "0"


def _use_dgrad_bnstats():
    # BN-backward sums from the dgrad store phase (module docstring);
    # PDT_DGRAD_BNSTATS=0 restores the separate bn_bwd stats pass (A/B runs).
    # Read once per block forward; the backward follows it.
    return os.environ.get("PDT_DGRAD_BNSTATS", "1") != "0"


def _dgrad_for_bn_relu(ext, bns, dy, w, stride, pad, H, W, t, z, mean, rstd):
    """dgrad of ``dy`` through the conv with weight ``w`` whose input was the
    output ``z`` of a BN+ReLU with BN input ``t``.  Returns (dz, ws, masked):
    with ``bns`` dz carries the ReLU mask, and ws the BN-backward sums when
    the glds kernel ran (else None)."""
    if not bns:
        return ext.conv2d_dgrad(dy, w, stride, pad, H, W), None, False
    dz, ws = ext.conv2d_dgrad_bnstats(dy, w, stride, pad, H, W, z, t, mean,
                                      rstd)
    return dz, ws, True


def _bn_relu_bwd(ext, dz, ws, masked, t, z, gamma, mean, rstd):
    """Backward of that BN+ReLU from what ``_dgrad_for_bn_relu`` returned."""
    if ws is not None:
        dt, dg, db = ext.bn_bwd_ws(_flat(dz), _flat(t), gamma, mean, rstd, ws)
    else:
        # masked without sums: another dgrad route ran and applied the mask
        dt, dg, db = ext.bn_bwd(_flat(dz), _flat(t), gamma, mean, rstd,
                                None if masked else _flat(z))
    return dt.reshape(t.shape), dg, db


def _accept_premask(x, accept, epi):
    """Consumer side of the handshake: True when this block will mask its
    returned dx by ``x > 0`` and has told x's producer so."""
    if not (accept and epi):
        return False
    fn = x.grad_fn
    if getattr(fn, "dy_premasked", None) is None:
        return False
    fn.dy_premasked = True
    return True


def _skip_grad_dgrad(ext, ctx, dyc, w, stride, pad, H, W, addend, x):
    """dx = dgrad(dyc, w) + addend, masked by x > 0 when this block agreed to
    (ctx.mask_in); fused into the dgrad epilogue unless gated off."""
    if ctx.epi:
        return ext.conv2d_dgrad(dyc, w, stride, pad, H, W, addend=addend,
                                out_mask=x if ctx.mask_in else None)
    # in-place in-house add (the skip grad rides the dgrad output buffer)
    return ext.add_(ext.conv2d_dgrad(dyc, w, stride, pad, H, W), addend)


def _flat(t):
    return t.reshape(-1, t.shape[-1])


class _FusedBasicBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(
        ctx, x, w1, g1, b1, w2, g2, b2, wd, gd, bd, bn1, bn2, bnd, stride,
        offer=False, mask_in=False, epi=False, bns=False,
    ):
        ext = native()
        # handshake state (module docstring): None = no offer made
        ctx.epi, ctx.mask_in, ctx.bns = epi, mask_in, bns
        ctx.dy_premasked = False if (offer and epi) else None
        x = x.contiguous()
        mom, eps = bn1.momentum, bn1.eps
        t1, ws1 = ext.conv2d_fwd_stats(x, w1, None, stride, 1, False)
        z2, mean1, rstd1 = ext.bn_fwd_ws(
            _flat(t1), g1, b1, ws1, bn1.running_mean, bn1.running_var,
            mom, eps, True,
        )
        z = z2.reshape(t1.shape)
        t2, ws2 = ext.conv2d_fwd_stats(z, w2, None, 1, 1, False)
        if wd is not None:
            td, wsd = ext.conv2d_fwd_stats(x, wd, None, stride, 0, False)
            idn2, meand, rstdd = ext.bn_fwd_ws(
                _flat(td), gd, bd, wsd, bnd.running_mean, bnd.running_var,
                mom, eps, False,
            )
            idn = idn2.reshape(td.shape)
        else:
            td = meand = rstdd = None
            idn = x
        # residual add + relu fused into bn2's normalize pass (one fewer
        # full-tensor read+write than a separate add_relu)
        out2, mean2, rstd2 = ext.bn_fwd_ws(
            _flat(t2), g2, b2, ws2, bn2.running_mean, bn2.running_var,
            mom, eps, True, _flat(idn.contiguous()),
        )
        out = out2.reshape(t2.shape)
        ctx.save_for_backward(
            x, w1, g1, t1, z, mean1, rstd1, w2, g2, t2, mean2, rstd2,
            wd, gd, td, meand, rstdd, out,
        )
        ctx.stride = stride
        return out

    @staticmethod
    def backward(ctx, dy):
        (x, w1, g1, t1, z, mean1, rstd1, w2, g2, t2, mean2, rstd2,
         wd, gd, td, meand, rstdd, out) = ctx.saved_tensors
        stride = ctx.stride
        ext = native()
        dy = dy.contiguous()
        H, W = x.shape[1], x.shape[2]
        Hz, Wz = z.shape[1], z.shape[2]

        # apply the add_relu mask ONCE; bn2/bnd backwards then read two
        # tensors instead of three, and the skip grad is g itself.  When the
        # downstream block already masked dy in its dgrad epilogue, dy is g.
        g = dy if ctx.dy_premasked else ext.relu_bwd(dy, out)
        g2d = _flat(g)
        dx2, dg2, db2 = ext.bn_bwd(g2d, _flat(t2), g2, mean2, rstd2, None)
        dx2 = dx2.reshape(t2.shape)
        use_side = _use_streams()
        main = torch.cuda.current_stream()
        side = _side_stream() if use_side else None
        if use_side:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                dw2 = ext.conv2d_wgrad(dx2, z, 1, 1, 3, 3).to(w2.dtype)
        # conv2 backward dgrad stays on the critical path
        dz, ws1, masked = _dgrad_for_bn_relu(
            ext, ctx.bns, dx2, w2, 1, 1, Hz, Wz, t1, z, mean1, rstd1)
        if not use_side:
            dw2 = ext.conv2d_wgrad(dx2, z, 1, 1, 3, 3).to(w2.dtype)
        # bn1 backward (its own fused ReLU: z is bn1's relu output)
        dt1, dg1, db1 = _bn_relu_bwd(ext, dz, ws1, masked, t1, z, g1, mean1,
                                     rstd1)
        if use_side:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                dw1 = ext.conv2d_wgrad(dt1, x, stride, 1, 3, 3).to(w1.dtype)
        else:
            dw1 = ext.conv2d_wgrad(dt1, x, stride, 1, 3, 3).to(w1.dtype)

        if wd is None:
            dx = _skip_grad_dgrad(ext, ctx, dt1, w1, stride, 1, H, W, g, x)
            dwd = dgd = dbd = None
        else:
            dxa = ext.conv2d_dgrad(dt1, w1, stride, 1, H, W)
            dtd, dgd, dbd = ext.bn_bwd(g2d, _flat(td), gd, meand, rstdd, None)
            dtd = dtd.reshape(td.shape)
            if use_side:
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    dwd = ext.conv2d_wgrad(dtd, x, stride, 0, 1, 1).to(wd.dtype)
            else:
                dwd = ext.conv2d_wgrad(dtd, x, stride, 0, 1, 1).to(wd.dtype)
            dx = _skip_grad_dgrad(ext, ctx, dtd, wd, stride, 0, H, W, dxa, x)
        if use_side:
            # weight grads are consumed (bucket accumulation) on the main
            # stream after this node returns
            main.wait_stream(side)
            for t in (dw2, dw1) + ((dwd,) if wd is not None else ()):
                t.record_stream(main)
        return (dx, dw1, dg1, db1, dw2, dg2, db2, dwd, dgd, dbd,
                None, None, None, None, None, None, None, None)


def fused_basic_block(x, conv1, bn1, conv2, bn2, convd, bnd, stride,
                      offer=False, accept=False):
    """Run a BasicBlock through the fused Function (training, native path).

    offer / accept: this block's output feeds / its input comes from an
    adjacent wired block (ReLU-mask handshake, module docstring)."""
    epi = _use_dgrad_epilogue()
    mask_in = _accept_premask(x, accept, epi)
    bns = _use_dgrad_bnstats()
    return _FusedBasicBlockFn.apply(
        x, conv1.weight, bn1.weight, bn1.bias,
        conv2.weight, bn2.weight, bn2.bias,
        convd.weight if convd is not None else None,
        bnd.weight if bnd is not None else None,
        bnd.bias if bnd is not None else None,
        bn1, bn2, bnd, stride, offer, mask_in, epi, bns,
    )


class _FusedBottleneckFn(torch.autograd.Function):
    """ResNet Bottleneck (1x1 -> 3x3(s) -> 1x1, + optional 1x1(s) downsample)
    as one autograd node, same fusions as the BasicBlock variant."""

    @staticmethod
    def forward(ctx, x, w1, g1, b1, w2, g2, b2, w3, g3, b3, wd, gd, bd,
                bn1, bn2, bn3, bnd, stride,
                offer=False, mask_in=False, epi=False, bns=False):
        ext = native()
        ctx.epi, ctx.mask_in, ctx.bns = epi, mask_in, bns
        ctx.dy_premasked = False if (offer and epi) else None
        x = x.contiguous()
        mom, eps = bn1.momentum, bn1.eps
        t1, ws1 = ext.conv2d_fwd_stats(x, w1, None, 1, 0, False)
        z1f, mean1, rstd1 = ext.bn_fwd_ws(
            _flat(t1), g1, b1, ws1, bn1.running_mean, bn1.running_var,
            mom, eps, True)
        z1 = z1f.reshape(t1.shape)
        t2, ws2 = ext.conv2d_fwd_stats(z1, w2, None, stride, 1, False)
        z2f, mean2, rstd2 = ext.bn_fwd_ws(
            _flat(t2), g2, b2, ws2, bn2.running_mean, bn2.running_var,
            mom, eps, True)
        z2 = z2f.reshape(t2.shape)
        t3, ws3 = ext.conv2d_fwd_stats(z2, w3, None, 1, 0, False)
        if wd is not None:
            td, wsd = ext.conv2d_fwd_stats(x, wd, None, stride, 0, False)
            idnf, meand, rstdd = ext.bn_fwd_ws(
                _flat(td), gd, bd, wsd, bnd.running_mean, bnd.running_var,
                mom, eps, False)
            idn = idnf.reshape(td.shape)
        else:
            td = meand = rstdd = None
            idn = x
        # residual add + relu fused into bn3's normalize pass
        out3, mean3, rstd3 = ext.bn_fwd_ws(
            _flat(t3), g3, b3, ws3, bn3.running_mean, bn3.running_var,
            mom, eps, True, _flat(idn.contiguous()))
        out = out3.reshape(t3.shape)
        ctx.save_for_backward(
            x, w1, g1, t1, z1, mean1, rstd1, w2, g2, t2, z2, mean2, rstd2,
            w3, g3, t3, mean3, rstd3, wd, gd, td, meand, rstdd, out)
        ctx.stride = stride
        return out

    @staticmethod
    def backward(ctx, dy):
        (x, w1, g1, t1, z1, mean1, rstd1, w2, g2, t2, z2, mean2, rstd2,
         w3, g3, t3, mean3, rstd3, wd, gd, td, meand, rstdd, out) = (
            ctx.saved_tensors)
        stride = ctx.stride
        ext = native()
        dy = dy.contiguous()
        H, W = x.shape[1], x.shape[2]
        H1, W1 = z1.shape[1], z1.shape[2]
        H2, W2 = z2.shape[1], z2.shape[2]

        g = dy if ctx.dy_premasked else ext.relu_bwd(dy, out)
        g2d = _flat(g)
        dx3, dg3, db3 = ext.bn_bwd(g2d, _flat(t3), g3, mean3, rstd3, None)
        dx3 = dx3.reshape(t3.shape)
        dz2, ws2, masked = _dgrad_for_bn_relu(
            ext, ctx.bns, dx3, w3, 1, 0, H2, W2, t2, z2, mean2, rstd2)
        dw3 = ext.conv2d_wgrad(dx3, z2, 1, 0, 1, 1).to(w3.dtype)

        dt2, dg2, db2 = _bn_relu_bwd(ext, dz2, ws2, masked, t2, z2, g2, mean2,
                                     rstd2)
        dz1, ws1, masked = _dgrad_for_bn_relu(
            ext, ctx.bns, dt2, w2, stride, 1, H1, W1, t1, z1, mean1, rstd1)
        dw2 = ext.conv2d_wgrad(dt2, z1, stride, 1, 3, 3).to(w2.dtype)

        dt1, dg1, db1 = _bn_relu_bwd(ext, dz1, ws1, masked, t1, z1, g1, mean1,
                                     rstd1)
        dw1 = ext.conv2d_wgrad(dt1, x, 1, 0, 1, 1).to(w1.dtype)

        if wd is None:
            dx = _skip_grad_dgrad(ext, ctx, dt1, w1, 1, 0, H, W, g, x)
            dwd = dgd = dbd = None
        else:
            dxa = ext.conv2d_dgrad(dt1, w1, 1, 0, H, W)
            dtd, dgd, dbd = ext.bn_bwd(g2d, _flat(td), gd, meand, rstdd, None)
            dtd = dtd.reshape(td.shape)
            dwd = ext.conv2d_wgrad(dtd, x, stride, 0, 1, 1).to(wd.dtype)
            dx = _skip_grad_dgrad(ext, ctx, dtd, wd, stride, 0, H, W, dxa, x)
        return (dx, dw1, dg1, db1, dw2, dg2, db2, dw3, dg3, db3,
                dwd, dgd, dbd, None, None, None, None, None,
                None, None, None, None)


def fused_bottleneck(x, conv1, bn1, conv2, bn2, conv3, bn3, convd, bnd,
                     stride, offer=False, accept=False):
    epi = _use_dgrad_epilogue()
    mask_in = _accept_premask(x, accept, epi)
    bns = _use_dgrad_bnstats()
    return _FusedBottleneckFn.apply(
        x, conv1.weight, bn1.weight, bn1.bias,
        conv2.weight, bn2.weight, bn2.bias,
        conv3.weight, bn3.weight, bn3.bias,
        convd.weight if convd is not None else None,
        bnd.weight if bnd is not None else None,
        bnd.bias if bnd is not None else None,
        bn1, bn2, bn3, bnd, stride, offer, mask_in, epi, bns,
    )
